"""The diagnosis of a statement: include/gstark_diagnose.h, csrc/diagnose.hip (gs_nonzero_spans), csrc/diagnose.h (gs_prover_diagnose),
genstark_amd/diagnose.py, js/prover.js.  Every expected report comes from the host-integer model of tests/diagnose_cases.py.

CPU tier: the whole flow on the tests' double, which lacks gs_nonzero_spans (the driver scans on the host).  GPU tier: the kernel against
Python in three field flavours, and every statement again on the HIP library, interpreted and compiled."""
import ctypes as C
import json
import os
import subprocess

import pytest

import genstark_amd as ga
from genstark_amd import _abi, airassembly, lib128
from genstark_amd._abi import Backend, GstarkError
from genstark_amd.errors import StarkError
from genstark_amd.field import PrimeField
from genstark_amd.prover import Prover

import diagnose_cases as dc
from conftest import ORACLE_LIB, _build_oracle
from sponge_common import NODE, ROOT, check_header_is_plain_c, check_symbol_table, flavour_fixture, needs_node

AA = os.path.join(ROOT, 'tests', 'golden', 'aa')
LIB_OPTS = {'hashAlgorithm': 'blake2s256', 'extensionFactor': 32, 'exeQueryCount': 44, 'friQueryCount': 20}
LEDGER_OPTS = {'hashAlgorithm': 'sha256', 'exeQueryCount': 24, 'friQueryCount': 12}
MIMC_OPTS = {'hashAlgorithm': 'blake2s256', 'extensionFactor': 16, 'exeQueryCount': 48, 'friQueryCount': 24}


# ---- the statements, on any backend ----------------------------------------------------------------------------------------------------
def check_table(backend, prove=True):
    """the four statements of the issue's table"""
    f = PrimeField(backend=backend)
    # [3, 2]: proves, ok, degrees as the model's
    air = dc.table_air(f, [3, 2])
    a = dc.table_assertions(air)
    d = Prover(air, dc.OPTS).diagnose(a, None, dc.SEED)
    assert d.ok and str(d) == 'ok' and d.assertions == []
    assert dc.same(d.constraints, dc.model_report(air, dc.SEED))
    assert [c['degree'] for c in d.constraints] == [189, 63]
    if prove:
        assert Prover(air, dc.OPTS).prove_bytes(a, None, dc.SEED)
    # [3, 1]: every constraint holds on every step, and the statement does not prove: the linear constraint next to the cubic one
    air = dc.table_air(f, [3, 1])
    d = Prover(air, dc.OPTS).diagnose(a, None, dc.SEED)
    assert dc.same(d.constraints, dc.model_report(air, dc.SEED))
    assert [c['violations'] for c in d.constraints] == [0, 0] and not d.ok
    c1 = d.constraints[1]
    assert (c1['degree'], c1['limit'], c1['needed'], c1['declared'], c1['atLeast']) == (63, 62, 2, 1, False)
    assert str(d) == 'constraint 1: declared degree 1 allows degree 62, measured 63: declare 2'
    if prove:
        with pytest.raises(StarkError, match='Low degree proof failed'):
            Prover(air, dc.OPTS).prove_bytes(a, None, dc.SEED)
    # [2, 1]: constraint 0 is over its limit too
    air = dc.table_air(f, [2, 1])
    d = Prover(air, dc.OPTS).diagnose(a, None, dc.SEED)
    assert dc.same(d.constraints, dc.model_report(air, dc.SEED)) and not d.ok
    c0 = d.constraints[0]
    assert c0['degree'] == 189 and c0['degree'] > c0['limit'] == 126 and c0['needed'] == 3 and not c0['atLeast']
    # the evaluation drifted from the transition by k0 - 1
    check_drift(backend)


def check_drift(backend):
    f = PrimeField(backend=backend)
    air = dc.table_air(f, [3, 3], drift=True)
    d = Prover(air, dc.OPTS).diagnose(dc.table_assertions(air), None, dc.SEED)
    model = dc.model_report(air, dc.SEED)
    assert dc.same(d.constraints, model) and not d.ok
    c0, c1 = d.constraints
    assert (c1['violations'], c1['firstStep'], c1['lastStep']) == (47, 1, 62) and c1['firstValue'] == model[1]['firstValue'] != 0
    assert (c0['violations'], c0['firstStep'], c0['lastStep'], c0['firstValue']) == (0, 63, 63, 0)
    assert str(d).startswith('constraint 1: violated on 47 of 63 steps, first at step 1 ')
    return d


def check_assertions(backend):
    f = PrimeField(backend=backend)
    air = dc.table_air(f, [3, 2])
    trace = air.hostTrace(dc.SEED)
    a = [{'step': 5, 'register': 1, 'value': trace[5][1] + 1}, {'step': 0, 'register': 0, 'value': dc.SEED[0]},
         {'step': 63, 'register': 0, 'value': trace[63][0] ^ 1}]
    p = Prover(air, dc.OPTS)
    d = p.diagnose(a, None, dc.SEED)
    assert d.assertions == [{'index': 0, 'step': 5, 'register': 1, 'expected': trace[5][1] + 1, 'found': trace[5][1]},
                            {'index': 2, 'step': 63, 'register': 0, 'expected': trace[63][0] ^ 1, 'found': trace[63][0]}]
    assert not d.ok and all(c['violations'] == 0 for c in d.constraints) and len(str(d).splitlines()) == 2
    with pytest.raises(StarkError, match='Assertion at step 5, register 1 conflicts with execution trace'):      # prove names one
        p.prove_bytes(a, None, dc.SEED)


def merkle_update_statement(f, bad_bit):
    from test_lib128 import merkle_case
    depth, index = 2, 1
    old_value, new_value = (9, 10), (11, 12)
    tree, _, _, bits = merkle_case(f, depth, index)
    leaves = [tree.nodes[(1 << depth) + i] for i in range(1 << depth)]
    leaves[index] = old_value
    path = lib128.PoseidonMerkleTree(f, leaves).prove(index)
    if bad_bit:
        bits = list(bits)
        bits[1] = 2                                       # one index "bit" that is not binary
    air = lib128.compute_merkle_update_air(f, depth)
    inputs, first = lib128.merkle_update_inputs(f, old_value, new_value, path[1:], bits)
    return air, inputs, first


def check_merkle_update(backend):
    f = PrimeField(backend=backend)
    for bad_bit in (False, True):
        air, inputs, first = merkle_update_statement(f, bad_bit)
        model = dc.model_report(air, first, inputs, with_degrees=False)
        d = Prover(air, LIB_OPTS).diagnose([{'step': 0, 'register': 0, 'value': first[0]}], inputs, first)
        assert dc.same(d.constraints, model) and len(d.constraints) == 25
        violated = [c['index'] for c in d.constraints if c['violations']]
        if bad_bit:
            assert violated == [24] and not d.ok and model[24]['violations'] > 0
            assert all(c['allZero'] or c['degree'] <= c['limit'] for c in d.constraints if c['index'] != 24)
        else:
            assert violated == [] and d.ok, str(d)


def ledger_statement(f, runs=2):
    from test_airassembly import ledger_model
    stark = airassembly.instantiate(os.path.join(AA, 'ledger.aa'), 'default', LEDGER_OPTS, field=f)
    balances, factors = [100 + 7 * i for i in range(runs)], [3 + i for i in range(runs)]
    deposits = [[5 + i + 2 * j for j in range(4)] for i in range(runs)]
    inputs = [balances, factors, deposits]
    model = ledger_model(f.modulus, balances, factors, deposits)
    last = 8 * runs - 1
    assertions = [{'step': 0, 'register': 0, 'value': balances[0]}, {'step': last, 'register': 2, 'value': model[last][2]},
                  {'step': last, 'register': 0, 'value': model[last][0]}]
    return stark.air, inputs, assertions


def check_ledger(backend):
    f = PrimeField(backend=backend)
    air, inputs, assertions = ledger_statement(f)
    d = Prover(air, LEDGER_OPTS).diagnose(assertions, inputs)
    inner, packed, firsts, _shapes = air.plan(inputs, None)
    model = dc.model_report(inner, firsts, packed)
    assert dc.same(d.constraints, model), (d.constraints, model)
    assert d.ok and d.steps == 16 and [c['declared'] for c in d.constraints] == [3, 3, 5]


def check_mimc(backend):
    stark = ga.instantiateMimc(64, MIMC_OPTS, backend=backend)
    control = ga.runMimc(stark.air.field, 64, stark.air.roundConstants, 3)
    p = Prover(stark.air, MIMC_OPTS)
    good = [{'step': 0, 'register': 0, 'value': 3}, {'step': 63, 'register': 0, 'value': control[-1]}]
    d = p.diagnose(good, [], [3])
    assert d.ok and d.constraints == [] and d.assertions == []
    d = p.diagnose([good[0], dict(good[1], value=control[-1] + 1)], [], [3])
    assert not d.ok and d.constraints == []
    assert d.assertions == [{'index': 1, 'step': 63, 'register': 0, 'expected': control[-1] + 1, 'found': control[-1]}]


def message(exc):
    return str(exc.value).split(': ', 1)[1]


def check_invalid_jobs(backend):
    f = PrimeField(backend=backend)
    air = dc.table_air(f, [3, 2])
    p = Prover(air, dc.OPTS)
    for bad in ([{'step': 64, 'register': 0, 'value': 1}], [{'step': 0, 'register': 2, 'value': 1}]):
        with pytest.raises(StarkError) as want:
            p.prove_bytes(bad, None, dc.SEED)
        with pytest.raises(StarkError) as got:
            p.diagnose(bad, None, dc.SEED)
        assert message(got) == message(want) and 'Invalid assertion' in message(got)
    for call in (p.prove_bytes, p.diagnose):
        with pytest.raises(TypeError, match='At least one assertion'):
            call([], None, dc.SEED)
        with pytest.raises(TypeError, match='must be an array'):
            call(None, None, dc.SEED)
        with pytest.raises(ValueError, match='Invalid assertion'):
            call([{'step': -1, 'register': 0, 'value': 1}], None, dc.SEED)
    # (degrees that ask for a larger extension factor than the AIR has are refused by GenericAir itself: no job is made)
    # ... and the context is as usable as before
    assert p.diagnose(dc.table_assertions(air), None, dc.SEED).ok


# ---- CPU tier: the tests' double ----------------------------------------------------------------------------------------------------------
def test_header_is_plain_c_and_symbols_are_a_table_of_their_own():
    check_header_is_plain_c('diagnose')
    assert _abi.DIAGNOSE_SYMBOLS == ('gs_nonzero_spans',)
    check_symbol_table('diagnose', _abi.DIAGNOSE_SYMBOLS, (_abi.EXPORTED_SYMBOLS, _abi.OPTIONAL_SYMBOLS, _abi.HADES_SYMBOLS, _abi.RESCUE_SYMBOLS,
                                                            _abi.TREE_UPDATE_SYMBOLS, _abi.TREE_VERIFY_SYMBOLS, _abi.MIMC_SYMBOLS, _abi.CURVE_SYMBOLS))
    header = open(os.path.join(ROOT, 'include', 'gstark_diagnose.h')).read()
    assert 'gs_prover_diagnose(' in header and 'gs_prover_diagnose_on(' in header
    assert 'define GS_PROVER_ABI_VERSION 2' in open(os.path.join(ROOT, 'include', 'gstark_prover.h')).read()


def test_double_lacks_the_scan(oracle_backend):
    assert not hasattr(oracle_backend.lib, 'gs_nonzero_spans')          # what follows runs the driver's host scan


def test_table_statements_oracle(oracle_backend):
    check_table(oracle_backend)


def test_every_conflicting_assertion_oracle(oracle_backend):
    check_assertions(oracle_backend)


def test_merkle_update_index_bit_oracle(oracle_backend):
    check_merkle_update(oracle_backend)


def test_ledger_assembly_oracle(oracle_backend):
    check_ledger(oracle_backend)


def test_mimc_reports_assertions_only_oracle(oracle_backend):
    check_mimc(oracle_backend)


def test_invalid_jobs_raise_what_prove_raises_oracle(oracle_backend):
    check_invalid_jobs(oracle_backend)


def test_proof_bytes_unchanged_around_a_diagnosis_oracle(oracle_backend):
    from generic_cases import build, RESCUE_OPTS
    air, stark, seed, assertions = build('rescue_64', oracle_backend)
    p = Prover(air, RESCUE_OPTS)
    first = p.prove_bytes(assertions, None, seed)
    assert first == stark.serialize(stark.prove(assertions, [], seed))          # the mirror's bytes: the job construction moved, nothing else
    assert p.diagnose(assertions, None, seed).ok
    assert p.prove_bytes(assertions, None, seed) == first


def test_device_library_without_the_entry_says_so():
    be = Backend(lib_path=_build_oracle(), allow_test_double=True)
    be.name = 'hip-gfx950'                                               # a device backend whose library lacks only the entry
    try:
        f = PrimeField(backend=be)
        air = dc.table_air(f, [3, 2])
        with pytest.raises(GstarkError, match=r'no gs_nonzero_spans \(include/gstark_diagnose\.h\)'):
            Prover(air, dc.OPTS).diagnose(dc.table_assertions(air), None, dc.SEED)
    finally:
        be.close()


def js_cases(f):
    out = []
    for name, degrees, drift, wrong in (('declared_3_1', [3, 1], False, 0), ('drift', [3, 3], True, 0), ('assertion', [3, 2], False, 1)):
        air = dc.table_air(f, degrees, drift)
        a = dc.table_assertions(air)
        out.append({'name': name, 'generic': air.descriptor(), 'extension_factor': 16, 'seed': [str(v) for v in dc.SEED],
                    'assertions': [dict(x, value=str(x['value'] + wrong)) for x in a]})
    _air, inputs, assertions = ledger_statement(f)
    strs = lambda x: [strs(v) for v in x] if isinstance(x, list) else str(x)
    out.append({'name': 'ledger', 'source': open(os.path.join(AA, 'ledger.aa')).read(), 'component': 'default', 'options': LEDGER_OPTS,
                'inputs': strs(inputs), 'assertions': [dict(x, value=str(x['value'])) for x in assertions]})
    return out


def run_js_diagnose(f, mode, tmp_path):
    env = dict(os.environ)
    if mode == 'double':
        _build_oracle()
        env.update({'GSTARK_LIB': ORACLE_LIB, 'GSTARK_ALLOW_TEST_DOUBLE': '1'})
    subprocess.check_call(['bash', os.path.join(ROOT, 'napi', 'build.sh')], stdout=subprocess.DEVNULL)
    cases, out = tmp_path / 'cases.json', tmp_path / 'out.json'
    cases.write_text(json.dumps(js_cases(f)))
    r = subprocess.run(['timeout', '-k', '10', '240', NODE, os.path.join(ROOT, 'tests', 'js_diagnose.js'), str(cases), str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'js diagnose OK: 4 statements' in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(out.read_text())


def check_js(backend, mode, tmp_path):
    """js/prover.js: diagnoseGenericSerialized on the [3, 1] and the k0 - 1 statements returns the report the Python host returns"""
    f = PrimeField(backend=backend)
    got = run_js_diagnose(f, mode, tmp_path)
    for name, degrees, drift in (('declared_3_1', [3, 1], False), ('drift', [3, 3], True)):
        air = dc.table_air(f, degrees, drift)
        d = Prover(air, dc.OPTS).diagnose(dc.table_assertions(air), None, dc.SEED)
        assert dc.same(d.constraints, dc.model_report(air, dc.SEED))
        want = [{k: (str(v) if k == 'firstValue' else v) for k, v in c.items()} for c in d.constraints]
        assert got[name]['constraints'] == want and got[name]['assertions'] == [] and got[name]['ok'] is False
    air, inputs, assertions = ledger_statement(f)                        # an AssemblyAir with input registers: diagnoseAssemblySerialized
    d = Prover(air, LEDGER_OPTS).diagnose(assertions, inputs)
    want = [{k: (str(v) if k == 'firstValue' else v) for k, v in c.items()} for c in d.constraints]
    assert d.ok and got['ledger'] == {'ok': True, 'assertions': [], 'constraints': want}
    last = dc.table_air(f, [3, 2]).hostTrace(dc.SEED)[63][0]
    assert got['assertion']['assertions'] == [{'index': 0, 'step': 63, 'register': 0, 'expected': str(last + 1), 'found': str(last)}]
    assert got['assertion']['ok'] is False and all(c['violations'] == 0 for c in got['assertion']['constraints'])


@needs_node
def test_node_returns_the_same_report_oracle(oracle_backend, tmp_path):
    check_js(oracle_backend, 'double', tmp_path)


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------------
flavour = flavour_fixture('p128', 'q64', 'p224')
BITS = {_abi.MODULUS_128: 128, _abi.MODULUS_64: 64, _abi.MODULUS_224: 224}
SHAPES = [(1, 1, 1), (1, 64, 63), (3, 300, 257), (64, 8, 5), (2, 65544, 65539)]


def patterns(n):
    singles = [('0', 0), ('last', n - 1), ('63', 63), ('64', 64), ('255', 255), ('256', 256), ('mid', n // 2)]
    return ['zero', 'ones', 'lowbyte', 'highbyte', 'random'] + [f'single:{name}' for name, col in singles if col < n]


def spans(be, ptr, rows, stride, n):
    out = [(C.c_uint64 * rows)() for _ in range(3)]
    rc = be.lib.gs_nonzero_spans(be.ctx, C.c_void_p(ptr), rows, stride, n, *out)
    return rc, [list(o) for o in out]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_nonzero_spans_equals_python(flavour, shape):
    rows, stride, n = shape
    es, bits = flavour.element_size, BITS[flavour.modulus]
    ptr = flavour.alloc(rows * stride * es)
    try:
        for pattern in patterns(n):
            values, counts, firsts, lasts = dc.spans_reference(rows, stride, n, pattern, bits)
            flavour.upload(ptr, b''.join(v.to_bytes(es, 'little') for v in values))
            rc, got = spans(flavour, ptr, rows, stride, n)
            print(shape, pattern, rc, got[0][:4], got[1][:4], got[2][:4])
            assert rc == 0 and got == [counts, firsts, lasts], (shape, pattern)
    finally:
        flavour.free(ptr)


@pytest.mark.gpu
def test_nonzero_spans_refuses(flavour):
    es = flavour.element_size
    ptr = flavour.alloc(64 * es)
    one = (C.c_uint64 * 1)()
    try:
        flavour.upload(ptr, bytes(64 * es))
        for args, word in (((C.c_void_p(ptr), 0, 8, 8, one, one, one), '0 rows'), ((C.c_void_p(ptr), 1, 8, 0, one, one, one), '0 columns'),
                           ((C.c_void_p(ptr), 1, 8, 9, one, one, one), '9 columns to scan in rows of 8'), ((None, 1, 8, 8, one, one, one), 'required'),
                           ((C.c_void_p(ptr), 1, 8, 8, None, one, one), 'required'), ((C.c_void_p(ptr), 1, 8, 8, one, None, one), 'required'),
                           ((C.c_void_p(ptr), 1, 8, 8, one, one, None), 'required')):
            assert flavour.lib.gs_nonzero_spans(flavour.ctx, *args) != 0
            assert word in flavour.lib.gs_last_error(flavour.ctx).decode()
        rc, got = spans(flavour, ptr, 2, 32, 32)                                # the context works on
        assert rc == 0 and got == [[0, 0], [32, 32], [32, 32]]
    finally:
        flavour.free(ptr)


@pytest.mark.gpu
def test_statements_hip(hip_backend):
    assert hasattr(hip_backend.lib, 'gs_nonzero_spans')
    check_table(hip_backend)
    check_assertions(hip_backend)
    check_merkle_update(hip_backend)
    check_ledger(hip_backend)
    check_mimc(hip_backend)
    check_invalid_jobs(hip_backend)


@pytest.mark.gpu
@pytest.mark.parametrize('check', [check_drift, check_merkle_update], ids=['drift', 'merkle_update'])
def test_statements_hip_compiled_programs(check):
    """Backend.jit(True): the evaluator runs compiled, so what is checked is what prove runs.  (The time of the Merkle-update case is the
    one hiprtc build of its 25-constraint Poseidon evaluator; the honest and the non-binary statement share the code object.)"""
    be = Backend(device=0).jit(True)
    try:
        before = be.jit_launches
        check(be)
        assert be.jit_launches > before
    finally:
        be.close()


@pytest.mark.gpu
def test_small_generic_cases_are_ok_hip(hip_backend):
    from generic_cases import SMALL, build, RESCUE_OPTS
    for name in SMALL:
        air, _stark, seed, assertions = build(name, hip_backend)
        d = Prover(air, RESCUE_OPTS).diagnose(assertions, None, seed)
        assert d.ok, (name, str(d))
        assert all(c['violations'] == 0 and not c['atLeast'] for c in d.constraints)


@pytest.mark.gpu
def test_prove_diagnose_prove_on_one_context_hip(hip_backend):
    from generic_cases import build, RESCUE_OPTS
    air, _stark, seed, assertions = build('rescue_64', hip_backend)
    p = Prover(air, RESCUE_OPTS)
    first = p.prove_bytes(assertions, None, seed)
    assert p.diagnose(assertions, None, seed).ok
    bad = [dict(assertions[0], step=air.steps)]
    with pytest.raises(StarkError):
        p.diagnose(bad, None, seed)                                             # a throw leaves the context usable
    assert p.prove_bytes(assertions, None, seed) == first


@pytest.mark.gpu
@needs_node
def test_node_returns_the_same_report_hip(hip_backend, tmp_path):
    check_js(hip_backend, 'hip', tmp_path)
