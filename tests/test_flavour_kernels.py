"""The kernels that only the other field builds compile (or that change with the element size), at the plan edges: tests/flavour_cases.py
on the five fixed flavours q64, q32, q17, p256, p224 and, through tests/runtime_modulus_worker.py, on the runtime-modulus build.

CPU tier: every check on the oracle flavours (oracle/liboracle_<name>.so) — pins the checks and their Python references without a
GPU; the _BitInt flavours stop at 2^13-point transforms, 40 000 inversions and 2^9 leaves there.  GPU tier: the same checks on
Backend(device=0, modulus=...), plus byte equality with the oracle flavour wherever both ran.

Which shapes a flavour runs is decided here, when the tests are collected, from the field's two-adicity (q17: 2^9) and those
caps: nothing is skipped at run time."""
import functools
import json
import os
import random
import subprocess
import sys

import pytest

import abi_cases as cases
import flavour_cases as fc
from conftest import ROOT, _build_oracle, native_same_bytes
from genstark_amd._abi import MODULUS_17, MODULUS_32, MODULUS_64, MODULUS_224, MODULUS_256, Backend
from genstark_amd.errors import StarkError
from genstark_amd.field import PrimeField
from genstark_amd.hostfield import HostField
from genstark_amd._mirror.stark import Stark

FLAVOURS = {'q64': MODULUS_64, 'q32': MODULUS_32, 'q17': MODULUS_17, 'p256': MODULUS_256, 'p224': MODULUS_224}
BITINT = ('p256', 'p224')                   # oracle flavours on C23 _BitInt arithmetic: slow
# the oracle's radix-2 transform runs beside the HIP one up to here on the GPU tier (_BitInt flavours; the others: every size)
BITINT_ORACLE_NTT_LOGN = 17

NTT_GROUPS = dict([('horner', fc.NTT_HORNER), ('logn8', fc.NTT_ONE_PASS)] + [(f'logn{k}', v) for k, v in fc.NTT_TWO_PASS.items()]
                  + [(f'logn{k}', v) for k, v in fc.NTT_THREE_PASS.items()])


def _groups(name, cpu):
    """[(group, argument)] this flavour runs on this tier."""
    adic = fc.two_adicity(FLAVOURS[name])
    capped = cpu and name in BITINT
    out = []
    for g, shapes in NTT_GROUPS.items():
        if any(logn <= adic for logn, _, _ in shapes) and not (capped and min(s[0] for s in shapes) > fc.FULL_NTT_LOGN):
            out.append(('ntt', g))
    out += [('inverse', n) for n in fc.INVERSE_SIZES if not (capped and n > fc.FULL_INVERSE_N)]
    for alg in ('sha256', 'blake2s256'):
        out += [('merge_rows', (alg, n)) for n in fc.MERGE_ROWS_SIZES]
        out += [('merkle', (alg, logn)) for logn in fc.MERKLE_LOGN if not (capped and logn > 9)]
    out += [('fri_fold', s) for s in fc.FRI_FOLD_SHAPES if s[0] <= adic]
    out += [('fri_layers', s) for s in fc.FRI_LAYERS_SHAPES if s[0] + 2 * s[1] <= adic]
    out += [('tail', s) for s in fc.TAIL_SHAPES if s[0] <= adic]
    out += [('mimc', s) for s in fc.MIMC_SHAPES if s[0] <= adic]
    return out


def _id(arg):
    if isinstance(arg, tuple):
        return '-'.join(_id(a) for a in arg)
    return 'x'.join(map(str, arg)) if isinstance(arg, list) else str(arg)


def _params(cpu):
    return [pytest.param(name, g, arg, id=f'{name}-{g}-{_id(arg)}') for name in FLAVOURS for g, arg in _groups(name, cpu)]


def _rng(*key):
    return random.Random(repr(key))


def run_group(backend, group, arg, reference=True):
    """One check group on one backend; returns what identifies its output bytes (None where the check compares every byte with its
    reference itself)."""
    adic = fc.two_adicity(backend.modulus)
    if group == 'ntt':
        return [fc.check_ntt_shape(backend, _rng('ntt', logn, plen), logn, plen, rows, reference)
                for logn, plen, rows in NTT_GROUPS[arg] if logn <= adic]
    if group == 'inverse':
        return fc.check_batch_inverse(backend, _rng('inv', arg), arg, reference)
    if group == 'merge_rows':
        return fc.check_hash_merge_rows(backend, _rng('rows', arg), *arg)
    if group == 'merkle':
        return fc.check_merkle(backend, _rng('merkle', arg), *arg)
    if group == 'fri_fold':
        return cases.check_fri_fold(backend, _rng('fold', arg), *arg)
    if group == 'fri_layers':
        if reference:
            fc.check_fri_layers_definition(backend, _rng('layers-def', arg), *arg)
        return cases.check_fri_layers(backend, _rng('layers', arg), *arg)
    if group == 'tail':
        return [cases.check_composition_tail(backend, _rng('tail', arg[0], with_c), *arg, with_c=with_c) for with_c in (True, False)]
    if group == 'mimc':
        return cases.check_mimc_composition(backend, _rng('mimc', arg), *arg)
    raise AssertionError(group)


@functools.lru_cache(maxsize=None)
def oracle_for(name):
    _build_oracle()
    return Backend(lib_path=os.path.join(ROOT, 'oracle', f'liboracle_{name}.so'), allow_test_double=True)


def test_shapes_reach_every_pass_kernel_in_every_role():
    """From the plan arithmetic of csrc/ntt.hip: the shape lists run k_ntt_pass<LB> for every LB 1..4 as a first pass and every LB
    0..4 as a table pass, and the running-product branch, in every field with roots of unity of order 2^21; q17 stops at [5,4]."""
    assert [fc.ntt_plan(k) for k in (8, 9, 13, 14, 16, 17, 20, 21)] == [[8], [5, 4], [7, 6], [7, 7], [8, 8], [6, 6, 5], [7, 7, 6], [7, 7, 7]]
    for name, q in FLAVOURS.items():
        adic = fc.two_adicity(q)
        roles = {r for shapes in NTT_GROUPS.values() for logn, _, _ in shapes if logn <= adic for r in fc.ntt_roles(logn)}
        if name == 'q17':
            assert adic == 9 and roles == {(4, 'first'), (1, 'first'), (0, 'table')}
        else:
            assert roles >= {(lb, 'first') for lb in range(1, 5)} | {(lb, 'table') for lb in range(5)} | {(3, 'running')}
    assert fc.ntt_roles(20)[2] == (2, 'table') and fc.ntt_roles(21)[2] == (3, 'running')       # the table limit lies between them


def test_field_edges_are_elements_of_the_field():
    for q in FLAVOURS.values():
        e = fc.field_edges(q)
        assert all(0 <= v < q for v in e) and {0, 1, q - 1, (1 << q.bit_length()) - q} <= set(e)
    assert {2**64, 2**64 - 1, 2**224, 2**224 - 1, 351 * 2**32 - 1} <= set(fc.field_edges(MODULUS_256))
    assert 2**32 not in fc.field_edges(MODULUS_32) and 2**32 in fc.field_edges(MODULUS_64)


@pytest.mark.parametrize('name,group,arg', _params(cpu=True))
def test_oracle_flavour(name, group, arg):
    run_group(oracle_for(name), group, arg)


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hip_for():
    """One HIP backend per flavour for the module, closed at the end."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = Backend(device=0, modulus=FLAVOURS[name])
            assert made[name].name == 'hip-gfx950' and made[name].modulus == FLAVOURS[name]
        return made[name]
    yield get
    for be in made.values():
        be.close()


def _oracle_runs_beside_hip(name, group, arg):
    if name in BITINT and group == 'ntt':
        return max(s[0] for s in NTT_GROUPS[arg]) <= BITINT_ORACLE_NTT_LOGN
    return True


@pytest.mark.gpu
@pytest.mark.parametrize('name,group,arg', _params(cpu=False))
def test_hip_flavour(hip_for, name, group, arg):
    got = run_group(hip_for(name), group, arg)
    if _oracle_runs_beside_hip(name, group, arg):
        assert got == run_group(oracle_for(name), group, arg, reference=False), 'HIP bytes differ from the oracle flavour'


@pytest.mark.gpu
def test_fibonacci_example_at_the_size_its_source_quotes(hip_for):
    """examples/demo/fibonacci.ts at 2^13 steps over the 32-bit field: the only proof in a small field whose domain (2^17) takes a
    three-pass transform, a streaming Merkle tree and multi-workgroup FRI layers.  HIP bytes == oracle-flavour bytes == the native
    driver's; the device-free verifier accepts them; a changed assertion is rejected."""
    from genstark_amd.air_generic import GenericAir
    from test_small_fields import FIBONACCI

    def fibonacci_air(field, steps):
        """test_small_fields.fibonacci_air with the extension factor its options name: 2^13 steps on a domain of 2^17 points"""
        return GenericAir(steps, 2, [1, 1], [], lambda r, k: [r[0] + r[1], r[0] + 2 * r[1]],
                          lambda r, n, k: [n[0] - (r[0] + r[1]), n[1] - (r[0] + 2 * r[1])], lambda seed: [seed[0], seed[1]], 16, field)
    steps = 2**13
    opts = {'hashAlgorithm': 'sha256', 'extensionFactor': 16, 'exeQueryCount': 32, 'friQueryCount': 16}
    assertions = [{'step': 0, 'register': 0, 'value': 1}, {'step': 0, 'register': 1, 'value': 1},
                  {'step': steps - 1, 'register': 1, 'value': FIBONACCI[steps]}]
    changed = assertions[:2] + [dict(assertions[2], value=FIBONACCI[steps] - 1)]
    hip = hip_for('q32')
    datas = []
    for be in (hip, oracle_for('q32')):
        air = fibonacci_air(PrimeField(backend=be), steps)
        assert air.extensionFactor == 16
        stark = Stark(air, opts)
        before = be.stats.get('ntt_points', 0)
        data = stark.serialize(stark.prove(assertions, [], [1, 1]))
        if be is hip:
            assert be.stats['ntt_points'] - before >= 2 << 17                    # both registers went through a 2^17-point transform
            assert stark.verify(assertions, stark.parse(data))
            with pytest.raises(StarkError):
                stark.verify(changed, stark.parse(data))
            native_same_bytes(stark, assertions, [], [1, 1], data)
        datas.append(data)
    assert datas[0] == datas[1], 'HIP proof bytes differ from the oracle flavour'
    hv = Stark(fibonacci_air(HostField(MODULUS_32), steps), opts)
    assert hv.verify(assertions, hv.parse(datas[0]))
    with pytest.raises(StarkError):
        hv.verify(changed, hv.parse(datas[0]))


# ---- the runtime-modulus build: one modulus per process -----------------------------------------------------------------------
def _run_worker(q, which, more=()):
    from test_runtime_modulus import WORKER
    r = subprocess.run([sys.executable, WORKER, str(q), which, 'kernels'], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (q, r.stderr[-4000:])
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec['modulus'] == str(q) and len(rec['proofs']) == 2
    # (a) up to 2^16 points, (b) up to 40 000, (c) up to 2^9 leaves, (d): every case ran
    assert {'ntt-16-65536-3', 'ntt-9-33-3', 'inverse-40000', 'merge-rows-sha256-4097', 'fri-layers-13', 'tail-13-0', 'mimc-12'} | set(more) <= set(rec['kernels'])
    assert not any(k.startswith(('ntt-17', 'inverse-524301')) for k in rec['kernels'])
    return rec


def test_runtime_modulus_kernels_on_the_oracle():
    from test_runtime_modulus import PRIMES
    _build_oracle()
    assert _run_worker(PRIMES[0], 'oracle')['backends'] == ['oracle']


@pytest.mark.gpu
@pytest.mark.parametrize('which', [0, 23], ids=['31-bit', '255-bit'])
def test_runtime_modulus_kernels_hip_equal_oracle(which):
    """(the 31-bit prime has roots of unity up to order 2^16; the 255-bit one also runs the multi-workgroup FRI layers over 2^19 points)"""
    from test_runtime_modulus import PRIMES
    _build_oracle()
    assert _run_worker(PRIMES[which], 'both', ['fri-layers-17'] if which else [])['backends'] == ['hip', 'oracle']
