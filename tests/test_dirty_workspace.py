"""Every user of the context's block cache on recycled, poisoned blocks: include/gstark_debug.h (gs_cache_fill, csrc/ctx.hip),
Backend.cache_fill, and the cases of tests/dirty_cases.py.

gs_alloc hands a freed block back with whatever its last user left in it, so in a long-lived process every call runs on dirty memory,
while a test that calls a shape once runs on blocks fresh from the driver — in practice zeros, which are so often the right answer (a
Jacobian point with Z = 0 is infinity, a zero flag is "finite", a zero counter is a reset one) that a read before the write cannot show.
Here every entry runs on a fresh context (the control), after a decoy of the same shape whose residue is wrong for it, and after the
cache has been filled with 0x01 (canonical-looking elements, set flags, small counters) and with 0xFF (non-canonical elements, every
flag set, counters at their maximum); then the cases interleave on one context, whole proofs are made and verified on poisoned
blocks, and the other field flavours run the control and the harshest fill.  Every comparison is of bytes, with what
tests/dirty_cases.py computes on Python integers, hashlib and the package's host members.

CPU tier: the header, the binding, the completeness lock (every file of csrc/ that takes blocks from the cache has a case) and the
references' independence of anything but their seed.  `python tests/test_dirty_workspace.py runtime <q>` is the check of the
runtime-modulus flavour (one modulus per process)."""
import functools
import gc
import hashlib
import os
import random
import re
import subprocess
import sys

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pytest

import dirty_cases as dc
from genstark_amd import _abi
from genstark_amd._abi import Backend, GstarkError
from genstark_amd.errors import StarkError
from genstark_amd.field import PrimeField
from sponge_common import ROOT, check_header_is_plain_c, check_symbol_table

CSRC = os.path.join(ROOT, 'genstark_amd', 'csrc')
FILLS = {'0x01': 0x01, '0xff': 0xFF}


# ---- the table, as the tests walk it -------------------------------------------------------------------------------------------------------
def shapes_of(c, flavour):
    """every shape in the 128-bit build, one (the second where there are several) in the others"""
    return c.shapes if flavour == 'p128' else (c.shapes[1] if len(c.shapes) > 1 else c.shapes[0],)


def table(flavour):
    return [(c, shape) for c in dc.CASES if flavour in c.flavours for shape in shapes_of(c, flavour)]


def ident(pair):
    c, shape = pair
    return f'{c.name}-{shape}'.replace(' ', '').replace("'", '')


@functools.lru_cache(maxsize=None)
def made_for(modulus, element_size, name, shape):
    """a case's inputs and expected bytes: computed once per process, on the host, and shared by every test that needs them"""
    c = next(c for c in dc.CASES if c.name == name)
    return dc.made(c, shape, dc.FieldShape(modulus, element_size))


def made_on(f, c, shape):
    return made_for(f.modulus, f.elementSize, c.name, shape)


def count_sites(csrc):
    """{file: the number of `gs_alloc(` / `gs_tmp_alloc(` call sites in it} over the sources of a csrc directory"""
    sites = {}
    for name in sorted(os.listdir(csrc)):
        if name.endswith(('.hip', '.h', '.cc')):
            found = len(re.findall(r'\bgs_(?:tmp_)?alloc\(', open(os.path.join(csrc, name)).read()))
            if found:
                sites[name] = found
    return sites


def lock_failures(csrc):
    """what the completeness lock holds against a csrc directory: nothing, or one line per file whose sites differ from the table's"""
    found, out = count_sites(csrc), []
    for name in sorted(set(found) | set(dc.WORKSPACE_SITES)):
        if found.get(name, 0) != dc.WORKSPACE_SITES.get(name, 0):
            out.append(f'{name}: {found.get(name, 0)} call sites of the block cache, tests/dirty_cases.py knows {dc.WORKSPACE_SITES.get(name, 0)}: give the new user a case')
    named = {name for c in dc.CASES for name in c.files}
    out += [f'{name}: no case of tests/dirty_cases.py names it' for name in sorted(set(dc.WORKSPACE_SITES) - set(dc.DEFINITION_SITES) - named)]
    out += [f'{name}: named by a case, absent from WORKSPACE_SITES' for name in sorted(named - set(dc.WORKSPACE_SITES))]
    return out


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    check_header_is_plain_c('debug')


def test_symbol_table_matches_the_header():
    others = [getattr(_abi, name) for name in dir(_abi) if name.endswith('_SYMBOLS') and name != 'DEBUG_SYMBOLS']
    assert len(others) >= 13
    check_symbol_table('debug', _abi.DEBUG_SYMBOLS, others)
    header = open(os.path.join(ROOT, 'include', 'gstark_debug.h')).read()
    assert set(re.findall(r'\b(gs_\w+)\(', header)) == set(_abi.DEBUG_SYMBOLS) == {'gs_cache_fill'}
    assert 'test hook' in header and 'OPTIONAL' in header


def test_cache_fill_on_the_double_raises_its_own_message(oracle_backend):
    assert not any(hasattr(oracle_backend.lib, name) for name in _abi.DEBUG_SYMBOLS)
    with pytest.raises(GstarkError, match=r'has no gs_cache_fill \(include/gstark_debug\.h\)'):
        oracle_backend.cache_fill(0xFF)


def test_every_flavour_of_the_library_exports_the_entry():
    for path in list(_abi.HIP_LIB_PATHS.values()) + [_abi.HIP_LIB_PATH_RUNTIME]:
        assert hasattr(_abi.load_library(path), 'gs_cache_fill'), path


def test_every_user_of_the_block_cache_has_a_case(tmp_path):
    """the completeness lock"""
    assert count_sites(CSRC) == dc.WORKSPACE_SITES
    assert lock_failures(CSRC) == []
    assert all(dc.WORKSPACE_SITES[name] == sites for name, sites in dc.DEFINITION_SITES.items())
    # ... and it does fail for a new user: a copy of scan.hip with one more temporary
    (tmp_path / 'scan.hip').write_text(open(os.path.join(CSRC, 'scan.hip')).read() + '\nstatic int more(gs_ctx *c, void **p) { return gs_tmp_alloc(c, 64, p); }\n')
    (tmp_path / 'fresh.hip').write_text('int fresh(gs_ctx *c, void **p) { return gs_alloc(c, 64, p); }\n')
    failures = lock_failures(str(tmp_path))
    assert any(line.startswith('scan.hip: 2 call sites') for line in failures) and any(line.startswith('fresh.hip: 1 call sites') for line in failures)
    names = [c.name for c in dc.CASES]
    assert len(names) == len(set(names)) and all(2 <= len(c.shapes) <= 6 for c in dc.CASES)


@pytest.mark.parametrize('pair', table('p128'), ids=ident)
def test_expected_bytes_depend_on_the_seed_alone(pair):
    """computed twice from the same seed: equal, whatever else the process has done (no device, no clock, no hash randomisation)"""
    c, shape = pair
    f = dc.FieldShape(_abi.MODULUS_128, 16)
    first, second = made_for(f.modulus, f.elementSize, c.name, shape), dc.made(c, shape, f)
    assert first.want == second.want and len(first.want) > 0
    assert repr(first.probe) == repr(second.probe) and repr(first.decoy) == repr(second.decoy)
    assert repr(first.probe) != repr(first.decoy)


def test_one_shape_in_the_other_flavours_has_expected_bytes_too():
    for flavour in ('p224', 'q64'):
        for c, shape in table(flavour)[:6]:
            f = dc.FieldShape(dc.FLAVOUR_MODULI[flavour], dc.ELEMENT_SIZES[flavour])
            assert made_for(f.modulus, f.elementSize, c.name, shape).want == dc.made(c, shape, f).want


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------------
def run_dropped(m, f, x):
    """run, and everything it allocated is back in the cache"""
    out = m.run(f, x)
    gc.collect()
    return out


def check_kernels(be, m, what):
    seen = be.traffic()
    for name in m.kernels:
        assert any(k.startswith(name) for k in seen), (what, name, sorted(seen))


def control(be, c, shape):
    f = PrimeField(backend=be)
    m = made_on(f, c, shape)
    be.traffic(True)
    got = run_dropped(m, f, m.probe)
    check_kernels(be, m, ident((c, shape)))
    be.traffic(False)
    assert got == m.want, ('clean control', c.name, shape, first_difference(got, m.want))


def after_decoy(be, c, shape, fill):
    f = PrimeField(backend=be)
    m = made_on(f, c, shape)
    run_dropped(m, f, m.decoy)
    if fill is not None:
        blocks, nbytes = be.cache_fill(fill)
        assert blocks > 0 and nbytes >= 256 * blocks
    got = run_dropped(m, f, m.probe)
    assert got == m.want, ('after the decoy' if fill is None else f'cache filled with {fill:#04x}', c.name, shape, first_difference(got, m.want))


def first_difference(got, want):
    if len(got) != len(want):
        return f'{len(got)} bytes, not {len(want)}'
    at = next(i for i in range(len(got)) if got[i] != want[i])
    return f'{sum(a != b for a, b in zip(got, want))} of {len(got)} bytes differ, the first at {at}: {got[at:at + 16].hex()} for {want[at:at + 16].hex()}'


@pytest.fixture
def fresh():
    """this test's own context of the 128-bit build (the session's hip_backend is never poisoned)"""
    be = Backend(device=0)
    try:
        yield be
    finally:
        gc.collect()
        be.close()


@pytest.mark.gpu
def test_the_hook_itself(fresh):
    be = fresh
    size, other = 5 * 4096, 3 * 256
    pattern = bytes(range(256)) * (size // 256)
    assert be.cache_fill(0xA5) == (0, 0)                                     # nothing is cached yet
    live = be.alloc(other)
    be.upload(live, pattern[:other])
    p = be.alloc(size)
    be.upload(p, pattern)
    be.free(p)
    assert be.cache_fill(0xA5) == (1, size)
    q = be.alloc(size)
    assert q == p and be.download(q, size) == b'\xa5' * size                 # the same block, every byte of it
    assert be.download(live, other) == pattern[:other]                       # a live block keeps its contents
    be.free(q)
    be.free(live)
    assert be.cache_fill(0x00) == (2, size + other)
    again = be.alloc(other)
    assert again == live and be.download(again, other) == bytes(other)
    be.free(again)
    with pytest.raises(GstarkError, match='not a byte'):
        be.cache_fill(256)
    assert be.lib.gs_cache_fill(None, 1, None, None) == -1                   # GS_ERR_ARG without a context
    be.call('gs_cache_fill', 7, None, None)                                  # the counts are optional


@pytest.mark.gpu
def test_the_scan_tile_is_the_plans(fresh):
    f = PrimeField(backend=fresh)
    T = dc.scan_tile(f)
    assert f.scanPlan()['tile'] == T and [f.scanPlan(n)['launches'] for n in (T, T + 1)] == [1, 3]


@pytest.mark.gpu
@pytest.mark.parametrize('pair', table('p128'), ids=ident)
def test_clean_control(fresh, pair):
    control(fresh, *pair)


@pytest.mark.gpu
@pytest.mark.parametrize('pair', table('p128'), ids=ident)
def test_after_a_decoy_of_the_same_shape(fresh, pair):
    after_decoy(fresh, *pair, None)


@pytest.mark.gpu
@pytest.mark.parametrize('pair', table('p128'), ids=ident)
def test_after_the_cache_is_filled_with_0x01(fresh, pair):
    after_decoy(fresh, *pair, 0x01)


@pytest.mark.gpu
@pytest.mark.parametrize('pair', table('p128'), ids=ident)
def test_after_the_cache_is_filled_with_0xff(fresh, pair):
    after_decoy(fresh, *pair, 0xFF)


@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(4))
def test_cases_interleaved_on_one_context(fresh, seed):
    """what the context itself holds between calls — the arrival counters, the counter of the deferred fetches, the staging buffers,
    the transform plans, the square-root tables, the composition tables — under every order of users the draw gives"""
    be, f = fresh, PrimeField(backend=fresh)
    rng = random.Random(0xD1A7 + seed)
    pairs = table('p128')
    for step in range(30):
        c, shape = pairs[rng.randrange(len(pairs))]
        m = made_on(f, c, shape)
        if rng.randrange(2):
            run_dropped(m, f, m.decoy)
        fill = rng.choice((None, 0x01, 0xFF))
        if fill is not None:
            be.cache_fill(fill)
        got = run_dropped(m, f, m.probe)
        assert got == m.want, (seed, step, c.name, shape, fill, first_difference(got, m.want))


def changed(assertions, modulus):
    wrong = [dict(a) for a in assertions]
    wrong[len(wrong) // 2]['value'] = (wrong[len(wrong) // 2]['value'] + 1) % modulus
    return wrong


def verdicts(nat, assertions, data, be):
    """the device entry on poisoned blocks: accepts the proof, and rejects a changed assertion with the host entry's text"""
    be.cache_fill(0xFF)
    assert nat.verify_bytes(assertions, data, device=True) is True
    texts = []
    for device in (False, True):
        be.cache_fill(0xFF)
        with pytest.raises(StarkError) as e:
            nat.verify_bytes(changed(assertions, be.modulus), data, device=device)
        texts.append(str(e.value))
    assert texts[0] == texts[1] and texts[0]


@pytest.mark.gpu
@pytest.mark.parametrize('which', range(len(dc.golden_proofs())), ids=[g['name'] for g in dc.golden_proofs()])
def test_whole_proofs_on_poisoned_blocks(fresh, which):
    import genstark_amd as ga
    from genstark_amd.native import NativeProver
    be, golden = fresh, dc.golden_proofs()[which]
    want = bytes.fromhex(golden['proofHex'])
    options = {'hashAlgorithm': golden['hash_algorithm'], 'extensionFactor': golden['extension_factor'], 'exeQueryCount': golden['exe_query_count'],
               'friQueryCount': golden['fri_query_count']}
    stark = ga.instantiateMimc(golden['steps'], options, None, backend=be)
    assertions = [{'step': a['step'], 'register': a['register'], 'value': int(a['value'])} for a in golden['assertions']]
    nat = NativeProver(stark)
    assert nat.prove_bytes(assertions, [], [golden['seed']]) == want
    assert be.cache_fill(0xFF)[0] > 0
    assert nat.prove_bytes(assertions, [], [golden['seed']]) == want         # the native driver
    be.cache_fill(0xFF)
    assert stark.serialize(stark.prove(assertions, [], [golden['seed']])) == want      # ... and its Python mirror, whose vectors are blocks of the cache too
    verdicts(nat, assertions, want, be)


@pytest.mark.gpu
@pytest.mark.parametrize('jit', [False, True], ids=['interpreted', 'compiled'])
def test_the_rescue_statement_on_poisoned_blocks(fresh, oracle_backend, jit):
    from genstark_amd.native import NativeProver
    from test_generic_air import rescue_case
    air, stark, full, assertions = rescue_case(oracle_backend, 64)
    want = stark.serialize(stark.prove(assertions, [], [42, 43]))            # the CPU oracle's bytes, before the device is touched
    be = fresh.jit(jit)
    air, stark, full, assertions = rescue_case(be, 64)
    nat = NativeProver(stark)
    assert nat.prove_bytes(assertions, [], [42, 43]) == want
    assert be.cache_fill(0xFF)[0] > 0
    assert nat.prove_bytes(assertions, [], [42, 43]) == want
    be.cache_fill(0xFF)
    assert stark.serialize(stark.prove(assertions, [], [42, 43])) == want
    assert bool(be.jit_launches) == jit
    verdicts(nat, assertions, want, be)


def check_a_flavour(be, flavour):
    """the control and the harshest fill at one shape per case"""
    f = PrimeField(backend=be)
    T = dc.scan_tile(f)
    assert f.scanPlan()['tile'] == T and [f.scanPlan(n)['launches'] for n in (T, T + 1)] == [1, 3]
    for c, shape in table(flavour):
        control(be, c, shape)
        after_decoy(be, c, shape, 0xFF)


@pytest.mark.gpu
@pytest.mark.parametrize('flavour', ['p224', 'q64'])
def test_other_flavours(flavour):
    for c, shape in table(flavour):                                          # the expected bytes first: no integer loop inside the device section
        made_for(dc.FLAVOUR_MODULI[flavour], dc.ELEMENT_SIZES[flavour], c.name, shape)
    be = Backend(device=0, modulus=dc.FLAVOUR_MODULI[flavour])
    try:
        check_a_flavour(be, flavour)
    finally:
        gc.collect()
        be.close()


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    from test_runtime_modulus import PRIMES
    q = PRIMES[12]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(q)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f'runtime dirty workspace: modulus {q} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


if __name__ == '__main__':
    q = int(sys.argv[2])
    for c, shape in table('rt'):
        made_for(q, 32, c.name, shape)
    be = Backend(device=0, modulus=q, lib_path=_abi.HIP_LIB_PATH_RUNTIME)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    check_a_flavour(be, 'rt')
    gc.collect()
    be.close()
    print(f'runtime dirty workspace: modulus {q} ok')
