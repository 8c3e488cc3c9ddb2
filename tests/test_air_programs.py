"""What compiled and interpreted AIR programs COMPUTE, on programs written for every branch of the code generator (csrc/air_codegen.h)
and of the interpreters (csrc/air_vm.hip), and on generated ones.  The reference is a model of the register machine of include/gstark.h
on Python integers (tests/air_programs.py); all of it is integer work, so every comparison is on equality.

CPU tier: the model against the oracle's loop (an independent implementation: this is what validates the model); every targeted program
builds for gfx950 and its source takes the branch the program is there for; the addition chains of emit_pow compute their exponents.
GPU tier: model = oracle = library interpreted = library compiled, and a compiled run must really be compiled (jit_launches)."""
import pytest

import air_programs as ap
from genstark_amd._abi import HIP_LIB_PATHS, Backend, load_library
from test_wide_fields import oracle_for

GENERATED_CPU = 200             # generated programs per flavour, model against oracle
GENERATED_GPU = {'p128': 24, 'q64': 6, 'p224': 6}
GROUP = 3                       # programs per parametrized case: a case stays at a few seconds, hiprtc builds included

# ABI-legal programs the generator declines (the interpreter then runs them), by flavour and name, each with its reason: none.
EXPECTED_FALLBACK = {}


def _oracle(name, oracle_backend):
    return oracle_backend if name == 'p128' else oracle_for(name)


_TARGETED = {}


def targeted(name):
    """Trace programs, then constraint programs, of one flavour (built once per process)."""
    if name not in _TARGETED:
        _TARGETED[name] = ap.targeted_programs(name) + ap.constraint_programs(name)
    return _TARGETED[name]


TARGETED_COUNT = len(ap.targeted_programs('q64')) + len(ap.constraint_programs('q64'))
WIDE_COUNT = len(ap.targeted_programs('p224')) + len(ap.constraint_programs('p224'))            # (other shapes around the interpreter's LDS rule)


def runs_of(p):
    """(program, segments) for every shape the program runs at."""
    return [(p, s) for s in p.segment_counts] if p.kind == 'trace' else [(p, None)]


def same(got, want, what):
    if got != want:
        at = next(i for i, (g, w) in enumerate(zip(got, want)) if g != w)
        raise AssertionError(f'{what}: element {at} of {len(want)} is {got[at]:#x}, the model says {want[at]:#x}')


# ---- the model itself -----------------------------------------------------------------------------------------------------------
def test_model_refuses_reads_of_unwritten_scratch_registers():
    q = ap.FLAVOURS['p128'][0]
    code = [(ap.LOADR, 0, 0, 0), (ap.OUT, 0, 0, 0), (ap.ADD, 1, 0, 2), (ap.OUT, 0, 1, 0)]
    with pytest.raises(ap.UndefinedRead):
        ap.run_trace(code, [], [], [], [[5]], 1, 2, q)
    # ... also when an EARLIER execution wrote it: the scratch file is cleared before every execution
    code = [(ap.LOADR, 0, 0, 0), (ap.LOADS, 1, 0, 0), (ap.ADD, 2, 0, 1), (ap.OUT, 0, 2, 0)]
    assert ap.run_trace(code, [], [], [[1]], [[5]], 1, 3, q) == [5, 6, 7]
    with pytest.raises(ap.UndefinedRead):
        ap.run_trace(code, [(ap.ADD, 3, 0, 1), (ap.OUT, 0, 3, 0)], [], [[1]], [[5]], 1, 3, q)


def test_model_applies_outputs_in_program_order_and_keeps_unwritten_registers():
    q = ap.FLAVOURS['q64'][0]
    p = ap.two_outs_program(q, 64)
    rows = [[3, 5], [q - 1, 2]]
    out = ap.run_trace(p.code, [], p.consts, [], rows, 2, 3, q)
    assert out[:6] == [3, 3, 3, q - 1, q - 1, q - 1]                    # register 0: the second OUT (r0), not the first (r0^2)
    assert out[6:] == [5, 45, 405, 2, 2, 2]                             # register 1: r1 * r0^2
    keep = ap.run_trace([(ap.LOADR, 0, 1, 0), (ap.OUT, 0, 0, 0)], [], [], [], [[1, 2, 3]], 1, 2, q)
    assert keep == [1, 2, 2, 2, 3, 3]
    cons = ap.run_constraints([(ap.LOADR, 0, 0, 0), (ap.LOADN, 1, 0, 0), (ap.LOADS, 2, 0, 0), (ap.SUB, 0, 1, 0), (ap.MUL, 0, 0, 2), (ap.OUT, 0, 0, 0)],
                              [], [10, 0, 20, 0, 40, 0], 6, 2, 3, 4, [[1, 2]], q)
    assert cons == [(20 - 10) * 1, (40 - 20) * 2, (10 - 40) * 1 % q]    # shift 4 over 3 points: the next point; the table is cyclic


# ---- CPU tier: model against the oracle double --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ap.FLAVOURS))
def test_model_equals_oracle_on_targeted_programs(name, oracle_backend):
    oracle = _oracle(name, oracle_backend)
    for prog in targeted(name):
        for p, segments in runs_of(prog):
            same(ap.run_on(oracle, p, segments), ap.model(p, segments), f'{name} {p.name} segments={segments}: the oracle')


@pytest.mark.parametrize('name', list(ap.FLAVOURS))
def test_model_equals_oracle_on_generated_programs(name, oracle_backend):
    oracle = _oracle(name, oracle_backend)
    kinds = set()
    for seed in range(GENERATED_CPU):
        p = ap.generated_program(seed, name)
        assert 10 <= len(p.code) <= 120 and 1 <= p.registers <= 8, f'seed {seed}'
        kinds |= {op for op, _, _, _ in p.code}
        segments = p.segment_counts[0] if p.kind == 'trace' else None
        same(ap.run_on(oracle, p, segments), ap.model(p, segments), f'{name} seed {seed}: the oracle')
    assert kinds == set(range(10)), 'the generator reaches every opcode'


# ---- CPU tier: every targeted program builds, on the branch it is there for -----------------------------------------------------------
@pytest.fixture(scope='module')
def hip_libs():
    return {name: load_library(HIP_LIB_PATHS[ap.FLAVOURS[name][0]]) for name in ap.FLAVOURS}


@pytest.mark.parametrize('group', range(0, TARGETED_COUNT, 4))
def test_targeted_programs_build_on_their_branch(group, hip_libs, tmp_path, monkeypatch):
    """128-bit library: the source contains the string its builder names, so that a later change of the generator cannot silently move a
    program off the branch it is there for."""
    for p in targeted('p128')[group:group + 4]:
        src = ap.generated_source(hip_libs['p128'], p, tmp_path, monkeypatch)
        body = src[src.index('extern "C" __global__'):]         # (the preamble defines gs_dot_flush, gs_blend, ...: the kernel must USE them)
        for text in p.expect:
            assert text in (src if text.startswith('#define') else body), f'{p.name}: the generated kernel has no `{text}`'


@pytest.mark.parametrize('name,group', [(name, g) for name, n in (('q64', TARGETED_COUNT), ('p224', WIDE_COUNT)) for g in range(0, n, 6)])
def test_targeted_programs_build_in_the_other_flavours(name, group, hip_libs, tmp_path, monkeypatch):
    """The blend, the lazy chains and the W-form rows are 128-bit only: same shapes, generic code — it has to build.  What the generator
    declines is listed in EXPECTED_FALLBACK, and only that."""
    for p in targeted(name)[group:group + 6]:
        src = ap.generated_source(hip_libs[name], p, tmp_path, monkeypatch, declined_ok=True)
        assert (src is None) == ((name, p.name) in EXPECTED_FALLBACK), f'{name} {p.name}: declined programs are listed by name'
        if src is None:
            continue
        assert 'lz_' not in src and 'gs_blend(' not in src[src.index('extern "C" __global__'):]


def test_flat_and_register_routes_of_constraint_programs(hip_libs, tmp_path, monkeypatch):
    q, bits = ap.FLAVOURS['p128']
    flat = ap.generated_source(hip_libs['p128'], ap.constraint_program(q, bits, True, 129, 2, 1, 33), tmp_path, monkeypatch)
    regs = ap.generated_source(hip_libs['p128'], ap.constraint_program(q, bits, False, 129, 2, 1, 33), tmp_path, monkeypatch)
    assert 'gs_dot9_acc(acc, ' in flat and 'const fe v' in flat and 'j % 129ull' in flat and 'j % 3ull' in flat
    assert 'gs_dot9_begin' not in regs[regs.index('extern "C"'):] and 't0 = p[' in regs and 'j % 129ull' in regs and 'fe x1 = t' in regs     # (a group of two)


def test_later_out_to_one_register_is_the_one_emitted(hip_libs, tmp_path, monkeypatch):
    """LOADR t0,r0; MUL t1,t0,t0; OUT 0,t1; OUT 0,t0: ssa_emit writes outputs depth by depth, so the first OUT (depth 1) used to land
    after the second (depth 0) and the compiled step ended with n0 = r0^2.  ssa_build now drops an OUT that a later one overwrites."""
    q, bits = ap.FLAVOURS['p128']
    src = ap.generated_source(hip_libs['p128'], ap.two_outs_program(q, bits), tmp_path, monkeypatch)
    body = src[src.index('for (unsigned long long k = 0'):]
    writes = [ln.strip() for ln in body.split('\n') if ln.strip().startswith('n0 = ')]
    assert writes == ['n0 = r0;', 'n0 = r0;'], writes          # the copy of the current row, then the one OUT that counts


# ---- CPU tier: the addition chains of emit_pow ------------------------------------------------------------------------------------
CHAIN_CHUNK = 8                 # exponents per build: a case stays below ten seconds (hiprtc inlines every product of every chain)


@pytest.mark.parametrize('name,chunk', [(name, c) for name in ('p128', 'q64') for c in range(10)])
def test_emitted_chains_compute_their_exponents(name, chunk, hip_libs, tmp_path, monkeypatch):
    """For every exponent the chain in the generated source, followed statement by statement on integers, computes exactly that exponent:
    canonical windows (gs_sqr / gs_mul over p3, p5, ...), and in the 128-bit library the lazy windows and the pattern chain."""
    q, bits = ap.FLAVOURS[name]
    exponents = ap.chain_test_exponents(q, bits)
    assert 60 <= len(exponents) <= 10 * CHAIN_CHUNK
    es = exponents[chunk * CHAIN_CHUNK:(chunk + 1) * CHAIN_CHUNK]
    src = ap.generated_source(hip_libs[name], ap.chains_program(q, es), tmp_path, monkeypatch)
    blocks = ap.chain_blocks(src)
    assert len(blocks) == len(es), f'{len(blocks)} chains for {len(es)} exponents'
    shapes = set()
    for e, block in zip(es, blocks):
        got, products, val = ap.chain_exponent(block)
        assert got == e, f'the chain for {e:#x} computes {got:#x}:\n{block}'
        assert products <= 2 * e.bit_length() // 3 + 2, f'{e:#x}: {products} products'          # (square-and-multiply is the bound to beat)
        shapes.add('pattern' if 'g1' in val else ('lazy' if 'lz_' in block else 'canonical'))
    if chunk == 0:              # small and structured exponents: every chain shape of the flavour occurs
        assert shapes == ({'pattern', 'lazy', 'canonical'} if name == 'p128' else {'canonical'})


def test_pattern_chain_threshold_and_words(hip_libs, tmp_path, monkeypatch):
    """pattern_plan away from Rescue's one exponent: a leading "10" run of 8 pairs takes the pattern chain, one of 7 does not; the tail's
    "11" is served by p3 only where there is one."""
    q, bits = ap.FLAVOURS['p128']
    es = ap.long_exponents(q, bits)
    names = ['run7_p3', 'run7', 'run8_p3', 'run8']
    src = ap.generated_source(hip_libs['p128'], ap.chains_program(q, [es[n] for n in names]), tmp_path, monkeypatch)
    blocks = dict(zip(names, ap.chain_blocks(src)))
    assert len(blocks) == 4
    for n in names:
        got, _, val = ap.chain_exponent(blocks[n])
        assert got == es[n], n
        assert ('g1' in val) == n.startswith('run8'), n
    assert 'const lz p3 = lz_mul_v(g1, p1, K);' in blocks['run8_p3'] and 'p3' not in blocks['run8']
    assert 'g8' in ap.chain_exponent(blocks['run8'])[2] and ap.chain_exponent(blocks['run8'])[2]['g8'] == int('10' * 8, 2)


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------
_HIP = {}


@pytest.fixture(scope='module')
def hip_backends():
    """name -> the product library of that flavour, interpreting (the suite's default mode)."""
    def get(name):
        if name not in _HIP:
            _HIP[name] = Backend(device=0, modulus=ap.FLAVOURS[name][0]).jit(False)
        return _HIP[name]
    yield get
    for b in _HIP.values():
        b.close()
    _HIP.clear()


def four_way(name, progs, oracle, interpreted, seed_of=lambda p: ''):
    """model = oracle = interpreted = compiled for every program at every shape; a compiled run is a compiled launch."""
    compiled = Backend(device=0, modulus=ap.FLAVOURS[name][0]).jit()
    try:
        for prog in progs:
            for p, segments in runs_of(prog):
                what = f'{name} {p.name}{seed_of(p)} segments={segments}'
                want = ap.model(p, segments)
                same(ap.run_on(oracle, p, segments), want, what + ': the oracle')
                before = interpreted.jit_launches
                same(ap.run_on(interpreted, p, segments), want, what + ': the library, interpreted')
                assert interpreted.jit_launches == before, what + ': the interpreting context launched a compiled program'
                before = compiled.jit_launches
                same(ap.run_on(compiled, p, segments), want, what + ': the library, compiled')
                host = p.kind == 'trace' and segments <= ap.HOST_SEGMENTS          # host_run, whatever the JIT mode
                expected = 0 if host or (name, p.name) in EXPECTED_FALLBACK else 1
                assert compiled.jit_launches - before == expected, what + f': {compiled.jit_launches - before} compiled launches, {expected} expected'
    finally:
        compiled.close()


@pytest.mark.gpu
@pytest.mark.parametrize('group', range(0, TARGETED_COUNT, GROUP))
def test_targeted_programs_four_ways(group, oracle_backend, hip_backends):
    four_way('p128', targeted('p128')[group:group + GROUP], oracle_backend, hip_backends('p128'))


@pytest.mark.gpu
@pytest.mark.parametrize('group', range(0, GENERATED_GPU['p128'], GROUP))
def test_generated_programs_four_ways(group, oracle_backend, hip_backends):
    progs = [ap.generated_program(seed, 'p128') for seed in range(group, group + GROUP)]
    four_way('p128', progs, oracle_backend, hip_backends('p128'), seed_of=lambda p: f' (seed {p.name.split("_")[1]})')


@pytest.mark.gpu
@pytest.mark.parametrize('name,group', [(name, g) for name, n in (('q64', TARGETED_COUNT), ('p224', WIDE_COUNT)) for g in range(0, n, GROUP)])
def test_targeted_programs_four_ways_in_the_other_flavours(name, group, oracle_backend, hip_backends):
    four_way(name, targeted(name)[group:group + GROUP], _oracle(name, oracle_backend), hip_backends(name))


@pytest.mark.gpu
@pytest.mark.parametrize('name,group', [(name, g) for name in ('q64', 'p224') for g in range(0, GENERATED_GPU[name], GROUP)])
def test_generated_programs_four_ways_in_the_other_flavours(name, group, oracle_backend, hip_backends):
    progs = [ap.generated_program(seed, name) for seed in range(group, group + GROUP)]
    four_way(name, progs, _oracle(name, oracle_backend), hip_backends(name), seed_of=lambda p: f' (seed {p.name.split("_")[1]})')
