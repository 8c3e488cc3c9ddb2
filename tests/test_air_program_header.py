"""csrc/air_program.h — the validator, static layout and opcodes the native consumers of an AIR program share — on a table of malformed
programs, each next to a well-formed neighbour.

CPU tier: the table goes through the validator's three doors without a device: a stand-alone filter built with g++
(tests/host_harness/air_program_host.cpp, also with -fsanitize=address,undefined), gs_air_jit_check_statics and gs_prover_verify_on.
GPU tier: the same table through gs_air_constraints, gs_air_trace_segments and gs_air_trace; every neighbour runs and equals the model."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import pytest

import air_programs as ap
from air_programs import LOADC, LOADR, LOADN, LOADS, ADD, SUB, MUL, POW, POWC, OUT
from conftest import ROOT
from genstark_amd._abi import HIP_LIB_PATHS, Backend, GstarkError, load_library

SOURCE = os.path.join(ROOT, 'tests', 'host_harness', 'air_program_host.cpp')
_BUILT = {}


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    """sanitized or not -> the filter, built on first use (a program of its own: nothing is preloaded)."""
    def get(sanitized=False):
        if sanitized not in _BUILT:
            exe = str(tmp_path_factory.mktemp('air_program_host') / f'air_program_host{"_san" if sanitized else ""}')
            extra = ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] if sanitized else ['-O2']
            subprocess.check_call(['g++', '-std=c++17', *extra, SOURCE, '-o', exe])
            _BUILT[sanitized] = exe
        return _BUILT[sanitized]
    return get


def _head(c):
    words = ' '.join(str(w) for ins in c.code for w in ins)
    iwords = ' '.join(str(w) for ins in c.init for w in ins)
    return f'prog {c.kind} {len(c.code)} {len(c.init)} {c.nconsts} {c.vm_regs} {c.registers} {c.nstatic} {c.nout}\n{words}\n{iwords}\n{" ".join(["2"] * c.nstatic)}\n'


def feed(exe, texts):
    out = subprocess.run([exe], input=''.join(texts), capture_output=True, text=True, check=True).stdout.split('\n')
    assert len(out) >= len(texts)
    return out[:len(texts)]


# ---- malformed programs -----------------------------------------------------------------------------------------------------------
def _case(name, code, bad_at, kind='trace', init=(), vm_regs=2, registers=1, nconsts=1, nstatic=1, nout=1):
    """bad_at: the instruction the validator names (None: the program is well formed, 'shape': refused before any instruction)."""
    return SimpleNamespace(name=name, kind=kind, code=list(code), init=list(init), vm_regs=vm_regs, registers=registers, nconsts=nconsts, nstatic=nstatic,
                           nout=nout, bad_at=bad_at)


def malformed_table():
    """(malformed, neighbour) pairs on the smallest shapes: registers = 1, vm_regs = 2, nconsts = 1, nstatic = 1, one to three
    instructions.  The neighbour is the same program with the index one lower (or the nearest well-formed relative) and must be accepted,
    so a validator that refuses everything cannot pass; neighbours read no scratch register they have not written (the model runs them)."""
    pre = [(LOADR, 0, 0, 0), (LOADR, 1, 0, 0)]          # t0 and t1 written
    pairs = []

    def pair(name, bad, good, **kw):
        pairs.append((_case(name, pre + [bad], 2, **kw), _case(name + '_neighbour', pre + [good], None, **kw)))
    for op in (10, 99):
        pair(f'opcode{op}', (op, 0, 1, 0), (OUT, 0, 1, 0))
    for opname, op in (('loadc', LOADC), ('loadr', LOADR), ('loads', LOADS), ('add', ADD), ('sub', SUB), ('mul', MUL), ('pow', POW), ('powc', POWC)):
        pair(f'{opname}_dst', (op, 2, 0, 0), (op, 1, 0, 0))
    pair('loadn_dst', (LOADN, 2, 0, 0), (LOADN, 1, 0, 0), kind='constraints')
    for opname, op in (('add', ADD), ('sub', SUB), ('mul', MUL)):
        pair(f'{opname}_a', (op, 0, 2, 0), (op, 0, 1, 0))
        pair(f'{opname}_b', (op, 0, 0, 2), (op, 0, 0, 1))
    pair('pow_a', (POW, 0, 2, 3), (POW, 0, 1, 3))
    pair('powc_a', (POWC, 0, 2, 0), (POWC, 0, 1, 0))
    pair('out_a', (OUT, 0, 2, 0), (OUT, 0, 1, 0))
    pair('loadc_a', (LOADC, 0, 1, 0), (LOADC, 0, 0, 0))
    pair('powc_b', (POWC, 0, 1, 1), (POWC, 0, 1, 0))
    pair('loadr_a', (LOADR, 0, 1, 0), (LOADR, 0, 0, 0))
    pair('loadn_a', (LOADN, 0, 1, 0), (LOADN, 0, 0, 0), kind='constraints')
    pair('loads_a', (LOADS, 0, 1, 0), (LOADS, 0, 0, 0))
    pair('out_dst', (OUT, 1, 0, 0), (OUT, 0, 0, 0))
    pair('out_dst_constraints', (OUT, 1, 0, 0), (OUT, 0, 0, 0), kind='constraints')
    pair('loadn_in_trace', (LOADN, 0, 0, 0), (LOADR, 0, 0, 0))
    ok_main = pre + [(OUT, 0, 1, 0)]
    pairs.append((_case('loadn_in_init', ok_main, 2, init=pre + [(LOADN, 0, 0, 0)]), _case('loadn_in_init_neighbour', ok_main, None, init=pre + [(LOADR, 0, 0, 0)])))
    pairs.append((_case('loads_in_init', ok_main, 2, init=pre + [(LOADS, 0, 0, 0)]), _case('loads_in_init_neighbour', pre[:1] + [(LOADS, 1, 0, 0), (OUT, 0, 1, 0)], None, init=pre)))
    one = [(LOADR, 0, 0, 0), (OUT, 0, 0, 0)]
    pairs.append((_case('no_instructions', [], 'shape'), _case('no_instructions_neighbour', one[:1], None)))
    for what, bad, good in (('vm_regs', 0, 1), ('vm_regs', 65, 64), ('registers', 0, 1), ('registers', 65, 64), ('nstatic', 65, 64)):
        for kind in ('trace', 'constraints'):
            shape = dict(kind=kind, nout=64 if what == 'registers' else 1)
            pairs.append((_case(f'{what}{bad}_{kind}', one, 'shape', **{**shape, what: bad}), _case(f'{what}{good}_{kind}', one, None, **{**shape, what: good})))
    return pairs


TABLE = malformed_table()
CASES = [c for pair in TABLE for c in pair]


def runnable(case, name, nc=64, segments=9, seglen=2):
    """The case as a program of tests/air_programs.py for one flavour (constants, tables and rows of that field)."""
    q = ap.FLAVOURS[name][0]
    p = SimpleNamespace(name=case.name, kind=case.kind, q=q, code=case.code, init=case.init, consts=[5] * case.nconsts, vm_regs=case.vm_regs, registers=case.registers)
    tables = [[(3 + s) % q, q - 1] for s in range(case.nstatic)]
    if case.kind == 'trace':
        p.statics, p.seglen, p.segment_counts = tables, seglen, (segments,)
        p.rows = lambda n: ap.first_rows(q, max(case.registers, 1), n, 7)
    else:
        p.tables, p.constraints, p.nc, p.pstride, p.shift, p.prow = tables, case.nout, nc, 1, 1, nc
        p.columns = [(q - 1 - 3 * i) % q for i in range(max(case.registers, 1) * nc)]
    return p


def expected(p, segments=None):
    if p.kind == 'constraints' and not any(op == OUT for op, _, _, _ in p.code):
        return [0] * (p.constraints * p.nc)              # nothing is written: the zeros the output buffer was filled with
    want = ap.model(p, segments)
    return want + [0] * (p.constraints * p.nc - len(want)) if p.kind == 'constraints' else want      # (constraints past the last OUT stay zero)


def test_table_pairs_every_malformed_program_with_an_accepted_neighbour():
    assert len(TABLE) >= 40 and all(bad.bad_at is not None and good.bad_at is None for bad, good in TABLE)
    assert all(1 <= len(c.code) <= 3 for c in CASES if c.name != 'no_instructions')


@pytest.mark.parametrize('sanitized', [False, True])
def test_malformed_programs_through_the_harness(sanitized, harness):
    for c, verdict in zip(CASES, feed(harness(sanitized), [_head(c) for c in CASES])):
        if c.bad_at is None:
            assert verdict == 'ok', f'{c.name}: {verdict}'
        elif c.bad_at == 'shape':
            assert verdict.startswith('refused air program: ') and 'instruction' not in verdict, f'{c.name}: {verdict}'
        else:
            op = (c.init or c.code)[c.bad_at][0] if 'in_init' in c.name else c.code[c.bad_at][0]
            assert verdict == f'refused air program: invalid instruction {c.bad_at} (op {op})', f'{c.name}: {verdict}'


@pytest.mark.parametrize('name', list(ap.FLAVOURS))
def test_malformed_programs_through_the_compile_check(name):
    """gs_air_jit_check_statics validates before it generates: GS_ERR_UNSUPPORTED with the validator's message (GS_ERR_ARG, as before,
    for no program at all and for more static registers than the machine has).  An evaluator's number of constraints is no argument of
    the hook, so its OUT destinations are bounded for trace programs only."""
    lib = load_library(HIP_LIB_PATHS[ap.FLAVOURS[name][0]])
    es = lib.gs_element_size()
    hook = lib.gs_air_jit_check_statics
    hook.restype = C.c_int
    hook.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                     C.c_char_p, C.c_void_p, C.c_uint64]
    for c in CASES:
        if c.name.startswith('out_dst_constraints'):
            continue
        p = runnable(c, name)
        tables = p.statics if c.kind == 'trace' else p.tables
        lens = (C.c_uint64 * max(len(tables), 1))(*[len(t) for t in tables])
        log = C.create_string_buffer(4096)
        rc = hook(0 if c.kind == 'trace' else 1, ap._words(c.code), len(c.code), ap._words(c.init), len(c.init), ap._pack(p.consts, es), len(p.consts), c.vm_regs,
                  c.registers, lens, len(tables), ap._pack([v for t in tables for v in t], es) if c.kind == 'trace' else None, log, len(log))
        text = log.value.decode(errors='replace')
        if c.bad_at is None:
            assert rc == 0, f'{c.name} is refused: {text}'
        elif c.name in ('no_instructions',) or c.name.startswith('nstatic65'):
            assert rc == -1, f'{c.name}: {rc}'
        else:
            assert rc == -3 and text.startswith('air program: '), f'{c.name}: {rc} {text}'
            if c.bad_at != 'shape':
                assert f'instruction {c.bad_at} ' in text, f'{c.name}: {text}'


def test_malformed_evaluators_through_the_native_verifier(oracle_backend):
    """The 64-step `foo` statement and its valid proof.  The statement's own evaluator is the accepted neighbour (the proof verifies); with
    one index of one instruction set to its bound — every rule the evaluator has an instruction for, at every instruction —, with an
    unknown opcode, without instructions or with vm_regs of 0 or 65 the job is refused with the validator's message."""
    from genstark_amd.field import PrimeField
    from genstark_amd.native import NativeProver
    from genstark_amd._mirror.stark import Stark
    from test_generic_air import foo_air
    air = foo_air(PrimeField(backend=oracle_backend))
    trace = air.hostTrace([1])
    assertions = [{'step': 0, 'register': 0, 'value': trace[0][0]}, {'step': 63, 'register': 0, 'value': trace[63][0]}]
    nat = NativeProver(Stark(air, None))
    proof = bytes(nat.prove_bytes(assertions, [], [1]))
    assert nat.verify_bytes(assertions, proof)
    job, _keep = nat._verify_job(assertions)
    ja = job.air
    code = [tuple(ja.e_code[4 * k:4 * k + 4]) for k in range(ja.e_ninstr)]
    vm, bounds = ja.vm_regs, {'vm': ja.vm_regs, 'k': ja.nconsts, 'r': ja.registers, 's': ja.nstatic, 'o': ja.nconstraints}
    fields = {LOADC: 'vk', LOADR: 'vr', LOADN: 'vr', LOADS: 'vs', ADD: 'vvv', SUB: 'vvv', MUL: 'vvv', POW: 'vv', POWC: 'vvk', OUT: 'ov'}

    def verdict(words, ninstr, vm_regs=vm):
        ja.e_code, ja.e_ninstr, ja.vm_regs = (C.c_uint32 * max(len(words), 1))(*words), ninstr, vm_regs
        err = C.create_string_buffer(512)
        rc = nat.lib.gs_prover_verify_on(nat.binding, C.byref(job), proof, len(proof), err, 512)
        return rc, err.value.decode(errors='replace')
    flat = [w for ins in code for w in ins]
    assert verdict(flat, len(code)) == (0, '')
    rules = set()
    for k, ins in enumerate(code):
        for pos, f in enumerate(fields[ins[0]]):
            bad = list(flat)
            bad[4 * k + 1 + pos] = bounds['vm' if f == 'v' else f]
            assert verdict(bad, len(code)) == (-1, f'air program: invalid instruction {k} (op {ins[0]})'), (k, ins, pos)
            rules.add((ins[0], pos))
        for op in (10, 99):
            bad = list(flat)
            bad[4 * k] = op
            assert verdict(bad, len(code)) == (-1, f'air program: invalid instruction {k} (op {op})')
    assert {op for op, _ in rules} >= {LOADC, LOADR, LOADN, ADD, SUB, OUT}, 'the statement exercises the loads, sums and the outputs'
    # what foo's evaluator has no instruction for: one instruction appended (a refusal comes before anything of the proof is read)
    n = len(code)
    for ins in ((LOADS, 0, bounds['s'], 0), (LOADS, vm, 0, 0), (POWC, 0, 0, bounds['k']), (POWC, 0, vm, 0), (POWC, vm, 0, 0), (MUL, vm, 0, 0),
                (MUL, 0, vm, 0), (MUL, 0, 0, vm), (POW, vm, 0, 3), (POW, 0, vm, 3)):
        assert verdict(flat + list(ins), n + 1) == (-1, f'air program: invalid instruction {n} (op {ins[0]})'), ins
    registers = ja.registers
    for r in (0, 65):
        ja.registers = r
        assert verdict(flat, n) == (-1, 'air program: too many registers')
    ja.registers = registers
    assert verdict(flat, 0) == (-1, 'air program: empty')
    for n in (0, 65):
        assert verdict(flat, len(code), vm_regs=n) == (-1, 'air program: vm_regs must be in 1..64')
    assert verdict(flat, len(code)) == (0, '')


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hip():
    b = Backend(device=0, modulus=ap.FLAVOURS['p128'][0]).jit(False)
    yield b
    b.close()


def refused(call, c):
    with pytest.raises(GstarkError) as e:
        call()
    assert 'failed (-1): air program: ' in str(e.value), f'{c.name}: {e.value}'
    if c.bad_at != 'shape':
        assert f'invalid instruction {c.bad_at} (op ' in str(e.value), f'{c.name}: {e.value}'


@pytest.mark.gpu
def test_malformed_programs_through_the_device_entry_points(hip):
    """gs_air_constraints (64 points), gs_air_trace_segments (9 segments of 2 steps: above the host threshold) and gs_air_trace: GS_ERR_ARG
    with the validator's message before any launch; every neighbour runs and equals the model."""
    for c in CASES:
        p = runnable(c, 'p128')
        if c.kind == 'constraints':
            if c.bad_at is None:
                assert ap.constraints_on(hip, p) == expected(p), c.name
            else:
                refused(lambda: ap.constraints_on(hip, p), c)
            continue
        single = runnable(c, 'p128', segments=1, seglen=18)
        single.init = []
        if c.bad_at is None:
            assert ap.trace_on(hip, p, 9) == expected(p, 9), c.name
            assert ap.trace_on(hip, single, 1) == expected(single, 1), c.name
        else:
            refused(lambda: ap.trace_on(hip, p, 9), c)
            if not c.init:
                refused(lambda: trace_single(hip, single), c)


def trace_single(backend, p):
    """gs_air_trace: one chain of p.seglen steps."""
    es = backend.element_size
    periods = (C.c_uint32 * max(len(p.statics), 1))(*[len(s) for s in p.statics])
    out = backend.alloc(max(p.registers, 1) * p.seglen * es)
    try:
        backend.call('gs_air_trace', ap._words(p.code), len(p.code), ap._pack(p.consts, es), len(p.consts), p.vm_regs, p.registers,
                     ap._pack([v for s in p.statics for v in s], es), periods, len(p.statics), ap._pack(p.rows(1)[0], es), p.seglen, C.c_void_p(out))
        return ap._unpack(backend.download(out, p.registers * p.seglen * es), es)
    finally:
        backend.free(out)
