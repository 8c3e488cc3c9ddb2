"""The programs the code generator (csrc/air_codegen.h) is pinned on, per fixed field flavour, and the two ways to put one through it:
the library's compile hook (tests/golden/make_air_jit_sources.py records with it) and the stand-alone harness
(tests/host_harness/air_codegen_host.cpp, tests/test_air_codegen_host.py).

Per flavour: targeted_programs, constraint_programs and generated_program(0..63) of tests/air_programs.py, and, in their own flavours,
the example AIRs tests/test_air_codegen.py builds.  An entry holds what the generator reads and nothing else."""
import ctypes as C
import os
from types import SimpleNamespace

import air_programs as ap
from field_corners import FIXED

SEEDS = range(64)
FLAVOUR_NAMES = list(FIXED)                 # p128, q64, q32, q17, p256, p224
ELEMENT_SIZE = {name: 32 if bits > 128 else 16 for name, (q, bits) in FIXED.items()}
CACHE_PROBE_SOURCE = b'extern "C" __global__ void gs_jit_probe(fe *o) { o[0] = fe_one(); }\n'


def _entry(name, kind, code, init, consts, vm_regs, registers, nout, lens, values):
    """values: the static tables' elements in one list (trace programs: the selector rule reads them), or None."""
    return SimpleNamespace(name=name, kind=kind, code=[tuple(i) for i in code], init=[tuple(i) for i in init], consts=list(consts), vm_regs=vm_regs,
                           registers=registers, nout=nout, lens=list(lens), values=values)


def _of_program(p):
    if p.kind == 'trace':
        return _entry(p.name, 'trace', p.code, p.init, p.consts, p.vm_regs, p.registers, p.registers, [len(s) for s in p.statics],
                      [v for s in p.statics for v in s] or None)
    return _entry(p.name, 'constraints', p.code, [], p.consts, p.vm_regs, p.registers, p.constraints, [len(t) for t in p.tables], None)


def _of_air(name, air):
    """What GenericAir.compileCheck hands to the compile hook: the trace program of a segmented AIR, and the constraint program."""
    lens = [len(v) for v in air.staticRegisters] + [air.steps] * air.secretInputCount
    q, out = air.field.modulus, []
    if air.segmentLength is not None:
        t, init = air.transitionProgram, air.initProgram
        values = None if air.secretInputCount else [v % q for table in air.staticRegisters for v in table] or None
        out.append(_entry(name + '_trace', 'trace', t.code, init.code if init is not None else [], t.consts, t.nregs, air.traceRegisterCount,
                          air.traceRegisterCount, lens, values))
    e = air.evaluationProgram
    out.append(_entry(name + '_constraints', 'constraints', e.code, [], e.consts, e.nregs, air.traceRegisterCount, e.nout, lens, None))
    return out


def _example_airs(name):
    from conftest import ROOT, _build_oracle
    from genstark_amd import lib224, poseidon
    from genstark_amd._abi import Backend
    from genstark_amd.field import PrimeField
    from genstark_amd.pointmul import point_mul_air
    from genstark_amd.rescue import rescue4x128_air
    if name not in ('p128', 'p224'):
        return []
    _build_oracle()
    lib = 'liboracle.so' if name == 'p128' else f'liboracle_{name}.so'
    f = PrimeField(backend=Backend(lib_path=os.path.join(ROOT, 'oracle', lib), allow_test_double=True))      # the AIRs need a field for their constants
    if name == 'p128':
        return (_of_air('rescue4x128_segmented', rescue4x128_air(1024, 16, f, segmented=True))
                + _of_air('poseidon6x128_segmented', poseidon.poseidon6x128_air(2048, 16, f, segmented=True))
                + _of_air('rescue4x128', rescue4x128_air(64, 16, f)))
    return _of_air('point_mul', point_mul_air(f)) + _of_air('verify_schnorr_signature', lib224.verify_schnorr_signature_air(f))


def corpus(name):
    """The entries of one flavour, in a fixed order, names unique."""
    programs = ap.targeted_programs(name) + ap.constraint_programs(name) + [ap.generated_program(seed, name) for seed in SEEDS]
    entries = [_of_program(p) for p in programs] + _example_airs(name)
    assert len({e.name for e in entries}) == len(entries)
    return entries


def _hex(vals, es):
    return b''.join(int(v).to_bytes(es, 'little') for v in vals).hex() or '-'


def harness_text(name, e):
    """The entry as tests/host_harness/air_codegen_host.cpp reads it."""
    es = ELEMENT_SIZE[name]
    words = ' '.join(str(w) for ins in e.code for w in ins)
    iwords = ' '.join(str(w) for ins in e.init for w in ins)
    return (f'flavour {name}\nprog {e.kind} {len(e.code)} {len(e.init)} {len(e.consts)} {e.vm_regs} {e.registers} {len(e.lens)} {e.nout}\n{words}\n{iwords}\n'
            f'{" ".join(str(n) for n in e.lens)}\nconsts {_hex(e.consts, es)}\nstatics {_hex(e.values or [], es)}\n')


def through_hook(lib, e):
    """gs_air_jit_check_statics(entry) -> (return code, log).  With GSTARK_AIR_JIT_DUMP set the library leaves the source in that directory."""
    es = lib.gs_element_size()
    hook = lib.gs_air_jit_check_statics
    hook.restype = C.c_int
    hook.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                     C.c_char_p, C.c_void_p, C.c_uint64]
    lens = (C.c_uint64 * max(len(e.lens), 1))(*e.lens)
    log = C.create_string_buffer(8192)
    rc = hook(0 if e.kind == 'trace' else 1, ap._words(e.code), len(e.code), ap._words(e.init), len(e.init), ap._pack(e.consts, es) or bytes(es), len(e.consts),
              e.vm_regs, e.registers, lens, len(e.lens), ap._pack(e.values or [], es), log, len(log))
    return rc, log.value.decode(errors='replace')
