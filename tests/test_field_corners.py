"""Each field's arithmetic on operands that take its rare carries (tests/field_corners.py): the carry out of the second fold, the
closing conditional subtraction, the wrap of the 64-bit fold, the subtraction after a Montgomery reduction.  Uniformly random operands
take these branches with probability 2^-32 .. 2^-170, so neither the random vectors of the other tests nor whole proofs ever do.

CPU tier: the generator's classes are counted (none may run empty); the device headers as they compile for the host, the host product
of host_field*.h and the lazy-limb products of gf128_lazy.h run in a stand-alone program (tests/host_harness/field_corners_host.cpp),
built with g++ and the ROCm clang++, optimised and with the address / undefined-behaviour sanitizers, against Python integers; the
oracle flavours take the same vectors through the ABI (the 128-bit one here, the others through check_arithmetic of
tests/test_small_fields.py).  The GPU tier lives beside the other GPU tests of each flavour (test_gpu_parity.py, test_small_fields.py,
test_wide_fields.py, test_runtime_modulus.py through its worker)."""
import os
import random
import shutil
import subprocess

import pytest

import field_corners as fc
from conftest import ROOT, _build_oracle
from test_runtime_modulus import PRIMES

RUNTIME_PRIMES = [PRIMES[i] for i in (0, 6, 7, 12, 18, 23)]            # the first parametrisation of tests/test_runtime_modulus.py
MODULI = dict(fc.FIXED)
MODULI.update({f'rt{p.bit_length()}_{i}': (p, p.bit_length()) for i, p in enumerate(RUNTIME_PRIMES)})

HARNESS = os.path.join(ROOT, 'tests', 'host_harness', 'field_corners_host.cpp')
FLAVOUR_FLAGS = {'p128': [], 'q64': [f'-DGS_SMALL_Q={fc.MODULUS_64}ull'], 'q32': [f'-DGS_SMALL_Q={fc.MODULUS_32}ull'],
                 'q17': [f'-DGS_SMALL_Q={fc.MODULUS_17}ull'], 'p256': ['-DGS_WIDE_BITS=256'], 'p224': ['-DGS_WIDE_BITS=224'], 'rt': ['-DGS_WIDE_BITS=0']}
COMPILERS = {'g++': 'g++', 'clang++': '/opt/rocm/lib/llvm/bin/clang++'}
if not os.path.exists(COMPILERS['clang++']):                            # the ROCm clang++ when present
    del COMPILERS['clang++']
MODES = {'O2': ['-O2'], 'sanitized': ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']}


# ---- the generator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(MODULI))
def test_every_reachable_class_is_populated(name):
    p, bits = MODULI[name]
    cases = fc.cases_for(p, bits)
    for cname, tuples in cases.items():
        assert all(0 <= v < p for t in tuples for v in t), cname
    count = fc.coverage(p, bits, cases)
    assert sorted(count) == sorted(fc.all_classes(p, bits))
    for cls, n in count.items():
        if fc._unreachable(cls, p, bits):
            assert n == 0, (name, cls, 'listed as unreachable, yet the generator reaches it')
        else:
            assert n >= fc.MIN_PER_CLASS, (name, cls, n)
    # squares alone take every reachable branch of the product too (fe_sqr, lz_sqr and the exponentiation chains see only them)
    squares = {}
    for a, b in fc.square_pairs(cases):
        for cls in fc.classify_product(p, bits, a, b):
            squares[cls] = squares.get(cls, 0) + 1
    for cls in fc.SQUARE_CLASSES.get(fc.kind_of(p, bits), []):
        assert squares.get(cls, 0) >= fc.MIN_PER_CLASS, (name, 'squares', cls, squares.get(cls, 0))


def test_the_unreachable_table_is_what_the_issue_expects():
    """No carry out of 2^256 in p224 sums; no carry limb of the Montgomery reduction for moduli below 2^255; no fold classes for q32 and
    q17 — and nothing is listed for a modulus that reaches it."""
    assert fc._unreachable('add_carry_out', *fc.FIXED['p224']) and not fc._unreachable('add_carry_out', *fc.FIXED['p256'])
    assert not fc._unreachable('add_carry_out', *fc.FIXED['p128']) and not fc._unreachable('add_carry_out', *fc.FIXED['q64'])
    for p in RUNTIME_PRIMES:
        assert p < 2**255 and fc._unreachable('redc1_carry_limb', p, p.bit_length()) and fc._unreachable('redc2_carry_limb', p, p.bit_length())
        assert fc._unreachable('redc1_sub', p, p.bit_length()) == (p * p < 2**256)
    for name in ('q32', 'q17'):
        assert fc.kind_of(*fc.FIXED[name]) == 'rem' and fc._unreachable('fold_carry', *fc.FIXED[name]) and fc._unreachable('final_sub', *fc.FIXED[name])
    assert not any(fc._unreachable('final_sub', *fc.FIXED[name]) for name in ('p128', 'q64', 'p256', 'p224'))
    assert all(reason for entries in fc.UNREACHABLE.values() for _, reason in entries)


def test_the_predicates_are_the_branches_of_a_plain_integer_model():
    """classify_product's asserts are the headers' own bounds ('cannot carry again', 'the wrapped value is tiny', k in {0, 1}): they hold
    over every corner vector and over random ones, and uniformly random operands take none of the rare branches."""
    rng = random.Random(5)
    for name, (p, bits) in MODULI.items():
        rare = {'fold2_carry', 'final_sub', 'k_set', 'close_overflow', 's3_wrap'}
        for _ in range(2000):
            cls = fc.classify_product(p, bits, rng.randrange(p), rng.randrange(p))
            if fc.kind_of(p, bits) in ('wide', 'p128'):
                assert not rare & set(cls), (name, cls)


# ---- the host tier ------------------------------------------------------------------------------------------------------------------
def host_lines(p, bits, flavour):
    """[(op, a, b, expected)] for the stand-alone program: every class through every routine it bears on."""
    cases = fc.cases_for(p, bits)
    inv = lambda v: pow(v, -1, p) if v % p else 0
    lines = []
    for a, b in fc.product_pairs(cases):
        r = a * b % p
        lines += [('mul', a, b, r), ('hmul', a, b, r), ('hmulw', a, b, r), ('hchain', a, b, (r * b + a) % p)]
        if flavour == 'p128':
            lines += [('lzmul', a, b, r), ('lzmulu', a, b, r), ('lzmulw', a, b, r)]
    for a, _ in fc.square_pairs(cases):
        lines += [('sqr', a, 0, a * a % p), ('pow2', a, 0, a * a % p), ('pow', a, 2, a * a % p)]
        if flavour == 'p128':
            lines.append(('lzsqr', a, 0, a * a % p))
    # x^3 and x^5 whose LAST product is steered: x = a, and the residue of x^3 (x^5) itself cannot be chosen, so take cube (fifth) roots
    # where they exist — gcd(e, p - 1) = 1 — else the plain corner operands
    small = [r for name in ('r_fixed_low', 'r_from_C', 'r_just_above_C', 'r_below_C') for r in fc.product_residues(p, bits, random.Random(p))[name]]
    for e, op in ((3, 'pow3'), (5, 'pow5')):
        if (p - 1) % e:
            d = pow(e, -1, p - 1)
            for r in small:
                x = pow(r, d, p)
                lines += [(op, x, 0, r), ('pow', x, e, r)]
        for a, _ in fc.square_pairs(cases)[:40]:
            lines.append((op, a, 0, pow(a, e, p)))
    for a, b in fc.sum_pairs(cases):
        lines += [('add', a, b, (a + b) % p), ('sub', a, b, (a - b) % p), ('hadd', a, b, (a + b) % p), ('hsub', a, b, (a - b) % p),
                  ('haddw', a, b, (a + b) % p)]
    edges = fc.edge_list(p, bits)
    for a in edges + [x for x, _ in fc.product_pairs(cases)[40:60]]:
        lines += [('neg', a, 0, (-a) % p), ('inv', a, 0, inv(a)), ('hinv', a, 0, inv(a)), ('pow', a, p - 2, inv(a)), ('pow', a, p - 1, 1 if a else 0)]
    for a in edges[:8]:
        for e in (0, 1, 2, 3, 5):
            lines.append(('pow', a, e, pow(a, e, p)))
    return lines


def build_harness(flavour, compiler, mode, outdir):
    exe = os.path.join(outdir, f'field_corners_host_{flavour}_{compiler}_{mode}')
    subprocess.check_call([COMPILERS[compiler], '-std=c++17', *MODES[mode], *FLAVOUR_FLAGS[flavour], HARNESS, '-o', exe])
    return exe


def run_harness(exe, p, bits, flavour):
    lines = host_lines(p, bits, flavour)
    text = ''.join(f'{op} {a:064x} {b:064x}\n' for op, a, b, _ in lines)
    args = [exe] + ([f'{p:064x}'] if flavour == 'rt' else [])
    r = subprocess.run(args, input=text, capture_output=True, text=True)              # run directly: nothing preloaded
    assert r.returncode == 0, (flavour, r.returncode, r.stderr[-3000:])
    out = r.stdout.split()
    assert len(out) == len(lines), (len(out), len(lines), r.stderr[-2000:])
    for (op, a, b, want), got in zip(lines, out):
        assert got != '?', op
        got = int(got, 16)
        assert got < p, (flavour, 'not canonical', op, hex(a), hex(b), hex(got))
        assert got == want, (flavour, op, hex(a), hex(b), hex(got), hex(want), fc.classify_product(p, bits, a, b))


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('compiler', sorted(COMPILERS))
@pytest.mark.parametrize('flavour', sorted(FLAVOUR_FLAGS))
def test_host_arithmetic_on_corners(flavour, compiler, mode, tmp_path):
    assert shutil.which(COMPILERS[compiler]), 'the host tier needs ' + compiler
    exe = build_harness(flavour, compiler, mode, str(tmp_path))
    moduli = [(p, p.bit_length()) for p in RUNTIME_PRIMES] if flavour == 'rt' else [fc.FIXED[flavour]]
    for p, bits in moduli:
        run_harness(exe, p, bits, flavour)


# ---- the oracle's ABI (the GPU tests lean on its bytes) -----------------------------------------------------------------------------
def test_corner_arithmetic_oracle_128(oracle_backend):
    fc.check_corner_arithmetic(oracle_backend, fc.MODULUS_128)


@pytest.mark.parametrize('name', ['p128', 'q64', 'p224'])
def test_corner_trace_oracle(name):
    from genstark_amd._abi import Backend
    _build_oracle()
    lib = 'liboracle.so' if name == 'p128' else f'liboracle_{name}.so'
    backend = Backend(lib_path=os.path.join(ROOT, 'oracle', lib), allow_test_double=True)
    fc.check_corner_trace(backend, fc.FIXED[name][0])
