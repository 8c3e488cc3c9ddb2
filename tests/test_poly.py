"""Long polynomials at arbitrary points: include/gstark_poly.h, csrc/poly_plan.h, csrc/poly.hip, polyFromRoots / divPolys / divModPolys /
evalPolyAtPoints / interpolateAtPoints of genstark_amd/field.py and js/galois.js.

Every comparison is equality with Python integers; the references are the schoolbook definitions below, written here and nowhere else.
CPU tier: the header, the binding table, the host plan on its own under the sanitizers (tests/host_harness/poly_plan_host.cpp), and the
Python members on the tests' double (which lacks the entries: the host fallback).  GPU tier: the four entries in the 128-bit flavour at
the sizes around the tree's switch-over (slots of 2^8 elements), under forced switch-overs, beyond the 4 096 points `interpolate` stops
at, in the other flavours, refused calls, node.  `python tests/test_poly.py runtime <q>` is the check of the runtime-modulus flavour
(one modulus per process)."""
import ctypes as C
import json
import os
import random
import subprocess
import sys
import types

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pytest

from genstark_amd import _abi
from genstark_amd._abi import MODULUS_17, MODULUS_224, Backend, GstarkError
from genstark_amd.field import PrimeField, Vector
from conftest import rand_elements
from sponge_common import ROOT, check_header_is_plain_c, check_symbol_table, flavour_fixture, needs_node, run_js
from test_curve import p224_double, q17_double      # noqa: F401 (fixtures)

P128 = 2**128 - 9 * 2**32 + 1
SIZES = (1, 2, 3, 5, 255, 256, 257, 511, 513, 1000)
DIV_SHAPES = ((1, 1), (5, 1), (5, 5), (4, 5), (600, 1), (600, 299), (600, 300), (600, 599), (513, 257))
EVAL_SHAPES = ((1, 1), (1, 300), (300, 1), (257, 256), (256, 257), (1000, 64), (64, 1000))


# ---- the references: schoolbook on Python integers ----------------------------------------------------------------------------------------
def ref_mul(a, b, p):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % p
    return out


def ref_from_roots(xs, p):
    out = [1]
    for x in xs:
        out = ref_mul(out, [-x % p, 1], p)
    return out


def ref_divmod(a, b, p):
    """long division: (q, r) with the lengths include/gstark_poly.h states"""
    la, lb = len(a), len(b)
    if la < lb:
        return [0], (list(a) + [0] * lb)[:lb - 1]
    r, q, inv = list(a), [0] * (la - lb + 1), pow(b[-1], p - 2, p)
    for k in range(la - lb, -1, -1):
        q[k] = r[k + lb - 1] * inv % p
        for j in range(lb):
            r[k + j] = (r[k + j] - q[k] * b[j]) % p
    assert not any(r[lb - 1:])
    return q, r[:lb - 1]


def ref_eval(poly, xs, p):
    out = []
    for x in xs:
        acc = 0
        for c in reversed(poly):
            acc = (acc * x + c) % p
        out.append(acc)
    return out


def ref_interpolate(xs, ys, p):
    """Lagrange, term by term"""
    out = [0] * len(xs)
    for i, (xi, yi) in enumerate(zip(xs, ys)):
        num, den = [1], 1
        for j, xj in enumerate(xs):
            if j != i:
                num = ref_mul(num, [-xj % p, 1], p)
                den = den * (xi - xj) % p
        w = yi * pow(den, p - 2, p) % p
        for k, c in enumerate(num):
            out[k] = (out[k] + w * c) % p
    return out


def elements(rng, p, n, distinct=False):
    """random elements of the field of p elements with its edge values among them"""
    if p == P128:
        out = rand_elements(rng, n)
    else:
        edges = [0, 1, 2, p - 1, p - 2, p >> 1]
        out = [rng.choice(edges) if rng.random() < 0.1 else rng.randrange(p) for _ in range(n)]
    if distinct:
        seen, unique = set(), []
        for x in out:
            while x in seen:
                x = rng.randrange(p)
            seen.add(x)
            unique.append(x)
        out = unique
    return out


def nonzero_top(rng, p, values):
    return values[:-1] + [values[-1] or rng.randrange(1, p)]


# ---- CPU tier: header, binding table, plan ------------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    check_header_is_plain_c('poly')


def test_symbol_table_matches_the_header():
    assert _abi.POLY_SYMBOLS == ('gs_poly_from_roots', 'gs_poly_div', 'gs_poly_eval_points', 'gs_poly_interpolate_points', 'gs_poly_schoolbook_log2')
    check_symbol_table('poly', _abi.POLY_SYMBOLS, (_abi.EXPORTED_SYMBOLS, _abi.OPTIONAL_SYMBOLS, _abi.HADES_SYMBOLS, _abi.RESCUE_SYMBOLS, _abi.TREE_UPDATE_SYMBOLS,
                                                  _abi.TREE_VERIFY_SYMBOLS, _abi.SPARSE_TREE_SYMBOLS, _abi.MIMC_SYMBOLS, _abi.CURVE_SYMBOLS, _abi.MSM_SYMBOLS,
                                                  _abi.DIAGNOSE_SYMBOLS))
    header = open(os.path.join(ROOT, 'include', 'gstark_poly.h')).read()
    assert '2^20' in header and '4 294 967 296 bytes' in header               # the caps are part of the contract
    assert 'only read-back' in header and 'downloads the leading coefficient' in header
    plan = open(os.path.join(ROOT, 'genstark_amd', 'csrc', 'poly_plan.h')).read()
    assert '#define POLY_WORKSPACE_CAP (4ull << 30)' in plan and '#define POLY_MAX_LEN (1ull << 20)' in plan and '#include <hip' not in plan and '__global__' not in plan


def test_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'poly_plan_host')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-omit-frame-pointer', os.path.join(ROOT, 'tests', 'host_harness', 'poly_plan_host.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'plans ok' in r.stdout and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


# ---- the members against the references: shared by the double (host fallback) and the device ------------------------------------------------
def check_from_roots(f, rng, sizes):
    p = f.modulus
    assert f.polyFromRoots([]).toValues() == [1]
    for n in sizes:
        xs = elements(rng, p, n)
        want = ref_from_roots(xs, p)
        assert f.polyFromRoots(xs).toValues() == want, n
        if n in (1, 257):
            assert f.polyFromRoots(f.newVectorFrom(xs)).toValues() == want, n


def division_operands(rng, p, la, lb, exact=False):
    b = nonzero_top(rng, p, elements(rng, p, lb))                            # (non-monic: the top is any non-zero element)
    a = elements(rng, p, la)
    if exact and la >= lb:
        a = ref_mul(nonzero_top(rng, p, elements(rng, p, la - lb + 1)), b, p)
    return a, b


def check_division(f, rng, shapes, exact_shape):
    p = f.modulus
    for la, lb in shapes:
        a, b = division_operands(rng, p, la, lb)
        want = ref_divmod(a, b, p)
        q, r = f.divModPolys(a, b)
        assert (q.toValues(), r.toValues()) == want, (la, lb)
        assert (q.length, r.length) == (max(la - lb + 1, 1), lb - 1)
        if (la, lb) == shapes[-1]:
            assert f.divPolys(f.newVectorFrom(a), f.newVectorFrom(b)).toValues() == want[0]
    a, b = division_operands(rng, p, *exact_shape, exact=True)
    q, r = f.divModPolys(a, b)
    assert (q.toValues(), r.toValues()) == ref_divmod(a, b, p) and not any(r.toValues()) and r.length == exact_shape[1] - 1
    with pytest.raises(GstarkError, match='leading coefficient'):
        f.divModPolys([1, 2, 3], [5, 0])


def check_evaluation(f, rng, shapes, horner=True):
    p = f.modulus
    for plen, n in shapes:
        poly, xs = elements(rng, p, plen), elements(rng, p, n)
        if n >= 5:
            xs[:5] = [0, 1, p - 1, xs[-1], xs[-1]]                            # the edge points, and one point three times
        want = ref_eval(poly, xs, p)
        got = f.evalPolyAtPoints(poly, xs, method='tree')
        assert got.toValues() == want, (plen, n)
        if horner:
            assert f.evalPolyAtPoints(poly, xs, method='horner').toBuffer() == got.toBuffer(), (plen, n)
            assert f.evalPolyAtPoints(poly, xs).toBuffer() == got.toBuffer(), (plen, n)
        if (plen, n) == shapes[-1]:
            assert f.evalPolyAtPoints(f.newVectorFrom(poly), f.newVectorFrom(xs), method='tree').toValues() == want
    assert f.evalPolyAtPoints([], [1, 2], method='tree').toValues() == [0, 0] and f.evalPolyAtPoints([7], [], method='tree').length == 0


def check_interpolation(f, rng, sizes, reference=None):
    p = f.modulus
    for n in sizes:
        xs, ys = elements(rng, p, n, distinct=True), elements(rng, p, n)
        want = reference(xs, ys) if reference else ref_interpolate(xs, ys, p)
        assert f.interpolateAtPoints(xs, ys).toValues() == want, n
        if n in (1, 257):
            assert f.interpolateAtPoints(f.newVectorFrom(xs), f.newVectorFrom(ys)).toValues() == want, n
    many = 300 if (p - 1) % (1 << 11) == 0 else 100                           # (the field of 96 769 elements has no transform for 301 points)
    for xs in ([4, 4], [1, 2, 3, 4, 5, 2], list(range(many)) + [17]):
        with pytest.raises(GstarkError, match='two of the x coordinates are equal'):
            f.interpolateAtPoints(xs, list(range(len(xs))))
    with pytest.raises(GstarkError, match='same as number of y'):
        f.interpolateAtPoints([1, 2], [1])


# ---- CPU tier: the Python members on the host fallback --------------------------------------------------------------------------------------
def test_the_double_lacks_the_entries_and_falls_back(p224_double):
    assert not any(hasattr(p224_double.lib, name) for name in _abi.POLY_SYMBOLS)
    f = PrimeField(backend=p224_double)
    rng = random.Random(0x901)
    check_from_roots(f, rng, (1, 2, 3, 40))
    check_division(f, rng, ((1, 1), (5, 1), (5, 5), (4, 5), (1, 3), (40, 17)), (30, 12))
    check_evaluation(f, rng, ((1, 1), (1, 9), (9, 1), (20, 33), (33, 20)))
    check_interpolation(f, rng, (1, 2, 3, 30))


def test_the_fallback_in_the_small_field(q17_double):
    f = PrimeField(backend=q17_double)
    rng = random.Random(0x1717)
    check_from_roots(f, rng, (1, 50))
    check_division(f, rng, ((1, 1), (60, 1), (60, 23), (5, 9)), (50, 20))
    check_evaluation(f, rng, ((1, 1), (30, 50), (50, 30)))
    check_interpolation(f, rng, (1, 50))
    assert f.interpolateAtPoints(list(range(1, 41)), list(range(40))).toValues() == f.interpolate(list(range(1, 41)), list(range(40))).toValues()


def test_a_device_library_without_the_entries_is_an_error(p224_double):
    """no quiet host path where a HIP library lacks only these entries: the double's library under the product backend's name"""
    f = PrimeField(backend=p224_double)
    f.backend = types.SimpleNamespace(name='hip-gfx950', lib=p224_double.lib, element_size=32, modulus=MODULUS_224)
    for attempt in (lambda: f.polyFromRoots([1]), lambda: f.divModPolys([1, 2], [1, 1]), lambda: f.divPolys([1, 2], [1, 1]),
                    lambda: f.evalPolyAtPoints([1], [2], method='tree'), lambda: f.interpolateAtPoints([1], [2])):
        with pytest.raises(GstarkError, match=r'no gs_poly_from_roots \(include/gstark_poly\.h\)'):
            attempt()


def test_bad_operands_raise(p224_double):
    f = PrimeField(backend=p224_double)
    with pytest.raises(GstarkError, match='at least one coefficient'):
        f.divModPolys([], [1])
    with pytest.raises(GstarkError, match='method'):
        f.evalPolyAtPoints([1], [1], method='fast')
    with pytest.raises(GstarkError, match='at least one point'):
        f.interpolateAtPoints([], [])
    long = f.newVector(1)
    long.length = (1 << 20) + 1                                              # (refused by its length alone)
    with pytest.raises(GstarkError, match=r'2\^20'):
        f.polyFromRoots(long)


# ---- GPU tier -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_from_roots_128(hip_backend):
    check_from_roots(PrimeField(backend=hip_backend), random.Random(0xF0), SIZES)


@pytest.mark.gpu
def test_division_128(hip_backend):
    check_division(PrimeField(backend=hip_backend), random.Random(0xD1), DIV_SHAPES, (600, 257))


@pytest.mark.gpu
def test_evaluation_128(hip_backend):
    f = PrimeField(backend=hip_backend)
    check_evaluation(f, random.Random(0xE7), EVAL_SHAPES + tuple((n, n) for n in SIZES))


@pytest.mark.gpu
def test_interpolation_128(hip_backend):
    f = PrimeField(backend=hip_backend)
    check_interpolation(f, random.Random(0x17), tuple(n for n in SIZES if n <= 600) + (600,), reference=lambda xs, ys: f.interpolate(xs, ys).toValues())
    rng = random.Random(0x18)
    xs, ys = elements(rng, f.modulus, 1000, distinct=True), elements(rng, f.modulus, 1000)
    assert ref_eval(f.interpolateAtPoints(xs, ys).toValues(), xs[:8] + xs[-8:], f.modulus) == ys[:8] + ys[-8:]


def seam_results(f, seed):
    """the calls of the tests above at n = 257 and (600, 299): bytes, to be compared between switch-overs"""
    rng = random.Random(seed)
    p = f.modulus
    xs, ys, poly = elements(rng, p, 257, distinct=True), elements(rng, p, 257), elements(rng, p, 600)
    a, b = division_operands(rng, p, 600, 299)
    q, r = f.divModPolys(a, b)
    out = [f.polyFromRoots(xs).toBuffer(), q.toBuffer(), r.toBuffer(), f.evalPolyAtPoints(poly, xs, method='tree').toBuffer(),
           f.evalPolyAtPoints(poly[:257], xs + xs + xs[:86], method='tree').toBuffer(), f.interpolateAtPoints(xs, ys).toBuffer()]
    want = [ref_from_roots(xs, p), *ref_divmod(a, b, p), ref_eval(poly, xs, p), ref_eval(poly[:257], xs + xs + xs[:86], p)]
    es = f.elementSize
    values = [[int.from_bytes(raw[i:i + es], 'little') for i in range(0, len(raw), es)] for raw in out]
    assert values[:5] == want and len(values[5]) == 257 and ref_eval(values[5], xs, p) == ys
    return out


@pytest.mark.gpu
def test_the_switch_over_does_not_change_a_result(hip_backend):
    f = PrimeField(backend=hip_backend)
    setter = hip_backend.lib.gs_poly_schoolbook_log2
    base = seam_results(f, 0x5EA)
    before = setter(8)
    try:
        assert before == 8
        for log2 in (2, 4, 10):
            assert setter(log2) in (8, 2, 4)
            assert seam_results(f, 0x5EA) == base, log2
        assert setter(0) == 10 and setter(99) == 1 and setter(8) == 12        # clamped to 1 .. 12
    finally:
        setter(before)


@pytest.mark.gpu
def test_beyond_the_host_cap(hip_backend):
    f = PrimeField(backend=hip_backend)
    p = f.modulus
    rng = random.Random(0x5000)
    n = 5000
    xs, ys = elements(rng, p, n, distinct=True), elements(rng, p, n)
    with pytest.raises(GstarkError):
        f.interpolate(xs, ys)                                                # the host route stops at 4 096 points
    xv = f.newVectorFrom(xs)
    poly = f.interpolateAtPoints(xv, ys)
    assert poly.length == n and f.evalPolyAtPoints(poly, xv, method='tree').toValues() == ys
    picks = sorted(rng.sample(range(n), 16))
    coefficients = poly.toValues()
    assert ref_eval(coefficients, [xs[i] for i in picks], p) == [ys[i] for i in picks]
    m = f.polyFromRoots(xv)
    mv = m.toValues()
    members = set(xs)
    outsider = next(x for x in range(2, n + 3) if x not in members)
    assert len(mv) == n + 1 and mv[-1] == 1 and ref_eval(mv, [xs[i] for i in picks], p) == [0] * 16 and ref_eval(mv, [outsider], p) != [0]
    q, r = f.divModPolys(m, [-xs[7] % p, 1])
    assert r.toValues() == [0] and q.length == n and ref_eval(q.toValues(), [outsider], p)[0] * (outsider - xs[7]) % p == ref_eval(mv, [outsider], p)[0]
    q1, r1 = f.divModPolys([(mv[0] + 1) % p] + mv[1:], [-xs[7] % p, 1])
    assert r1.toValues() == [1] and q1.toBuffer() == q.toBuffer()


def check_seams(be, seed):
    seam_results(PrimeField(backend=be), seed)


other_flavour = flavour_fixture('q64', 'p224')


@pytest.mark.gpu
def test_other_flavours(other_flavour):
    check_seams(other_flavour, other_flavour.modulus % 65521)


@pytest.mark.gpu
def test_the_small_field_and_its_longest_transform():
    be = Backend(device=0, modulus=MODULUS_17)
    try:
        f = PrimeField(backend=be)
        assert f._polyOmega()[1] == 9                                        # 96 768 = 2^9 * 189
        rng = random.Random(0x17)
        check_from_roots(f, rng, (100,))
        check_division(f, rng, ((100, 37), (100, 1)), (100, 41))
        check_evaluation(f, rng, ((100, 100), (60, 100), (300, 100)))
        check_interpolation(f, rng, (100,))
        xs = elements(rng, MODULUS_17, 300, distinct=True)
        for attempt in (lambda: f.interpolateAtPoints(xs, xs), lambda: f.evalPolyAtPoints(xs, xs, method='tree'), lambda: f.divModPolys(list(range(1, 601)), [1, 2, 3])):
            with pytest.raises(GstarkError, match=r'omega_log2 is 9, this call needs transforms of 2\^1[01] points'):
                attempt()
        assert f.polyFromRoots(xs[:100]).toValues() == ref_from_roots(xs[:100], MODULUS_17)       # ... and the context goes on
    finally:
        be.close()


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    from test_runtime_modulus import PRIMES
    for q in (PRIMES[2], PRIMES[-1]):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(q)], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f'runtime poly: modulus {q} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
def test_refused_calls_enqueue_nothing(hip_backend):
    f = PrimeField(backend=hip_backend)
    p = f.modulus
    call, (omega, log2) = hip_backend.call, f._polyOmega()
    ptr = lambda v: C.c_void_p(v.ptr)
    xs, ys = f.newVectorFrom([3, 5, 8]), f.newVectorFrom([1, 4, 9])
    out, flag = f.newVectorFrom([7, 7, 7, 7]), Vector(hip_backend, 1, element_size=1)
    hip_backend.upload(flag.ptr, b'\x07')
    over = (1 << 20) + 1
    bad_omega = b'\xff' * hip_backend.element_size

    def good():
        """a valid call of every entry on the same context gives the right values"""
        call('gs_poly_from_roots', omega, log2, ptr(xs), 3, ptr(out))
        assert out.toValues() == ref_from_roots([3, 5, 8], p)
        q, r = f.newVector(2), f.newVector(2)
        call('gs_poly_div', omega, log2, ptr(out), 4, ptr(xs), 3, ptr(q), ptr(r))
        assert (q.toValues(), r.toValues()) == ref_divmod(ref_from_roots([3, 5, 8], p), [3, 5, 8], p)
        call('gs_poly_div', omega, log2, ptr(out), 4, ptr(xs), 3, None, ptr(r))       # either result may be left out
        call('gs_poly_div', omega, log2, ptr(out), 4, ptr(xs), 3, ptr(q), None)
        assert (q.toValues(), r.toValues()) == ref_divmod(ref_from_roots([3, 5, 8], p), [3, 5, 8], p)
        values = f.newVector(3)
        call('gs_poly_eval_points', omega, log2, ptr(ys), 3, ptr(xs), 3, ptr(values))
        assert values.toValues() == ref_eval([1, 4, 9], [3, 5, 8], p)
        coefficients = f.newVector(3)
        call('gs_poly_interpolate_points', omega, log2, ptr(xs), ptr(values), 3, ptr(coefficients), ptr(flag))
        assert coefficients.toValues() == [1, 4, 9] and flag.toBuffer() == b'\x00'
        hip_backend.upload(flag.ptr, b'\x07')
        hip_backend.upload(out.ptr, b''.join(f.le(7) for _ in range(4)))

    refusals = (
        ('gs_poly_from_roots', (omega, log2, ptr(xs), over, ptr(out)), 'n: at most'),
        ('gs_poly_div', (omega, log2, ptr(xs), over, ptr(xs), 3, ptr(out), None), 'la: at most'),
        ('gs_poly_div', (omega, log2, ptr(xs), 3, ptr(xs), over, ptr(out), None), 'lb: at most'),
        ('gs_poly_div', (omega, log2, ptr(xs), 0, ptr(xs), 3, ptr(out), None), 'la: at least'),
        ('gs_poly_eval_points', (omega, log2, ptr(xs), over, ptr(xs), 3, ptr(out)), 'len: at most'),
        ('gs_poly_eval_points', (omega, log2, ptr(xs), 3, ptr(xs), over, ptr(out)), 'npoints: at most'),
        ('gs_poly_interpolate_points', (omega, log2, ptr(xs), ptr(ys), over, ptr(out), ptr(flag)), 'n: at most'),
        ('gs_poly_from_roots', (omega, log2, None, 3, ptr(out)), 'xs is required'),
        ('gs_poly_from_roots', (omega, log2, ptr(xs), 3, None), 'out is required'),
        ('gs_poly_from_roots', (None, log2, ptr(xs), 3, ptr(out)), 'omega is required'),
        ('gs_poly_div', (omega, log2, None, 3, ptr(xs), 3, ptr(out), None), 'a is required'),
        ('gs_poly_div', (omega, log2, ptr(xs), 3, None, 3, ptr(out), None), 'b is required'),
        ('gs_poly_eval_points', (omega, log2, None, 3, ptr(xs), 3, ptr(out)), 'poly is required'),
        ('gs_poly_eval_points', (omega, log2, ptr(xs), 3, None, 3, ptr(out)), 'xs is required'),
        ('gs_poly_eval_points', (omega, log2, ptr(xs), 3, ptr(xs), 3, None), 'out is required'),
        ('gs_poly_interpolate_points', (omega, log2, None, ptr(ys), 3, ptr(out), ptr(flag)), 'xs is required'),
        ('gs_poly_interpolate_points', (omega, log2, ptr(xs), None, 3, ptr(out), ptr(flag)), 'ys is required'),
        ('gs_poly_interpolate_points', (omega, log2, ptr(xs), ptr(ys), 3, None, ptr(flag)), 'out is required'),
        ('gs_poly_interpolate_points', (omega, log2, ptr(xs), ptr(ys), 3, ptr(out), None), 'flag is required'),
        ('gs_poly_from_roots', (bad_omega, log2, ptr(xs), 3, ptr(out)), 'omega is not a canonical'),
        ('gs_poly_interpolate_points', (bad_omega, log2, ptr(xs), ptr(ys), 3, ptr(out), ptr(flag)), 'omega is not a canonical'),
        ('gs_poly_from_roots', (omega, log2 - 1, ptr(xs), 3, ptr(out)), rf'omega is not of order 2\^{log2 - 1}'),
    )
    for name, args, match in refusals:
        with pytest.raises(GstarkError, match=match):
            call(name, *args)
        assert out.toValues() == [7, 7, 7, 7] and flag.toBuffer() == b'\x07', name      # nothing was enqueued
        good()
    # an omega of too small an order for the plan: 2^8 points serve 64 roots ... and not 1 000 (transforms of 2^11 points)
    w8 = f.le(f.getRootOfUnity(1 << 8))
    big = f.newVectorFrom(list(range(1, 1001)))
    room = f.newVector(1001)
    call('gs_poly_from_roots', w8, 8, ptr(big), 64, ptr(room))
    assert room.toValues()[:65] == ref_from_roots(list(range(1, 65)), p)
    for name, args in (('gs_poly_from_roots', (w8, 8, ptr(big), 1000, ptr(room))), ('gs_poly_eval_points', (w8, 8, ptr(big), 1000, ptr(big), 1000, ptr(room))),
                       ('gs_poly_interpolate_points', (w8, 8, ptr(big), ptr(big), 1000, ptr(room), ptr(flag))), ('gs_poly_div', (w8, 8, ptr(big), 1000, ptr(big), 400, ptr(room), None))):
        with pytest.raises(GstarkError, match=r'omega_log2 is 8, this call needs transforms of 2\^1[01] points'):
            call(name, *args)
    assert flag.toBuffer() == b'\x07'
    zero_top = f.newVectorFrom([1, 2, 0])
    with pytest.raises(GstarkError, match=r'b: the leading coefficient b\[lb - 1\] is zero'):
        call('gs_poly_div', omega, log2, ptr(xs), 3, ptr(zero_top), 3, ptr(out), None)
    assert out.toValues() == [7, 7, 7, 7]
    good()


# ---- node -----------------------------------------------------------------------------------------------------------------------------------
def js_expectations(path):
    """what tests/js_poly.js must find, from the references: n = 257 and (600, 299) in the 128-bit field"""
    p = 2**128 - 9 * 2**32 + 1
    rng = random.Random(0x15)
    xs, ys, poly = elements(rng, p, 257, distinct=True), elements(rng, p, 257), elements(rng, p, 600)
    a, b = division_operands(rng, p, 600, 299)
    q, r = ref_divmod(a, b, p)
    few_x, few_y = xs[:12], ys[:12]
    text = lambda vs: [str(v) for v in vs]
    with open(path, 'w') as fh:
        json.dump({'modulus': str(p), 'xs': text(xs), 'ys': text(ys), 'poly': text(poly), 'a': text(a), 'b': text(b), 'q': text(q), 'r': text(r),
                   'from_roots': text(ref_from_roots(xs, p)), 'values': text(ref_eval(poly, xs, p)), 'few': text(ref_interpolate(few_x, few_y, p))}, fh)


@needs_node
def test_js_on_a_library_without_the_entries(tmp_path):
    """has() is false, the members throw an Error that names what is missing, interpolate is as before"""
    run_js('poly', 'double', tmp_path, js_expectations)


@needs_node
@pytest.mark.gpu
def test_js_on_hip(tmp_path):
    run_js('poly', 'hip', tmp_path, js_expectations)


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q, lib_path=_abi.HIP_LIB_PATH_RUNTIME)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    check_seams(be, q % 65521)
    print(f'runtime poly: modulus {q} ok')
