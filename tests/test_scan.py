"""Running sums, running products and linear recurrences on the device: include/gstark_scan.h, csrc/scan_plan.h, csrc/scan.hip, the
PrimeField members prefixSum* / prefixProduct* / sum* / prod* / linearRecurrence* / scanPlan (genstark_amd/field.py), and the same members of
js/galois.js.

Every comparison is against itertools.accumulate or a plain loop on Python integers, byte for byte.  CPU tier: the header, the binding
table, the host plan on its own under the sanitizers (tests/host_harness/scan_plan_host.cpp), and the whole Python layer on the tests'
double (which lacks the entries: the host fallback).  GPU tier: the lengths at which each level of the plan can go wrong (a lane, a wave,
a tile, more tile aggregates than one wave holds), values that wrap, reset or do not commute, uniform and flagged segments with their
heads on the seams, in-place calls, refused calls, the other flavours, one call at the cap, the grand product of a permutation check, node.
`python tests/test_scan.py runtime <q>` is the check of the runtime-modulus flavour (one modulus per process)."""
import ctypes as C
import itertools
import json
import os
import random
import re
import subprocess
import sys
import types

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pytest

from genstark_amd import _abi
from genstark_amd._abi import MODULUS_17, MODULUS_32, MODULUS_64, MODULUS_128, MODULUS_224, MODULUS_256, Backend, GstarkError
from genstark_amd.field import Matrix, PrimeField, Vector
from sponge_common import ROOT, check_header_is_plain_c, check_symbol_table, needs_node, run_js
from test_curve import p224_double      # noqa: F401 (fixture)

SECP256K1 = 2**256 - 2**32 - 977
CAP = 1 << 24
OPS = ('sum', 'product', 'affine')


# ---- the definitions, on Python integers --------------------------------------------------------------------------------------------------
def head_flags(n, cols=None, heads=None):
    """the head flag of every element: element 0, every multiple of cols, every byte with its low bit set"""
    return [i == 0 or bool(cols and i % cols == 0) or bool(heads is not None and heads[i] & 1) for i in range(n)]


def segments(values, flags):
    """the values cut where a flag is set"""
    out = []
    for v, h in zip(values, flags):
        if h:
            out.append([])
        out[-1].append(v)
    return out


def ref_scan(p, op, values, flags, exclusive):
    """sum or product: itertools.accumulate over every segment on its own"""
    start, step = (0, lambda x, y: (x + y) % p) if op == 'sum' else (1, lambda x, y: x * y % p)
    out = []
    for seg in segments(values, flags):
        run = list(itertools.accumulate(seg, step, initial=start))
        out += run[:-1] if exclusive else run[1:]
    return out


def ref_affine(p, a, b, flags, x0, exclusive):
    """x[i] = a[i] * x[i-1] + b[i], every segment from x0: a plain loop"""
    out, x = [], x0
    for i, (bi, h) in enumerate(zip(b, flags)):
        if h:
            x = x0
        before = x
        x = ((a if isinstance(a, int) else a[i]) * x + bi) % p
        out.append(before if exclusive else x)
    return out


def ref_totals(p, op, values, rows, cols):
    return [ref_scan(p, op, values[r * cols:(r + 1) * cols], head_flags(cols), False)[-1] for r in range(rows)]


def le(f, values):
    return b''.join(f.le(v) for v in values)


def flag_vector(f, heads):
    v = Vector(f.backend, len(heads), element_size=1)
    if heads:
        f.backend.upload(v.ptr, bytes(heads))
    return v


def check_vector_forms(f, rng, n, ops=OPS, heads=None, a_values=None, values=None, b_values=None, x0=None):
    """every op, inclusive and exclusive, of one vector of n elements (random unless given) against the definitions, byte for byte"""
    p = f.modulus
    flags = head_flags(n, heads=heads)
    hv = flag_vector(f, heads) if heads is not None else None
    values = values if values is not None else [rng.randrange(p) for _ in range(n)]
    vec = f.newVectorFrom(values)
    for op in ops:
        for exclusive in (False, True):
            if op == 'affine':
                a = a_values if a_values is not None else [rng.randrange(p) for _ in range(n)]
                b = b_values if b_values is not None else values
                start = x0 if x0 is not None else rng.randrange(p)
                got = f.linearRecurrence(a if isinstance(a, int) else f.newVectorFrom(a), vec if b is values else f.newVectorFrom(b), start, exclusive, hv)
                want = ref_affine(p, a, b, flags, start, exclusive)
            else:
                member = f.prefixSumVectorElements if op == 'sum' else f.prefixProductVectorElements
                got = member(vec, exclusive, hv)
                want = ref_scan(p, op, values, flags, exclusive)
            assert isinstance(got, Vector) and got.length == n
            assert got.toBuffer() == le(f, want), (op, exclusive, n)
    assert vec.toBuffer() == le(f, values)                                   # the input is as it was


# ---- CPU tier: header, binding table, plan ----------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    check_header_is_plain_c('scan')


def test_symbol_table_matches_the_header():
    others = [getattr(_abi, name) for name in dir(_abi) if name.endswith('_SYMBOLS') and name != 'SCAN_SYMBOLS']
    assert len(others) >= 12
    check_symbol_table('scan', _abi.SCAN_SYMBOLS, others)
    header = open(os.path.join(ROOT, 'include', 'gstark_scan.h')).read()
    assert set(re.findall(r'\b(gs_\w+)\(', header)) == set(_abi.SCAN_SYMBOLS) == {'gs_scan', 'gs_scan_affine', 'gs_reduce', 'gs_scan_plan'}
    assert '2^24' in header and 'never `a`' in header


def test_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'scan_plan_host')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-omit-frame-pointer', os.path.join(ROOT, 'tests', 'host_harness', 'scan_plan_host.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'scan plan OK' in r.stdout and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


# ---- CPU tier: the Python layer on the host fallback ------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=['p128', 'p224'])
def double_field(request, oracle_backend, p224_double):
    be = oracle_backend if request.param == 'p128' else p224_double
    assert not any(hasattr(be.lib, name) for name in _abi.SCAN_SYMBOLS)
    return PrimeField(backend=be)


def test_the_fallback_on_vectors(double_field):
    f, p = double_field, double_field.modulus
    assert f.scanPlan() is None
    rng = random.Random(0x5CA9)
    for n in (0, 1, 2, 7, 100):
        check_vector_forms(f, rng, n)
        check_vector_forms(f, rng, n, heads=[rng.randrange(256) for _ in range(n)])
        check_vector_forms(f, rng, n, ops=('affine',), a_values=rng.randrange(p))
    values = [rng.randrange(p) for _ in range(50)]
    assert f.prefixSumVectorElements(values).toValues() == list(itertools.accumulate(values, lambda x, y: (x + y) % p))      # lists in, a Vector out
    assert f.prefixProductVectorElements(values, True).toValues() == [1] + list(itertools.accumulate(values, lambda x, y: x * y % p))[:-1]
    heads = [0] * 50
    heads[0], heads[20], heads[21] = 0, 1, 3
    assert f.prefixSumVectorElements(values, heads=heads).toValues() == ref_scan(p, 'sum', values, head_flags(50, heads=heads), False)
    assert f.linearRecurrence(values, values[::-1], 5).toValues() == ref_affine(p, values, values[::-1], head_flags(50), 5, False)
    assert f.linearRecurrence(3, [1] * 10).toValues() == [(3**(i + 1) - 1) // 2 % p for i in range(10)]                       # a geometric sum
    x = rng.randrange(p)
    assert f.linearRecurrence(x, values).toValues()[-1] == sum(c * pow(x, 49 - i, p) for i, c in enumerate(values)) % p       # a Horner chain
    assert f.linearRecurrence(2, [0] * 4, x0=1, exclusive=True).toValues() == [1, 2, 4, 8]
    assert f.sumVectorElements(values) == sum(values) % p and f.sumVectorElements(f.newVectorFrom(values)) == sum(values) % p
    prod = 1
    for v in values:
        prod = prod * v % p
    assert f.prodVectorElements(values) == prod and f.prodVectorElements(f.newVectorFrom(values)) == prod
    assert f.sumVectorElements([]) == 0 and f.prodVectorElements([]) == 1 and f.prefixSumVectorElements([]).length == 0
    zeros = [3, 0, 5, 7, 2, 9]
    assert f.prefixProductVectorElements(zeros, heads=[0, 0, 0, 1, 0, 0]).toValues() == [3, 0, 0, 7, 14, 126]                  # a zero stays in its segment


def test_the_fallback_on_matrices(double_field):
    f, p = double_field, double_field.modulus
    rng = random.Random(0x5CAA)
    for rows, cols in ((1, 1), (3, 1), (1, 9), (5, 7)):
        n = rows * cols
        values, factors = [rng.randrange(p) for _ in range(n)], [rng.randrange(p) for _ in range(n)]
        nested = lambda flat: [flat[r * cols:(r + 1) * cols] for r in range(rows)]
        flags = head_flags(n, cols)
        m = f.newMatrixFrom(nested(values))
        for op, member, reduce_member in (('sum', f.prefixSumMatrixRows, f.sumMatrixRows), ('product', f.prefixProductMatrixRows, f.prodMatrixRows)):
            for exclusive in (False, True):
                got = member(m, exclusive)
                assert isinstance(got, Matrix) and (got.rowCount, got.colCount) == (rows, cols)
                assert got.toBuffer() == le(f, ref_scan(p, op, values, flags, exclusive))
                got, totals = member(nested(values), exclusive, totals=True)
                assert got.toBuffer() == le(f, ref_scan(p, op, values, flags, exclusive))
                assert isinstance(totals, Vector) and totals.toBuffer() == le(f, ref_totals(p, op, values, rows, cols))
            assert reduce_member(m).toBuffer() == reduce_member(nested(values)).toBuffer() == le(f, ref_totals(p, op, values, rows, cols))
        for exclusive in (False, True):
            x0 = rng.randrange(p)
            got = f.linearRecurrenceMatrixRows(f.newMatrixFrom(nested(factors)), m, x0, exclusive)
            assert isinstance(got, Matrix) and got.toBuffer() == le(f, ref_affine(p, factors, values, flags, x0, exclusive))
            assert f.linearRecurrenceMatrixRows(7, nested(values), x0, exclusive).toBuffer() == le(f, ref_affine(p, 7, values, flags, x0, exclusive))
    empty = f.prefixSumMatrixRows([])
    assert isinstance(empty, Matrix) and empty.rowCount == 0 and f.sumMatrixRows([]).length == 0


def test_bad_shapes_raise(double_field):
    f, p, be = double_field, double_field.modulus, double_field.backend
    other = 1 if f.elementSize != 1 else 2
    with pytest.raises(GstarkError, match='lengths differ'):
        f.linearRecurrence([1, 2, 3], [1, 2])
    with pytest.raises(GstarkError, match='lengths differ'):
        f.linearRecurrence(f.newVectorFrom([1, 2]), f.newVectorFrom([1, 2, 3]))
    with pytest.raises(GstarkError, match='shapes differ'):
        f.linearRecurrenceMatrixRows([[1, 2], [3, 4]], [[1, 2, 3, 4]])
    with pytest.raises(GstarkError, match='different lengths'):
        f.prefixSumMatrixRows([[1, 2], [3]])
    for attempt in (lambda: f.prefixSumVectorElements([p]), lambda: f.prefixProductVectorElements([-1]), lambda: f.sumVectorElements([p + 1]),
                    lambda: f.prodMatrixRows([[p]]), lambda: f.linearRecurrence(p, [1]), lambda: f.linearRecurrence([p], [1]), lambda: f.linearRecurrence([1], [p]),
                    lambda: f.linearRecurrence(1, [1], x0=p), lambda: f.linearRecurrenceMatrixRows(1, [[1]], x0=-1)):
        with pytest.raises(GstarkError, match='canonical'):
            attempt()
    with pytest.raises(GstarkError, match='integers'):
        f.prefixSumVectorElements([None])
    with pytest.raises(GstarkError, match='x0 is an integer'):
        f.linearRecurrence(1, [1], x0=None)
    with pytest.raises(GstarkError, match='3 heads and 2 values'):
        f.prefixSumVectorElements([1, 2], heads=[1, 0, 0])
    with pytest.raises(GstarkError, match='1 heads and 2 values'):
        f.linearRecurrence(1, [1, 2], heads=Vector(be, 1, element_size=1))
    with pytest.raises(GstarkError, match='heads is a vector of bytes'):
        f.prefixProductVectorElements([1, 2], heads=f.newVectorFrom([1, 0]))
    with pytest.raises(GstarkError, match='heads are bytes'):
        f.prefixSumVectorElements([1, 2], heads=[0, 256])
    with pytest.raises(GstarkError, match=f'{other}-byte entries'):
        f.prefixSumVectorElements(Vector(be, 4, element_size=other))
    with pytest.raises(GstarkError, match='not a Matrix'):
        f.prefixSumVectorElements(f.newMatrixFrom([[1, 2]]))
    with pytest.raises(GstarkError, match='not a Vector'):
        f.sumMatrixRows(f.newVectorFrom([1, 2]))
    with pytest.raises(GstarkError, match='0 columns'):
        f.prefixSumMatrixRows([[], []])
    owner = f.newVectorFrom([0])._owner                                      # views that claim 2^24 + 1 elements: refused before anything reads them
    big, wide = Vector(be, CAP + 1, owner=owner), Matrix(be, 4097, 4096, owner=owner)
    for attempt in (lambda: f.prefixSumVectorElements(big), lambda: f.prefixProductVectorElements(big), lambda: f.sumVectorElements(big), lambda: f.prodVectorElements(big),
                    lambda: f.linearRecurrence(1, big), lambda: f.linearRecurrence(big, big), lambda: f.prefixSumMatrixRows(wide), lambda: f.prodMatrixRows(wide),
                    lambda: f.linearRecurrenceMatrixRows(1, wide)):
        with pytest.raises(GstarkError, match=r'at most 2\^24'):
            attempt()


def test_a_device_library_without_the_entries_is_an_error(p224_double):
    """no quiet host path where a HIP library lacks only these entries: the double's library under the product backend's name"""
    named = types.SimpleNamespace(name='hip-gfx950', lib=p224_double.lib, element_size=32)
    f = PrimeField(backend=p224_double)
    f.backend = named
    for attempt in (lambda: f.prefixSumVectorElements([4]), lambda: f.prefixProductVectorElements([4]), lambda: f.sumVectorElements([4]), lambda: f.prodVectorElements([4]),
                    lambda: f.prefixSumMatrixRows([[4]]), lambda: f.prefixProductMatrixRows([[4]]), lambda: f.sumMatrixRows([[4]]), lambda: f.prodMatrixRows([[4]]),
                    lambda: f.linearRecurrence(1, [4]), lambda: f.linearRecurrenceMatrixRows(1, [[4]]), f.scanPlan):
        with pytest.raises(GstarkError, match=r'no gs_scan \(include/gstark_scan\.h\)'):
            attempt()
    named.lib = types.SimpleNamespace(gs_scan=1, gs_reduce=1, gs_scan_plan=1)          # ... and the other entry is named when it is the one missing
    with pytest.raises(GstarkError, match=r'no gs_scan_affine \(include/gstark_scan\.h\)'):
        f.linearRecurrence(1, [4])


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def f128(hip_backend):
    f = PrimeField(backend=hip_backend)
    plan = f.scanPlan()
    assert plan['maxElements'] == CAP and plan['tile'] == 256 * plan['elementsPerThread'] and plan['elementsPerThread'] * f.elementSize == 64
    return f


def plan_lengths(f):
    plan = f.scanPlan()
    T, E = plan['tile'], plan['elementsPerThread']
    return T, E, (1, 2, 63, 64, 65, 64 * E - 1, 64 * E, 64 * E + 1, T - 1, T, T + 1, 2 * T + 1, 65 * T + 3)


@pytest.mark.gpu
@pytest.mark.parametrize('op', OPS)
def test_lengths_at_every_level_of_the_plan(f128, op):
    T, E, lengths = plan_lengths(f128)
    assert 65 * T + 3 > 64 * T                                               # more tile aggregates than one wave holds
    assert [f128.scanPlan(n)['launches'] for n in (0, 1, T, T + 1, 65 * T + 3, CAP, CAP + 1)] == [0, 1, 1, 3, 3, 3, 0]
    rng = random.Random(0x5CAB)
    for n in lengths:
        check_vector_forms(f128, rng, n, ops=(op,))


@pytest.mark.gpu
def test_values_that_matter(f128):
    f, p = f128, f128.modulus
    T, E, _ = plan_lengths(f)
    rng = random.Random(0x5CAC)
    n = 2 * T + 1
    check_vector_forms(f, rng, n, ops=('sum',), values=[p - 1] * n)          # sums that wrap p at every step
    for zero_at in (T - 1, T):                                               # a zero at the last element of a tile, at the first of the next
        values = [rng.randrange(1, p) for _ in range(n)]
        values[zero_at] = 0
        check_vector_forms(f, rng, n, ops=('product',), values=values)
    a = [rng.randrange(1, p) for _ in range(n)]
    for k in (0, 1, 63, 64, 4 * E * 64 - 1, T - 1, T, T + 1, 2 * T):          # zeros in a: the chain forgets what came before
        a[k] = 0
    check_vector_forms(f, rng, n, ops=('affine',), a_values=a)
    # random (a, b) do not commute: composing any two neighbours the other way round gives another answer
    a, b = [rng.randrange(2, p) for _ in range(n)], [rng.randrange(1, p) for _ in range(n)]
    assert all((a[i + 1] * b[i] + b[i + 1]) % p != (a[i] * b[i + 1] + b[i]) % p for i in range(n - 1))
    check_vector_forms(f, rng, n, ops=('affine',), a_values=a, b_values=b)
    for scalar in (0, 1, p - 1, rng.randrange(p)):                           # a as ONE scalar
        check_vector_forms(f, rng, n, ops=('affine',), a_values=scalar)
    check_vector_forms(f, rng, n, ops=('affine',), a_values=scalar, x0=0)
    assert f.sumVectorElements(f.newVectorFrom([p - 1] * n)) == (p - 1) * n % p
    assert f.prodVectorElements(f.newVectorFrom(b)) == ref_scan(p, 'product', b, head_flags(n), False)[-1]
    assert f.prodVectorElements(f.newVectorFrom(b[:T])) == ref_scan(p, 'product', b[:T], head_flags(T), False)[-1]           # one launch


UNIFORM_COLS = ('1', '3', '64', '65', 'T + 1', '3T + 5')


def uniform_shape(T, which):
    cols = eval(which.replace('3T', '3 * T'), {'T': T})
    return (3 * T) // cols + 2, cols


def head_properties(T, E, n, cols):
    """which of the seams the heads of `rows` uniform segments fall on"""
    heads = range(0, n, cols)
    lane = lambda i: (i % T) // E % 64
    per_tile = [sum(1 for i in heads if i // T == t) for t in range((n + T - 1) // T)]
    found = set()
    found |= {'first lane of a wave'} if any(lane(i) == 0 for i in heads if i) else set()
    found |= {'last lane of a wave'} if any(lane(i) == 63 for i in heads) else set()
    found |= {'first element of a tile'} if any(i % T == 0 for i in heads if i) else set()
    found |= {'last element of a tile'} if any(i % T == T - 1 for i in heads) else set()
    found |= {'a tile with no head'} if any(c == 0 for c in per_tile) else set()
    found |= {'a tile with many heads'} if any(c >= 16 for c in per_tile) else set()
    return found


@pytest.mark.gpu
def test_uniform_segments_cover_every_seam(f128):
    """from T, E and the list of cols alone: a later change of the tile cannot silently drop a case"""
    T, E, _ = plan_lengths(f128)
    found, found_beyond_one = set(), set()
    for which in UNIFORM_COLS:
        rows, cols = uniform_shape(T, which)
        assert rows * cols > 2 * T + 1 and (rows * cols + T - 1) // T >= 3, which      # the total crosses at least three tiles
        props = head_properties(T, E, rows * cols, cols)
        found |= props
        found_beyond_one |= props if cols > 1 else set()
    every = {'first lane of a wave', 'last lane of a wave', 'first element of a tile', 'last element of a tile', 'a tile with no head', 'a tile with many heads'}
    assert found == every and found_beyond_one == every


@pytest.mark.gpu
@pytest.mark.parametrize('which', UNIFORM_COLS)
def test_uniform_segments(f128, which):
    f, p = f128, f128.modulus
    T, E, _ = plan_lengths(f)
    rows, cols = uniform_shape(T, which)
    n = rows * cols
    rng = random.Random(0x5CAD + cols)
    values, factors = [rng.randrange(p) for _ in range(n)], [rng.randrange(p) for _ in range(n)]
    flags = head_flags(n, cols)
    m, am = Matrix(f.backend, rows, cols), Matrix(f.backend, rows, cols)
    f.backend.upload(m.ptr, le(f, values))
    f.backend.upload(am.ptr, le(f, factors))
    for op, member, reduce_member in (('sum', f.prefixSumMatrixRows, f.sumMatrixRows), ('product', f.prefixProductMatrixRows, f.prodMatrixRows)):
        want_totals = le(f, ref_totals(p, op, values, rows, cols))
        for exclusive in (False, True):
            want = le(f, ref_scan(p, op, values, flags, exclusive))
            assert member(m, exclusive).toBuffer() == want, (op, exclusive)
            got, totals = member(m, exclusive, totals=True)
            assert got.toBuffer() == want and totals.toBuffer() == want_totals, (op, exclusive)
        assert reduce_member(m).toBuffer() == want_totals                    # the reduction alone gives the same totals
    for exclusive in (False, True):
        x0 = rng.randrange(p)
        assert f.linearRecurrenceMatrixRows(am, m, x0, exclusive).toBuffer() == le(f, ref_affine(p, factors, values, flags, x0, exclusive))
        assert f.linearRecurrenceMatrixRows(factors[0], m, x0, exclusive).toBuffer() == le(f, ref_affine(p, factors[0], values, flags, x0, exclusive))
    assert m.toBuffer() == le(f, values)


@pytest.mark.gpu
def test_rows_within_one_tile(f128):
    """one launch: rows, totals and the reduction with no carry anywhere"""
    f, p = f128, f128.modulus
    T, E, _ = plan_lengths(f)
    rng = random.Random(0x5CB3)
    for rows, cols in ((1, 1), (3, 5), (E + 1, 63), (T // 8, 8), (1, T)):
        n = rows * cols
        assert f.scanPlan(n)['launches'] == 1
        values = [rng.randrange(p) for _ in range(n)]
        nested, flags = [values[r * cols:(r + 1) * cols] for r in range(rows)], head_flags(n, cols)
        for op, member, reduce_member in (('sum', f.prefixSumMatrixRows, f.sumMatrixRows), ('product', f.prefixProductMatrixRows, f.prodMatrixRows)):
            for exclusive in (False, True):
                got, totals = member(nested, exclusive, totals=True)
                assert got.toBuffer() == le(f, ref_scan(p, op, values, flags, exclusive)) and totals.toBuffer() == le(f, ref_totals(p, op, values, rows, cols))
            assert reduce_member(nested).toBuffer() == le(f, ref_totals(p, op, values, rows, cols))
        assert f.linearRecurrenceMatrixRows(nested, nested, 9, True).toBuffer() == le(f, ref_affine(p, values, values, flags, 9, True))


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['1/7', '1/5000', 'all ones', 'all zeros', 'first byte 0', 'high bits', 'a zero segment'])
def test_flagged_segments(f128, which):
    f, p = f128, f128.modulus
    T, E, _ = plan_lengths(f)
    n = 9 * T + 1
    rng = random.Random(0x5CAE)
    values = None
    if which in ('1/7', '1/5000'):
        density = 7 if which == '1/7' else 5000
        heads = [1 if rng.randrange(density) == 0 else 0 for _ in range(n)]
        assert any(heads)
    elif which == 'all ones':
        heads = [1] * n
    elif which == 'all zeros':
        heads = [0] * n
    elif which == 'first byte 0':
        heads = [0] + [1 if rng.randrange(100) == 0 else 0 for _ in range(n - 1)]
    elif which == 'high bits':                                               # only the low bit counts
        heads = [rng.randrange(256) & 0xfe if rng.randrange(7) else rng.randrange(256) | 1 for _ in range(n)]
        assert any(h > 1 and not h & 1 for h in heads) and any(h > 1 and h & 1 for h in heads)
    else:                                                                    # a segment with a zero, then a segment that must recover
        heads = [1 if i % (T // 2 + 3) == 0 else 0 for i in range(n)]
        values = [rng.randrange(1, p) for _ in range(n)]
        values[T // 2 + 5] = 0
        want = ref_scan(p, 'product', values, head_flags(n, heads=heads), False)
        assert want[T // 2 + 3 + T // 2 + 2] == 0 and all(want[T + 6:])       # zero to the end of its segment, and nowhere after
    check_vector_forms(f, rng, n, heads=heads, values=values)


@pytest.mark.gpu
def test_in_place_and_refused_overlaps(f128):
    f, p, be = f128, f128.modulus, f128.backend
    T, E, _ = plan_lengths(f)
    n, es = 2 * T + 1, f.elementSize
    rng = random.Random(0x5CAF)
    values, factors = [rng.randrange(p) for _ in range(n)], [rng.randrange(p) for _ in range(n)]
    flags, ptr = head_flags(n), lambda v, off=0: C.c_void_p(v.ptr + off * es)
    for op in (0, 1):
        for exclusive in (0, 1):
            v = f.newVectorFrom(values)
            be.call('gs_scan', op, exclusive, ptr(v), None, 1, n, ptr(v), None)                   # out is values
            assert v.toBuffer() == le(f, ref_scan(p, OPS[op], values, flags, bool(exclusive)))
    x0 = rng.randrange(p)
    for exclusive in (0, 1):
        a, b = f.newVectorFrom(factors), f.newVectorFrom(values)
        be.call('gs_scan_affine', exclusive, ptr(a), None, ptr(b), f.le(x0), None, 1, n, ptr(b))      # out is b
        assert b.toBuffer() == le(f, ref_affine(p, factors, values, flags, x0, bool(exclusive))) and a.toBuffer() == le(f, factors)
    a, b, out = f.newVectorFrom(factors), f.newVectorFrom(values), f.newVectorFrom([7] * n)
    with pytest.raises(GstarkError, match='overlaps a'):
        be.call('gs_scan_affine', 0, ptr(a), None, ptr(b), f.le(x0), None, 1, n, ptr(a))             # never a
    with pytest.raises(GstarkError, match='overlaps a'):
        be.call('gs_scan_affine', 0, ptr(a), None, ptr(b), f.le(x0), None, 1, n - 1, ptr(a, 1))
    for shift in (1, T):                                                     # a shifted overlap, either way: all but one element in common, and one
        with pytest.raises(GstarkError, match='without being exactly the input'):
            be.call('gs_scan', 0, 0, ptr(b), None, 1, n - shift, ptr(b, shift), None)
        with pytest.raises(GstarkError, match='without being exactly the input'):
            be.call('gs_scan', 1, 0, ptr(b, shift), None, 1, n - shift, ptr(b), None)
        with pytest.raises(GstarkError, match='without being exactly the input'):
            be.call('gs_scan_affine', 0, ptr(a), None, ptr(b), f.le(x0), None, 1, n - shift, ptr(b, shift))
    with pytest.raises(GstarkError, match='totals_out overlaps'):
        be.call('gs_scan', 0, 0, ptr(b), None, 1, n, ptr(out), ptr(b, 5))
    with pytest.raises(GstarkError, match='totals_out overlaps'):
        be.call('gs_reduce', 0, ptr(b), 1, n, ptr(b))
    assert a.toBuffer() == le(f, factors) and b.toBuffer() == le(f, values) and out.toBuffer() == le(f, [7] * n)             # nothing was enqueued
    be.call('gs_scan_affine', 0, ptr(a), None, ptr(b), f.le(x0), None, 1, n, ptr(out))               # ... and the context is as usable as before
    assert out.toBuffer() == le(f, ref_affine(p, factors, values, flags, x0, False))


@pytest.mark.gpu
def test_refused_calls_leave_the_context_usable(f128):
    f, p, be = f128, f128.modulus, f128.backend
    T, E, _ = plan_lengths(f)
    n = T + 1
    rng = random.Random(0x5CB0)
    values = [rng.randrange(p) for _ in range(n)]
    v, out = f.newVectorFrom(values), f.newVectorFrom([7] * n)
    ptr = lambda x: C.c_void_p(x.ptr)
    want = {op: le(f, ref_scan(p, op, values, head_flags(n), False)) for op in ('sum', 'product')}
    want['affine'] = le(f, ref_affine(p, 3, values, head_flags(n), 0, False))

    def correct_call_gives_correct_bytes():
        assert f.prefixSumVectorElements(v).toBuffer() == want['sum'] and f.prefixProductVectorElements(v).toBuffer() == want['product']
        assert f.linearRecurrence(3, v).toBuffer() == want['affine']

    refused = [
        (r'at most 2\^24', lambda: be.call('gs_scan', 0, 0, ptr(v), None, 1, CAP + 1, ptr(out), None)),
        (r'at most 2\^24', lambda: be.call('gs_scan', 1, 0, ptr(v), None, 4097, 4096, ptr(out), None)),
        (r'at most 2\^24', lambda: be.call('gs_scan', 1, 0, ptr(v), None, 1 << 63, 2, ptr(out), None)),                   # rows * cols wraps to 0
        (r'at most 2\^24', lambda: be.call('gs_scan_affine', 0, None, f.le(3), ptr(v), None, None, 1, CAP + 1, ptr(out))),
        (r'at most 2\^24', lambda: be.call('gs_reduce', 0, ptr(v), CAP + 1, 1, ptr(out))),
        ('cols is 0', lambda: be.call('gs_scan', 0, 0, ptr(v), None, 3, 0, ptr(out), None)),
        ('cols is 0', lambda: be.call('gs_scan_affine', 0, None, f.le(3), ptr(v), None, None, 3, 0, ptr(out))),
        ('cols is 0', lambda: be.call('gs_reduce', 1, ptr(v), 3, 0, ptr(out))),
        ('op is GS_SCAN_SUM or GS_SCAN_PRODUCT, not 2', lambda: be.call('gs_scan', 2, 0, ptr(v), None, 1, n, ptr(out), None)),   # an unknown op
        ('op is GS_SCAN_SUM or GS_SCAN_PRODUCT, not -1', lambda: be.call('gs_reduce', -1, ptr(v), 1, n, ptr(out))),
        ('1-byte entries', lambda: f.prefixSumVectorElements(Vector(be, n, element_size=1))),                               # an element-size mismatch
        ('heads is a vector of bytes', lambda: f.prefixSumVectorElements(v, heads=f.newVectorFrom([1] * n))),
        ('canonical', lambda: be.call('gs_scan_affine', 0, None, b'\xff' * f.elementSize, ptr(v), None, None, 1, n, ptr(out))),
        ('canonical', lambda: be.call('gs_scan_affine', 0, None, f.le(3), ptr(v), f.le(p), None, 1, n, ptr(out))),
        ('required', lambda: be.call('gs_scan', 0, 0, None, None, 1, n, ptr(out), None)),
        ('required', lambda: be.call('gs_scan', 0, 0, ptr(v), None, 1, n, None, None)),
        ('heads go with rows == 1', lambda: be.call('gs_scan', 0, 0, ptr(v), ptr(flag_vector(f, [1] * n)), 2, n // 2, ptr(out), None)),
    ]
    for message, attempt in refused:
        with pytest.raises(GstarkError, match=message):
            attempt()
        assert out.toBuffer() == le(f, [7] * n)                              # nothing was enqueued
        correct_call_gives_correct_bytes()
    assert be.lib.gs_scan(None, 0, 0, ptr(v), None, 1, n, ptr(out), None) == -1                   # GS_ERR_ARG without a context
    be.call('gs_scan', 0, 0, None, None, 0, 0, None, None)                   # 0 elements does nothing
    be.call('gs_scan', 0, 0, None, None, 0, 5, None, None)
    be.call('gs_scan_affine', 0, None, f.le(3), None, None, None, 0, 0, None)
    be.call('gs_reduce', 0, None, 0, 0, None)
    assert out.toBuffer() == le(f, [7] * n)


def check_a_flavour(f, rng):
    """all three ops at 2T + 1 and one uniform-segment case"""
    p = f.modulus
    T, E, _ = plan_lengths(f)
    assert E * f.elementSize == 64 and T == 256 * E
    check_vector_forms(f, rng, 2 * T + 1)
    rows, cols = 5, T // 2 + 3
    values = [rng.randrange(p) for _ in range(rows * cols)]
    nested = [values[r * cols:(r + 1) * cols] for r in range(rows)]
    flags = head_flags(rows * cols, cols)
    got, totals = f.prefixProductMatrixRows(nested, totals=True)
    assert got.toBuffer() == le(f, ref_scan(p, 'product', values, flags, False)) and totals.toBuffer() == le(f, ref_totals(p, 'product', values, rows, cols))
    assert f.prefixSumMatrixRows(nested, True).toBuffer() == le(f, ref_scan(p, 'sum', values, flags, True))
    assert f.sumMatrixRows(nested).toBuffer() == le(f, ref_totals(p, 'sum', values, rows, cols))
    assert f.linearRecurrenceMatrixRows(nested, nested, 5).toBuffer() == le(f, ref_affine(p, values, values, flags, 5, False))


@pytest.mark.gpu
@pytest.mark.parametrize('modulus', [MODULUS_64, MODULUS_32, MODULUS_17, MODULUS_256, MODULUS_224], ids=['q64', 'q32', 'q17', 'p256', 'p224'])
def test_other_flavours(modulus):
    be = Backend(device=0, modulus=modulus)
    try:
        check_a_flavour(PrimeField(backend=be), random.Random(modulus % 65521))
    finally:
        be.close()


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(SECP256K1)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'runtime scan: modulus {SECP256K1} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
def test_one_call_at_the_cap(f128):
    """max_elements in one call, built and checked with vector members on the device; no Python loop runs over the values"""
    f, p = f128, f128.modulus
    n = f.scanPlan()['maxElements']
    assert n == CAP and f.scanPlan(n)['launches'] == 3
    g = 0x1234567 * 2**64 + 0x89abcdef
    series = f.getPowerSeries(g, n)                                          # g^i
    constant = f.mulVectorElements(f.getPowerSeries(1, n), g)               # g, n times
    want = f.mulVectorElements(series, g).toBuffer()                        # g^(i+1)
    assert want[:f.elementSize] == f.le(g) and want[-f.elementSize:] == f.le(pow(g, n, p))
    assert f.prefixProductVectorElements(constant).toBuffer() == want
    sums = f.prefixSumVectorElements(series)                                 # (g^(i+1) - 1) / (g - 1)
    assert f.addVectorElements(f.mulVectorElements(sums, g - 1), 1).toBuffer() == want
    chain = f.linearRecurrence(g, f.getPowerSeries(1, n))                    # the same geometric sums as a recurrence: x[i] = g * x[i-1] + 1
    assert f.addVectorElements(f.mulVectorElements(chain, g - 1), 1).toBuffer() == want


@pytest.mark.gpu
def test_the_grand_product_of_a_permutation_check(f128):
    f, p = f128, f128.modulus
    T, E, _ = plan_lengths(f)
    n = 2 * T + 1
    rng = random.Random(0x5CB1)
    a = [rng.randrange(p) for _ in range(n)]
    b = list(a)
    rng.shuffle(b)
    gamma = rng.randrange(p)
    assert all((x + gamma) % p for x in a)
    av, bv = f.newVectorFrom(a), f.newVectorFrom(b)
    ratios = f.divVectorElements(f.addVectorElements(av, gamma), f.addVectorElements(bv, gamma))
    running = f.prefixProductVectorElements(ratios)
    assert running.getValue(n - 1) == 1 and running.getValue(n // 2) != 1 and f.prodVectorElements(ratios) == 1
    b[T + 1] = (b[T + 1] + 1) % p                                            # no longer a permutation
    ratios = f.divVectorElements(f.addVectorElements(av, gamma), f.addVectorElements(f.newVectorFrom(b), gamma))
    assert f.prefixProductVectorElements(ratios).getValue(n - 1) != 1 and f.prodVectorElements(ratios) != 1


# ---- node -------------------------------------------------------------------------------------------------------------------------------
JS_T = 1024                                                                  # the tile of the 128-bit field (asserted against the plan in js_scan.js)


def js_expectations(path):
    """what tests/js_scan.js must find, from host integers: the three ops, both forms, one vector, uniform and flagged segments at T + 1
    and 2T + 1 in the 128-bit field"""
    p = MODULUS_128
    rng = random.Random(0x5CB2)
    cases = []
    for n in (JS_T + 1, 2 * JS_T + 1):
        values, factors = [rng.randrange(p) for _ in range(n)], [rng.randrange(p) for _ in range(n)]
        heads = [1 if rng.randrange(7) == 0 else rng.randrange(256) & 0xfe for _ in range(n)]
        cols = next(c for c in (3, 5, 7, 25, 41, 683) if n % c == 0)
        x0 = rng.randrange(p)
        case = {'n': n, 'values': [str(v) for v in values], 'factors': [str(v) for v in factors], 'heads': heads, 'cols': cols, 'x0': str(x0), 'want': {}}
        for form, flags in (('vector', head_flags(n)), ('flagged', head_flags(n, heads=heads)), ('uniform', head_flags(n, cols))):
            for exclusive in (False, True):
                key = f'{form}/{"exclusive" if exclusive else "inclusive"}'
                case['want'][f'sum/{key}'] = [str(v) for v in ref_scan(p, 'sum', values, flags, exclusive)]
                case['want'][f'product/{key}'] = [str(v) for v in ref_scan(p, 'product', values, flags, exclusive)]
                case['want'][f'affine/{key}'] = [str(v) for v in ref_affine(p, factors, values, flags, x0, exclusive)]
                case['want'][f'scalar/{key}'] = [str(v) for v in ref_affine(p, factors[0], values, flags, x0, exclusive)]
        case['totals'] = {op: [str(v) for v in ref_totals(p, op, values, n // cols, cols)] for op in ('sum', 'product')}
        cases.append(case)
    with open(path, 'w') as fh:
        json.dump({'modulus': str(p), 'tile': JS_T, 'cases': cases}, fh)


@needs_node
def test_js_on_a_library_without_the_entries(tmp_path):
    """the members throw an Error that names what is missing"""
    run_js('scan', 'double', tmp_path, js_expectations)


@needs_node
@pytest.mark.gpu
def test_js_on_hip(tmp_path):
    run_js('scan', 'hip', tmp_path, js_expectations)


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q, lib_path=_abi.HIP_LIB_PATH_RUNTIME)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    check_a_flavour(PrimeField(backend=be), random.Random(q % 65521))
    print(f'runtime scan: modulus {q} ok')
