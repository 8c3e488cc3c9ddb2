"""gs_eval_polys_at_points (include/gstark_boundary.h): many polynomials at many arbitrary points, against Horner on Python integers.

Every comparison is exact.  The lengths walk every seam of the kernel: the 256 threads of a workgroup, one segment (S coefficients, asked
of the library) and two; the points include 0 and 1; the rows lie in a stride longer than any of them with non-zero values beyond their
lengths that must not reach a result.  `python tests/test_eval_polys_at_points.py runtime <q>` is the same check for the runtime-modulus
flavour (one modulus per process)."""
import ctypes as C
import os
import random
import sys

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pytest

from genstark_amd import _abi
from genstark_amd._abi import Backend
from genstark_amd.field import PrimeField

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def horner(coef, x, p):
    acc = 0
    for c in reversed(coef):
        acc = (acc * x + c) % p
    return acc


def eval_rows(be, f, rows, lens, stride, xs):
    """rows: `stride` integers each (whatever lies beyond lens[r] included) -> [[p_r(x) for x in xs] for r] from the entry point"""
    es = f.elementSize
    polys = be.alloc(max(len(rows) * stride, 1) * es)
    be.upload(polys, b''.join(f.le(c) for row in rows for c in row) or bytes(es))
    out = be.alloc(len(rows) * len(xs) * es)
    be.call('gs_eval_polys_at_points', C.c_void_p(polys), len(rows), stride, (C.c_uint64 * len(rows))(*lens), b''.join(f.le(x) for x in xs), len(xs), C.c_void_p(out))
    raw = be.download(out, len(rows) * len(xs) * es)
    be.free(polys), be.free(out)
    return [[int.from_bytes(raw[(r * len(xs) + k) * es:(r * len(xs) + k + 1) * es], 'little') for k in range(len(xs))] for r in range(len(rows))]


def check_entry_point(be, rng):
    f = PrimeField(backend=be)
    p = f.modulus
    S = be.lib.gs_eval_polys_at_points_segment()
    assert S >= 512 and S % 256 == 0
    nz = lambda: rng.randrange(1, p)                  # non-zero: a coefficient read from beyond a row's length changes the value
    cases = [((0, 1, 257), 300, [rng.randrange(p)]),                                                            # no coefficients, one, npoints = 1
             ((255, 256, 513, S - 1, S, 2 * S + 1, 257, S + 1, 2 * S - 1, 2 * S), 2 * S + 9, [0, 1, nz(), p - 1, nz()]),
             ((3, 300, 0), 301, [nz() for _ in range(129)])]                                                      # no multiple of the point block
    for lens, stride, xs in cases:
        rows = [[nz() for _ in range(stride)] for _ in lens]
        got = eval_rows(be, f, rows, lens, stride, xs)
        for r, n in enumerate(lens):
            assert got[r] == [horner(rows[r][:n], x, p) for x in xs], (lens, n)
        if 0 in xs:
            assert all(got[r][xs.index(0)] == (rows[r][0] if n else 0) for r, n in enumerate(lens))
    # stride == len, one row, one point: nothing but the row is there to be read
    row = [nz() for _ in range(S + 7)]
    assert eval_rows(be, f, [row], [S + 7], S + 7, [5 % p]) == [[horner(row, 5 % p, p)]]
    with pytest.raises(_abi.GstarkError):
        eval_rows(be, f, [row], [S + 8], S + 7, [1])   # a length beyond the stride is refused


@pytest.mark.gpu
@pytest.mark.parametrize('modulus', [None, _abi.MODULUS_64, _abi.MODULUS_17, _abi.MODULUS_224], ids=['p128', 'q64', 'q17', 'p224'])
def test_against_integers(modulus):
    be = Backend(device=0, modulus=modulus)
    try:
        check_entry_point(be, random.Random(0xE7A1))
    finally:
        be.close()


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    import subprocess
    from test_runtime_modulus import PRIMES
    q = PRIMES[6]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(q)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'runtime eval_polys_at_points: modulus {q} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
def test_agrees_with_eval_poly_at(hip_backend):
    """2^14 coefficients at 68 points: gs_eval_poly_at, one call per point, gives the same elements"""
    f = PrimeField(backend=hip_backend)
    rng = random.Random(68)
    poly = f.newVectorFrom([rng.randrange(f.modulus) for _ in range(1 << 14)])
    xs = [rng.randrange(f.modulus) for _ in range(68)]
    got = f.evalPolysAtPoints([poly], xs).toValues()
    assert got == [[f.evalPolyAt(poly, x) for x in xs]]


@pytest.mark.gpu
def test_python_surface(hip_backend):
    """PrimeField.evalPolysAtPoints: a Matrix and a list of vectors of different lengths; equal to evalPolyAt per polynomial and point,
    also on a library without the entry point (the fallback)"""
    f = PrimeField(backend=hip_backend)
    rng = random.Random(7)
    p = f.modulus
    values = [[rng.randrange(p) for _ in range(700)] for _ in range(3)]
    m = f.newMatrixFrom(values)
    xs = [0, 1, p + 5, rng.randrange(p), rng.randrange(p)]
    want = [[f.evalPolyAt(m.row(r), x % p) for x in xs] for r in range(3)]
    assert f.evalPolysAtPoints(m, xs).toValues() == want == [[horner(v, x % p, p) for x in xs] for v in values]
    vecs = [f.newVectorFrom(values[0][:1]), f.newVectorFrom(values[1][:258]), f.newVectorFrom(values[2])]
    assert f.evalPolysAtPoints(vecs, xs).toValues() == [[f.evalPolyAt(v, x % p) for x in xs] for v in vecs]

    class _Without:            # the same library seen without the optional entry point
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name == 'gs_eval_polys_at_points':
                raise AttributeError(name)
            return getattr(self._lib, name)
    lib = hip_backend.lib
    hip_backend.lib = _Without(lib)
    try:
        assert f.evalPolysAtPoints(m, xs).toValues() == want
    finally:
        hip_backend.lib = lib


def test_the_entry_point_is_optional_and_declared():
    """bound like gs_boundary_polys: not one of the mandatory symbols, declared in include/gstark_boundary.h"""
    assert 'gs_eval_polys_at_points' in _abi.OPTIONAL_SYMBOLS and 'gs_eval_polys_at_points' not in _abi.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, 'include', 'gstark_boundary.h')).read()
    assert 'gs_eval_polys_at_points(' in header and 'gs_eval_polys_at_points_segment(' in header


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    check_entry_point(be, random.Random(q % 65521))
    print(f'runtime eval_polys_at_points: modulus {q} ok')
