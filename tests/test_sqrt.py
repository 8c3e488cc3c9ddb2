"""Square roots in the field and compressed curve points on the device: include/gstark_sqrt.h, csrc/sqrt_plan.h, csrc/sqrt.hip,
PrimeField.sqrt / sqrtVectorElements / isSquareVectorElements (genstark_amd/field.py), Curve.liftX / compressMany / decompressMany
(genstark_amd/curve.py), and the same members of js/galois.js and js/curve.js.

Every comparison is against the definition on Python integers: flag == (a == 0 or a^((p-1)/2) == 1); root^2 == a, root < p, root even;
root == 0 where the flag is 0.  CPU tier: the header, the binding table, the host plan on its own under the sanitizers
(tests/host_harness/sqrt_plan_host.cpp), and the whole Python layer on the tests' double (which lacks the entries: the host fallback) — the
96 769 field exhaustively, the 224-bit field on the values that put one non-zero digit into every window.  GPU tier: the whole 17-bit
field in one call; the 224- and 128-bit fields at the seams of a wave, with waves of non-residues next to waves of squares; the other
flavours; the plan each library reports; lifts that feed mulMany and containsMany without a read-back; refused calls; node.
`python tests/test_sqrt.py runtime <q>` is the check of the runtime-modulus flavour (one modulus per process)."""
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
from genstark_amd._abi import MODULUS_17, MODULUS_32, MODULUS_64, MODULUS_128, MODULUS_224, MODULUS_256, Backend, GstarkError
from genstark_amd.curve import B_224, G_224, Curve, curve224
from genstark_amd.field import Matrix, PrimeField, Vector, host_sqrt
from sponge_common import ROOT, check_header_is_plain_c, check_symbol_table, needs_node, run_js
from test_curve import SMALL_B, SMALL_ORDERS, SMALL_POINTS, host_field, p224_double, q17_double      # noqa: F401 (fixtures)

SECP256K1 = 2**256 - 2**32 - 977             # p = 3 (mod 4): s = 1
ED25519 = 2**255 - 19                        # p = 5 (mod 8): s = 2
COMPOSITE = 96769 * 65537
COUNTS = (1, 63, 64, 65, 257, 4097)
SMALL_Y0 = (48282, 58531, 86725)             # the x of the three points with y = 0 on y^2 = x^3 - 3x + 28 over the 96 769 field


def split(p):
    """(s, t, z, g): p - 1 = 2^s * t, the smallest non-residue z >= 2, g = z^t"""
    s = ((p - 1) & -(p - 1)).bit_length() - 1
    z = next(z for z in range(2, 1000) if pow(z, (p - 1) // 2, p) == p - 1)
    return s, (p - 1) >> s, z, pow(z, (p - 1) >> s, p)


def special_values(p):
    """0, 1, 4, p - 1, g (a non-residue with e = 1), g^(2^k) for every k < s (one non-zero digit in each window position), g^(2^s - 2)
    (every digit all ones)"""
    s, _, _, g = split(p)
    return [0, 1, 4, p - 1, g] + [pow(g, 1 << k, p) for k in range(s)] + [pow(g, (1 << s) - 2, p)]


def mixed_values(p, count, rng):
    """the special values in turn, between random squares and random non-residues"""
    special, z = special_values(p), split(p)[2]
    out = []
    for i in range(count):
        r = rng.randrange(1, p)
        out.append(special[(i // 3) % len(special)] if i % 3 == 0 else (r * r % p if i % 3 == 1 else z * r * r % p))
    return out


def is_square(a, p):
    return a == 0 or pow(a, (p - 1) // 2, p) == 1


def check_roots(p, values, roots, flags):
    assert len(values) == len(roots) == len(flags)
    for a, r, f in zip(values, roots, flags):
        assert f == (1 if is_square(a, p) else 0), (a, f)
        if f:
            assert r * r % p == a and r < p and r % 2 == 0, (a, r)
        else:
            assert r == 0, (a, r)


def sliding_products(e):
    """field products of x^e by sliding windows of three bits from the top (csrc/sqrt_plan.h): x^2, x^3, x^5, x^7, every squaring, every
    product but the first"""
    if not e:
        return 0
    bits = bin(e)[2:]
    i, products, first = 0, 4, True
    while i < len(bits):
        if bits[i] == '0':
            products, i = products + 1, i + 1
            continue
        n = min(3, len(bits) - i)
        while bits[i + n - 1] == '0':
            n -= 1
        products += 0 if first else n + 1
        first, i = False, i + n
    return products


def expected_plan(p, chain):
    s, t, _, _ = split(p)
    w = min(8, s)
    n = -(-s // w)
    common = sliding_products((t - 1) // 2) + 2 + n
    if chain and n in (1, 2, 4, 12):
        products = common + (s - w) + n * (n - 1) // 2
    else:
        products = common + sum(s - min((j + 1) * w, s) for j in range(n)) + (n - 1) + max(n - 2, 0)
    return {'twoAdicity': s, 'windowBits': w, 'windows': n, 'productsPerRoot': products}


# ---- CPU tier: header, binding table, plan ----------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    check_header_is_plain_c('sqrt')


def test_symbol_table_matches_the_header():
    others = [getattr(_abi, name) for name in dir(_abi) if name.endswith('_SYMBOLS') and name != 'SQRT_SYMBOLS']
    assert len(others) >= 12
    check_symbol_table('sqrt', _abi.SQRT_SYMBOLS, others)
    header = open(os.path.join(ROOT, 'include', 'gstark_sqrt.h')).read()
    import re
    assert set(re.findall(r'\b(gs_\w+)\(', header)) == set(_abi.SQRT_SYMBOLS)
    assert '2^20' in header and 'modulus is not prime' in header
    assert _abi.CURVE_SYMBOLS == ('gs_curve_mul', 'gs_curve_contains')


def test_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'sqrt_plan_host')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-omit-frame-pointer', os.path.join(ROOT, 'tests', 'host_harness', 'sqrt_plan_host.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'sqrt plan OK' in r.stdout and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_two_adicity_of_the_built_fields():
    for p, s, z in ((MODULUS_128, 32, 3), (MODULUS_64, 30, 3), (MODULUS_32, 25, 3), (MODULUS_17, 9, 11), (MODULUS_256, 32, 3), (MODULUS_224, 96, 11),
                    (ED25519, 2, 2), (SECP256K1, 1, 3)):
        assert split(p)[0] == s and split(p)[2] == z
    assert expected_plan(MODULUS_224, True)['productsPerRoot'] - sliding_products((1 << 127) - 1) == 2 + 88 + 66 + 12


# ---- CPU tier: the Python layer on the host fallback ------------------------------------------------------------------------------------
def test_the_fallback_on_the_whole_small_field(q17_double):
    assert not any(hasattr(q17_double.lib, name) for name in _abi.SQRT_SYMBOLS)
    f = PrimeField(backend=q17_double)
    assert f.twoAdicity == 9 and f.sqrtPlan() is None
    values = list(range(MODULUS_17))
    roots, flags = f.sqrtVectorElements(values)
    assert isinstance(roots, Vector) and isinstance(flags, Vector) and flags.elementSize == 1 and roots.length == flags.length == MODULUS_17
    roots, flags = roots.toValues(), list(flags.toBuffer())
    assert sum(flags) == 48385                                               # 0 and the 48 384 non-zero squares
    check_roots(MODULUS_17, values, roots, flags)
    assert list(f.isSquareVectorElements(f.newVectorFrom(values)).toBuffer()) == flags
    assert f.sqrt(0) == 0 and f.sqrt(4) == 2 and f.sqrt(1) == MODULUS_17 - 1 and f.sqrt(11) is None


def test_the_fallback_on_the_listed_values_of_the_224_bit_field(p224_double):
    p = MODULUS_224
    f = PrimeField(backend=p224_double)
    assert f.twoAdicity == 96
    rng = random.Random(0x5157)
    g = split(p)[3]
    assert not is_square(g, p) and is_square(g * g % p, p)
    values = special_values(p) + [pow(rng.randrange(1, p), 2, p) for _ in range(200)] + [11 * pow(rng.randrange(1, p), 2, p) % p for _ in range(200)]
    assert len(values) == 5 + 96 + 1 + 400
    roots, flags = f.sqrtVectorElements(values)
    roots, flags = roots.toValues(), list(flags.toBuffer())
    check_roots(p, values, roots, flags)
    assert flags[:5] == [1, 1, 1, 1, 0] and flags[5] == 0 and all(flags[6:5 + 96]) and flags[5 + 96] == 1 and all(flags[102:302]) and not any(flags[302:])
    for a, r, ok in zip(values, roots, flags):
        assert f.sqrt(a) == (r if ok else None)
    assert list(f.isSquareVectorElements(values).toBuffer()) == flags
    assert f.sqrtVectorElements([])[0].length == 0 and f.isSquareVectorElements([]).length == 0


def small_curve_points():
    """every affine point of y^2 = x^3 - 3x + 28 over the 96 769 field, from the definition: {x: [ys]}"""
    p = MODULUS_17
    by_square = {}
    for y in range(p):
        by_square.setdefault(y * y % p, []).append(y)
    return {x: sorted(by_square[rhs]) for x in range(p) for rhs in [((x * x - 3) * x + SMALL_B) % p] if rhs in by_square}


def check_small_lifts(curve, even, odd):
    """the lifts of every x of the field by both parities against the definition"""
    p, points = MODULUS_17, small_curve_points()
    assert len(points) == 48601 and sum(len(ys) for ys in points.values()) == 97199 == SMALL_POINTS - 1
    assert sorted(x for x, ys in points.items() if ys == [0]) == list(SMALL_Y0)
    found = set()
    for x in range(p):
        if x not in points:
            assert even[x] is None and odd[x] is None, x
            continue
        assert even[x] is not None and odd[x] is not None, x
        (xe, ye), (xo, yo) = even[x], odd[x]
        assert xe == xo == x and sorted({ye, yo}) == points[x], x
        assert (ye % 2 == 0 and yo % 2 == 1) or (ye == yo == 0 and x in SMALL_Y0), x
        found |= {(x, ye), (x, yo)}
    assert len(found) == 97199 and all(curve.contains(pt) for pt in SMALL_ORDERS)
    return sorted(found)


def test_lifts_of_every_x_of_the_small_field(q17_double):
    curve = Curve(PrimeField(backend=q17_double), -3, SMALL_B)
    assert not curve.liftsOnDevice
    xs = list(range(MODULUS_17))
    even, odd = curve.liftX(xs), curve.liftX(xs, [1] * MODULUS_17)
    affine = check_small_lifts(curve, even, odd)
    cx, cp = curve.compressMany(affine)
    assert cx == [x for x, _ in affine] and cp == [y & 1 for _, y in affine]
    assert curve.decompressMany(cx, cp) == affine
    out, flags = curve.liftX(xs[:300], device=True)                          # the fallback's device=True: the same shapes from host values
    assert isinstance(out, Matrix) and (out.rowCount, out.colCount) == (300, 2) and isinstance(flags, Vector) and flags.elementSize == 1
    assert [tuple(r) if ok else None for r, ok in zip(out.toValues(), flags.toBuffer())] == even[:300]
    vx, vp = curve.compressMany(affine[:300], device=True)
    assert vx.toValues() == cx[:300] and list(vp.toBuffer()) == cp[:300]
    assert curve.decompressMany(vx, vp) == affine[:300]
    host = Curve(host_field(MODULUS_17), -3, SMALL_B)                        # a field without a backend: host integers all the way
    assert host.liftX(xs[:500], [1] * 500) == odd[:500] and host.compressMany(affine[:50]) == (cx[:50], cp[:50])


def test_compressed_points_of_the_224_bit_curve(p224_double):
    curve = curve224(PrimeField(backend=p224_double))
    G = curve.G
    assert curve.compress(G) == (G[0], G[1] & 1) and curve.decompress(G[0], G[1] & 1) == G
    assert curve.decompress(G[0], 1 - (G[1] & 1)) == curve.neg(G)
    p = MODULUS_224
    missing = next(x for x in range(1, 100) if not is_square(((x * x - 3) * x + B_224) % p, p))
    assert curve.decompress(missing, 0) is None and curve.decompress(missing, 1) is None
    assert curve.liftX([G[0], missing], [G[1] & 1, 0]) == [G, None]
    assert curve.liftX([]) == [] and curve.compressMany([]) == ([], [])


def test_a_device_library_without_the_entries_is_an_error(p224_double):
    """no quiet host path where a HIP library lacks only these entries: the double's library under the product backend's name"""
    named = types.SimpleNamespace(name='hip-gfx950', lib=p224_double.lib, element_size=32)
    f = PrimeField(backend=p224_double)
    f.backend = named
    for attempt in (lambda: f.sqrtVectorElements([4]), lambda: f.isSquareVectorElements([4]), f.sqrtPlan):
        with pytest.raises(GstarkError, match=r'no gs_field_sqrt \(include/gstark_sqrt\.h\)'):
            attempt()
    assert f.sqrt(4) == 2                                                    # (host integers by definition: not a device member)
    curve = Curve(types.SimpleNamespace(modulus=MODULUS_224, backend=named, elementSize=32), -3, B_224)
    for attempt in (lambda: curve.liftX([G_224[0]]), lambda: curve.decompressMany([G_224[0]], [0]), lambda: curve.compressMany([G_224])):
        with pytest.raises(GstarkError, match=r'no gs_field_sqrt \(include/gstark_sqrt\.h\)'):
            attempt()
    lib = types.SimpleNamespace(gs_field_sqrt=1, gs_curve_compress=1, gs_field_sqrt_plan=1)     # ... and the other entry is named when it is the one missing
    curve = Curve(types.SimpleNamespace(modulus=MODULUS_224, backend=types.SimpleNamespace(name='hip-gfx950', lib=lib), elementSize=32), -3, B_224)
    with pytest.raises(GstarkError, match=r'no gs_curve_lift_x \(include/gstark_sqrt\.h\)'):
        curve.liftX([G_224[0]])


def test_bad_shapes_raise(p224_double):
    f = PrimeField(backend=p224_double)
    curve = curve224(f)
    G = curve.G
    with pytest.raises(GstarkError, match='canonical'):
        f.sqrtVectorElements([MODULUS_224])
    with pytest.raises(GstarkError, match='canonical'):
        f.isSquareVectorElements([-1])
    with pytest.raises(GstarkError, match='integers'):
        f.sqrtVectorElements([None])
    with pytest.raises(GstarkError, match='1-byte entries'):
        f.sqrtVectorElements(Vector(p224_double, 4, element_size=1))
    big = Vector(p224_double, (1 << 20) + 1, owner=f.newVectorFrom([0])._owner)      # a view that claims 2^20 + 1 elements: refused before anything reads it
    for attempt in (lambda: f.sqrtVectorElements(big), lambda: f.isSquareVectorElements(big), lambda: curve.liftX(big)):
        with pytest.raises(GstarkError, match=r'at most 2\^20'):
            attempt()
    with pytest.raises(GstarkError, match='2 parities and 1 xs'):
        curve.liftX([G[0]], [0, 1])
    with pytest.raises(GstarkError, match='0 parities and 1 xs'):
        curve.decompressMany([G[0]], [])
    with pytest.raises(GstarkError, match='parities are 0 or 1'):
        curve.liftX([G[0]], [2])
    with pytest.raises(GstarkError, match='needs the parities'):
        curve.decompressMany([G[0]], None)
    with pytest.raises(GstarkError, match='canonical'):
        curve.liftX([MODULUS_224])
    with pytest.raises(GstarkError, match='canonical'):
        curve.decompress(-1, 0)
    with pytest.raises(GstarkError, match='bytes'):
        curve.liftX([G[0]], f.newVectorFrom([1]))
    with pytest.raises(GstarkError, match='field elements'):
        curve.liftX(Vector(p224_double, 1, element_size=1))
    with pytest.raises(GstarkError, match='not on the curve'):
        curve.compressMany([(G[0], G[1] + 1)])
    with pytest.raises(GstarkError, match='2 columns'):
        curve.compressMany(f.newMatrixFrom([[1, 2, 3]]))


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------------
def device_roots(f, values):
    roots, flags = f.sqrtVectorElements(values)
    return roots.toValues(), list(flags.toBuffer())


@pytest.fixture(scope='module')
def q17_hip():
    be = Backend(device=0, modulus=MODULUS_17)
    yield be
    be.close()


@pytest.mark.gpu
def test_the_whole_small_field_in_one_call(q17_hip):
    f = PrimeField(backend=q17_hip)
    values = list(range(MODULUS_17))
    vec = f.newVectorFrom(values)
    roots, flags = device_roots(f, vec)                                      # ONE call
    assert sum(flags) == 48385
    check_roots(MODULUS_17, values, roots, flags)
    assert list(f.isSquareVectorElements(vec).toBuffer()) == flags            # ... and one of flags only
    assert f.sqrtPlan() == expected_plan(MODULUS_17, True)


@pytest.mark.gpu
def test_lifts_of_every_x_of_the_small_field_on_the_device(q17_hip):
    f = PrimeField(backend=q17_hip)
    curve = Curve(f, -3, SMALL_B)
    assert curve.liftsOnDevice
    xs = f.newVectorFrom(list(range(MODULUS_17)))
    ones = Vector(q17_hip, MODULUS_17, element_size=1)
    q17_hip.upload(ones.ptr, b'\x01' * MODULUS_17)
    even, odd = curve.liftX(xs), curve.liftX(xs, ones)
    affine = check_small_lifts(curve, even, odd)
    vx, vp = curve.compressMany(affine, device=True)
    assert vx.toValues() == [x for x, _ in affine] and list(vp.toBuffer()) == [y & 1 for _, y in affine]
    assert curve.decompressMany(vx, vp) == affine
    out, flags = curve.liftX(xs, ones, device=True)                          # where there is no point: (0, 0) and flag 0
    assert [tuple(r) if ok else None for r, ok in zip(out.toValues(), flags.toBuffer())] == odd
    assert all(r == [0, 0] for r, ok in zip(out.toValues(), flags.toBuffer()) if not ok)


@pytest.fixture(scope='module', params=['p224', 'p128'])
def seam_field(request):
    be = Backend(device=0, modulus={'p224': MODULUS_224, 'p128': MODULUS_128}[request.param])
    yield PrimeField(backend=be)
    be.close()


@pytest.mark.gpu
def test_seams_of_a_wave(seam_field):
    f, p = seam_field, seam_field.modulus
    assert f.sqrtPlan() == expected_plan(p, True)
    rng = random.Random(p % 65519)
    for count in COUNTS:
        values = mixed_values(p, count, rng)
        roots, flags = device_roots(f, values)
        check_roots(p, values, roots, flags)
        assert list(f.isSquareVectorElements(values).toBuffer()) == flags
    # the same inputs, placed so that one wave holds only non-residues and the next only squares: no result depends on its neighbours
    answer = dict(zip(values, zip(roots, flags)))
    squares, others = [a for a in values if answer[a][1]], [a for a in values if not answer[a][1]]
    assert len(squares) >= 256 and len(others) >= 256
    placed = []
    for k in range(4):
        placed += others[64 * k:64 * k + 64] + squares[64 * k:64 * k + 64]
    roots, flags = device_roots(f, placed)
    assert flags == ([0] * 64 + [1] * 64) * 4
    assert list(zip(roots, flags)) == [answer[a] for a in placed]


@pytest.mark.gpu
@pytest.mark.parametrize('modulus', [MODULUS_256, MODULUS_64, MODULUS_32], ids=['p256', 'q64', 'q32'])
def test_other_flavours(modulus):
    be = Backend(device=0, modulus=modulus)
    try:
        f = PrimeField(backend=be)
        assert f.sqrtPlan() == expected_plan(modulus, True)
        values = mixed_values(modulus, 257, random.Random(modulus % 65521))
        roots, flags = device_roots(f, values)
        check_roots(modulus, values, roots, flags)
        assert list(f.isSquareVectorElements(values).toBuffer()) == flags
    finally:
        be.close()


@pytest.mark.gpu
def test_lifts_feed_the_curve_entries_without_a_read_back():
    be = Backend(device=0, modulus=MODULUS_224)
    try:
        f = PrimeField(backend=be)
        curve = curve224(f)
        assert curve.liftsOnDevice
        made, inf = curve.mulMany(curve.G, list(range(1, 301)), device=True)     # k * G for k = 1 .. 300
        assert not any(inf.toBuffer())
        xs, parities = curve.compressMany(made, device=True)
        lifted, flags = curve.liftX(xs, parities, device=True)
        assert isinstance(lifted, Matrix) and isinstance(flags, Vector)
        assert curve.containsMany(lifted) == [True] * 300 and flags.toBuffer() == b'\x01' * 300
        originals = made.toValues()
        assert lifted.toValues() == originals and originals[0] == list(G_224)
        assert curve.mulMany(lifted, [1] * 300) == [tuple(r) for r in originals]
        flipped = Vector(be, 300, element_size=1)
        be.upload(flipped.ptr, bytes(1 - b for b in parities.toBuffer()))
        assert curve.decompressMany(xs, flipped) == [curve.neg(tuple(r)) for r in originals]
        assert curve.decompress(G_224[0], G_224[1] & 1) == G_224
    finally:
        be.close()


@pytest.mark.gpu
def test_refused_calls_enqueue_nothing(hip_backend):
    f = PrimeField(backend=hip_backend)
    p, es = f.modulus, hip_backend.element_size
    call, ptr = hip_backend.call, lambda v: C.c_void_p(v.ptr)
    values, roots, points = f.newVectorFrom([4, 9, 16]), f.newVectorFrom([7, 7, 7]), f.newMatrixFrom([[7, 7]] * 3)
    flags = Vector(hip_backend, 3, element_size=1)
    hip_backend.upload(flags.ptr, b'\x07\x07\x07')
    a, b = f.le(5), f.le((4 - 1 - 5) % p)                                    # y^2 = x^3 + 5x - 2, through (1, 2)
    over = (1 << 20) + 1
    for name, args in (('gs_field_sqrt', (ptr(values), over, ptr(roots), ptr(flags))), ('gs_curve_lift_x', (a, b, ptr(values), None, over, ptr(points), ptr(flags))),
                       ('gs_curve_compress', (ptr(points), over, ptr(roots), ptr(flags)))):
        with pytest.raises(GstarkError, match=r'at most 2\^20'):
            call(name, *args)
    for name, args in (('gs_field_sqrt', (None, 3, ptr(roots), ptr(flags))), ('gs_field_sqrt', (ptr(values), 3, ptr(roots), None)),
                       ('gs_curve_lift_x', (a, b, None, None, 3, ptr(points), ptr(flags))), ('gs_curve_lift_x', (a, b, ptr(values), None, 3, None, ptr(flags))),
                       ('gs_curve_lift_x', (a, b, ptr(values), None, 3, ptr(points), None)), ('gs_curve_lift_x', (None, b, ptr(values), None, 3, ptr(points), ptr(flags))),
                       ('gs_curve_lift_x', (a, None, ptr(values), None, 3, ptr(points), ptr(flags))), ('gs_curve_compress', (None, 3, ptr(roots), ptr(flags))),
                       ('gs_curve_compress', (ptr(points), 3, None, ptr(flags))), ('gs_curve_compress', (ptr(points), 3, ptr(roots), None))):
        with pytest.raises(GstarkError, match='required'):
            call(name, *args)
    for args in ((b'\xff' * es, b, ptr(values), None, 3, ptr(points), ptr(flags)), (a, f.le(p), ptr(values), None, 3, ptr(points), ptr(flags))):
        with pytest.raises(GstarkError, match='canonical'):
            call('gs_curve_lift_x', *args)
    assert hip_backend.lib.gs_field_sqrt(None, ptr(values), 3, ptr(roots), ptr(flags)) == -1       # GS_ERR_ARG without a context
    call('gs_field_sqrt', None, 0, None, None)                               # count == 0 does nothing
    call('gs_curve_lift_x', a, b, None, None, 0, None, None)
    call('gs_curve_compress', None, 0, None, None)
    assert roots.toValues() == [7, 7, 7] and points.toValues() == [[7, 7]] * 3 and flags.toBuffer() == b'\x07\x07\x07'      # nothing was enqueued
    call('gs_field_sqrt', ptr(values), 3, ptr(roots), ptr(flags))           # ... and valid calls succeed
    assert flags.toBuffer() == b'\x01\x01\x01' and roots.toValues() == [r if r % 2 == 0 else p - r for r in (2, 3, 4)]
    call('gs_curve_lift_x', a, b, ptr(f.newVectorFrom([1, 1, 1])), None, 3, ptr(points), ptr(flags))
    assert points.toValues() == [[1, 2]] * 3 and flags.toBuffer() == b'\x01\x01\x01'


RUNTIME_MODULI = {'s = 1': SECP256K1, 's = 2': ED25519, 's = 96': MODULUS_224}


def run_runtime(q, timeout=300):
    return subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(q)], cwd=ROOT, capture_output=True, text=True, timeout=timeout)


@pytest.mark.gpu
@pytest.mark.parametrize('which', list(RUNTIME_MODULI) + ['ntt-friendly'])
def test_runtime_modulus_flavour(which):
    if which == 'ntt-friendly':
        from test_runtime_modulus import PRIMES
        q = PRIMES[-1]
        assert q.bit_length() == 255 and split(q)[0] >= 32
    else:
        q = RUNTIME_MODULI[which]
    r = run_runtime(q)
    assert r.returncode == 0 and f'runtime sqrt: modulus {q} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
def test_runtime_modulus_flavour_refuses_a_composite():
    r = run_runtime(COMPOSITE)
    assert r.returncode == 0 and f'runtime sqrt: modulus {COMPOSITE} refused: modulus is not prime' in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---- node -------------------------------------------------------------------------------------------------------------------------------
def js_expectations(path):
    """what tests/js_sqrt.js must find, from host integers: 65 roots and 65 lifts in the 224-bit field"""
    p = MODULUS_224
    rng = random.Random(0x5A)
    f = host_field(p)
    c224 = Curve(f, -3, B_224)
    values = mixed_values(p, 65, rng)
    flags = [1 if is_square(a, p) else 0 for a in values]
    roots = [host_sqrt(a, p) for a in values]
    check_roots(p, values, [r or 0 for r in roots], flags)
    xs = [c224._hostMul(G_224, k)[0] for k in range(1, 33)] + [rng.randrange(p) for _ in range(33)]
    parities = [rng.randrange(2) for _ in xs]
    lifted = [c224.decompress(x, b) for x, b in zip(xs, parities)]
    assert all(pt is not None for pt in lifted[:32]) and any(pt is None for pt in lifted)
    text = lambda pt: None if pt is None else [str(pt[0]), str(pt[1])]
    with open(path, 'w') as fh:
        json.dump({'modulus': str(p), 'values': [str(a) for a in values], 'flags': flags, 'roots': [None if r is None else str(r) for r in roots],
                   'xs': [str(x) for x in xs], 'parities': parities, 'lifted': [text(pt) for pt in lifted]}, fh)


@needs_node
def test_js_on_a_library_without_the_entries(tmp_path):
    """the host sqrt equals the Python host; the device members throw an Error that names what is missing"""
    run_js('sqrt', 'double', tmp_path, js_expectations)


@needs_node
@pytest.mark.gpu
def test_js_on_hip(tmp_path):
    run_js('sqrt', 'hip', tmp_path, js_expectations)


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q, lib_path=_abi.HIP_LIB_PATH_RUNTIME)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    f = PrimeField(backend=be)
    if q == COMPOSITE:
        for attempt in (lambda: f.sqrtVectorElements([4]), f.sqrtPlan, lambda: f.isSquareVectorElements([4])):      # the first call and every later one
            try:
                attempt()
            except GstarkError as e:
                assert 'gs_field_sqrt' in str(e) and '(-3)' in str(e) and 'modulus is not prime' in str(e), e
            else:
                raise AssertionError('a composite modulus was not refused')
        print(f'runtime sqrt: modulus {q} refused: modulus is not prime')
    else:
        assert f.sqrtPlan() == expected_plan(q, False)
        values = mixed_values(q, 257, random.Random(q % 65521))
        roots, flags = device_roots(f, values)
        check_roots(q, values, roots, flags)
        assert list(f.isSquareVectorElements(values).toBuffer()) == flags
        if q == MODULUS_224:
            curve = curve224(f)
            made = curve.mulMany(curve.G, list(range(1, 66)))
            cx, cp = curve.compressMany(made)
            assert curve.decompressMany(cx, cp) == made
        print(f'runtime sqrt: modulus {q} ok')
