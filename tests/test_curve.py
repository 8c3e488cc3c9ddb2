"""Scalar multiplications on short Weierstrass curves on the device: include/gstark_curve.h, csrc/curve.hip, genstark_amd/curve.py,
js/curve.js, and the Schnorr / point-multiplication helpers that feed lib224's and pointmul's STARKs.

Every comparison is equality with host integers.  CPU tier: the header, the binding table, and the whole Python layer on the tests' double
(which lacks the entry points: the host fallback) against `ec_multiply` and the reference's known answers.  GPU tier: every special case
of the group law on a curve of 97 200 points over the 96 769 field, where every schedule meets them within a few bits; the 224-bit curve
at the seams of a wave and of a workgroup against digests of the products `ec_multiply` computed once (tests/golden/curve224_products.json,
written by tests/golden/make_curve_products.py: 40 ms a product on Python integers); other flavours; refused calls; device-made keys and signatures
feeding the two STARKs.  `python tests/test_curve.py runtime <q>` is the check of the runtime-modulus flavour (one modulus per process)."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pytest

from genstark_amd import _abi, lib224
from genstark_amd._abi import MODULUS_17, MODULUS_224, Backend, GstarkError
from genstark_amd.curve import (B_224, G_224, ORDER_224, Curve, curve224, schnorr_inputs, schnorr_public_keys, schnorr_sign_many,
                                schnorr_verify_many)
from genstark_amd.field import Matrix, PrimeField, Vector
from genstark_amd.pointmul import ec_multiply, point_mul_air, point_mul_inputs, to_bits
from sponge_common import FLAVOURS, ROOT, check_header_is_plain_c, check_symbol_table, flavour_fixture, needs_node, run_js

P224 = MODULUS_224


# ---- CPU tier: header and binding table -------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    check_header_is_plain_c('curve')


def test_symbol_table_matches_the_header():
    assert _abi.CURVE_SYMBOLS == ('gs_curve_mul', 'gs_curve_contains')
    check_symbol_table('curve', _abi.CURVE_SYMBOLS, (_abi.EXPORTED_SYMBOLS, _abi.OPTIONAL_SYMBOLS, _abi.HADES_SYMBOLS, _abi.RESCUE_SYMBOLS, _abi.TREE_UPDATE_SYMBOLS,
                                                    _abi.TREE_VERIFY_SYMBOLS, _abi.MIMC_SYMBOLS))


@pytest.fixture(scope='module')
def p224_double():
    from test_wide_fields import oracle_for
    be = oracle_for('p224')
    yield be
    be.close()


@pytest.fixture(scope='module')
def q17_double():
    from conftest import _build_oracle
    _build_oracle()
    be = Backend(lib_path=os.path.join(ROOT, 'oracle', 'liboracle_q17.so'), allow_test_double=True)
    yield be
    be.close()


def test_the_double_lacks_the_entries_and_falls_back(p224_double):
    assert not any(hasattr(p224_double.lib, name) for name in _abi.CURVE_SYMBOLS)
    curve = curve224(PrimeField(backend=p224_double))
    assert not curve.onDevice
    assert curve.mul(G_224, 2) == ec_multiply(P224, G_224, 2)
    out, flags = curve.mulMany(G_224, [3, ORDER_224], device=True)           # the fallback's device=True: the same shapes from host values
    assert isinstance(out, Matrix) and isinstance(flags, Vector)
    assert out.toValues() == [list(ec_multiply(P224, G_224, 3)), [0, 0]] and flags.toBuffer() == b'\x00\x01'


def test_a_device_library_without_the_entries_is_an_error(p224_double):
    """no quiet host path where a HIP library lacks only these entries: the double's library under the product backend's name"""
    import types
    field = types.SimpleNamespace(modulus=MODULUS_224, backend=types.SimpleNamespace(name='hip-gfx950', lib=p224_double.lib))
    curve = Curve(field, -3, B_224)
    for attempt in (lambda: curve.mulMany(G_224, [1]), lambda: curve.containsMany([G_224])):
        with pytest.raises(GstarkError, match=r'no gs_curve_mul \(include/gstark_curve\.h\)'):
            attempt()


# ---- CPU tier: the Python layer on the host fallback ------------------------------------------------------------------------------
def test_curve224_constants(p224_double):
    curve = curve224(PrimeField(backend=p224_double))
    gx, gy = curve.G
    assert curve.b == (gy * gy - gx ** 3 - curve.a * gx) % P224 == B_224 and curve.a == P224 - 3
    from test_lib224 import SIG_G
    assert curve.G == tuple(SIG_G) == G_224 and curve.order == ORDER_224 and ORDER_224.bit_length() == 224
    assert curve.contains(curve.G) and curve.contains(None) and not curve.contains((gx, gy ^ 1))
    assert curve.mul(curve.G, curve.order) is None
    assert curve.mul(curve.G, curve.order - 1) == (gx, P224 - gy) == curve.neg(curve.G)


def test_fallback_equals_ec_multiply(p224_double):
    curve = curve224(PrimeField(backend=p224_double))
    rng = random.Random(0x224)
    scalars = [rng.getrandbits(256) for _ in range(20)]
    want = [ec_multiply(P224, G_224, k) for k in scalars]
    assert curve.mulMany(G_224, scalars) == want
    assert curve.mulMany([G_224] * 20, scalars) == want
    assert curve.mulMany(curve.field.newMatrixFrom([list(G_224)]), scalars[:3]) == want[:3]
    assert curve.mulMany(want[:4], scalars[4:8]) == [ec_multiply(P224, pt, k) for pt, k in zip(want[:4], scalars[4:8])]
    assert curve.mulMany(G_224, scalars[:4], bits=100) == [ec_multiply(P224, G_224, k & ((1 << 100) - 1)) for k in scalars[:4]]
    assert curve.mulMany(G_224, [5, 0, 7], addends=[want[0], want[1], None]) == [curve.add(want[0], ec_multiply(P224, G_224, 5)), want[1], ec_multiply(P224, G_224, 7)]
    assert curve.mulMany(G_224, []) == [] and curve.containsMany([]) == []
    assert curve.containsMany([G_224, (G_224[0], G_224[1] + 1), want[3]]) == [True, False, True]


def test_golden_digests_are_ec_multiply(golden):
    """the digests of the smallest counts of every list of tests/golden/curve224_products.json, recomputed with the control"""
    n = ORDER_224
    scalars, multipliers = golden.scalars[:16], golden.multipliers[:16]
    assert scalars[:13] == [0, 1, 2, n - 2, n - 1, n, n + 1, n + 2, 2 * n, 2 * n + 1, 1 << 224, 1 << 255, (1 << 256) - 1] and len(golden.scalars) == 1000
    points = [ec_multiply(P224, G_224, r) for r in multipliers]
    fixed = [ec_multiply(P224, G_224, k) for k in scalars]
    variable = [ec_multiply(P224, pt, k) for pt, k in zip(points, scalars)]
    assert fixed[0] is None and fixed[5] is None and fixed[8] is None and fixed[9] == G_224
    for count in (1, 16):
        for name, values in (('points', points), ('fixed', fixed), ('variable', variable)):
            assert golden.digest(values[:count]) == golden.want[name][str(count)], (name, count)


@pytest.fixture(scope='module')
def golden():
    """the rows (from their seed) and the recorded digests of what ec_multiply gives for them: tests/golden/make_curve_products.py"""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location('make_curve_products', os.path.join(ROOT, 'tests', 'golden', 'make_curve_products.py'))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    with open(os.path.join(ROOT, 'tests', 'golden', 'curve224_products.json')) as fh:
        want = json.load(fh)
    scalars, multipliers = maker.rows(ORDER_224)
    return types.SimpleNamespace(scalars=scalars, multipliers=multipliers, want=want, digest=maker.digest)


def same_as_recorded(golden, name, got, host_rows):
    """got == what ec_multiply gave for the first len(got) rows of list `name`, by digest; on a mismatch the host law names the rows"""
    if golden.digest(got) == golden.want[name][str(len(got))]:
        return True
    host = Curve(host_field(MODULUS_224), -3, B_224)
    wrong = [(k, g) for k, (g, (pt, scalar)) in enumerate(zip(got, host_rows)) if g != host._hostMul(pt, scalar)]
    raise AssertionError((name, len(got), wrong[:3]))


def known_signature():
    from test_lib224 import SIG_H, SIG_P, SIG_R, SIG_S
    return tuple(SIG_P), SIG_H, (tuple(SIG_R), SIG_S)


def test_schnorr_verify_accepts_the_known_signature_and_refuses_changed_ones(p224_double):
    curve = curve224(PrimeField(backend=p224_double))
    P, h, (R, s) = known_signature()
    assert curve.contains(P) and curve.contains(R)
    assert curve.mul(curve.G, s) == curve.add(R, curve.mul(P, h))
    got = schnorr_verify_many(curve, [P] * 4, [h, h ^ 1, h, h], [(R, s), (R, s), (R, s + 1), (curve.neg(R), s)])
    assert got == [True, False, False, False]
    assert schnorr_verify_many(curve, [(P[0], P[1] ^ 1)], [h], [(R, s)]) == [False]      # a key that is no point of the curve
    assert schnorr_verify_many(curve, [], [], []) == []


def test_schnorr_inputs_are_those_of_the_reference(p224_double):
    from test_lib224 import SIG_G, SIG_H, SIG_P, SIG_R, SIG_S
    curve = curve224(PrimeField(backend=p224_double))
    P, h, sig = known_signature()
    raw, assertions = schnorr_inputs(curve, [P], [h], [sig])
    at0 = lambda reg, v: {'step': 0, 'register': reg, 'value': v}
    assert raw == [[SIG_G[0]], [SIG_G[1]], [to_bits(SIG_S)], [SIG_P[0]], [SIG_P[1]], [to_bits(SIG_H)], [SIG_R[0]], [SIG_R[1]]]      # test_lib224.check_schnorr
    assert assertions == [at0(0, SIG_G[0]), at0(1, SIG_G[1]), at0(2, 0), at0(3, 0), at0(7, SIG_P[0]), at0(8, SIG_P[1]), at0(9, SIG_R[0]),
                          at0(10, SIG_R[1]), {'step': 255, 'register': 13, 'value': SIG_H}]
    raw2, assertions2 = schnorr_inputs(curve, [P, P], [h, h], [sig, sig])
    assert all(col == [raw[j][0]] * 2 for j, col in enumerate(raw2))
    assert assertions2 == assertions + [dict(a, step=a['step'] + 256) for a in assertions]
    air = lib224.verify_schnorr_signature_air(curve.field, 2)
    assert len(air.expandInputs(raw2)) == 8 and air.segmentSeeds(raw2) == [[SIG_G[0], SIG_G[1], SIG_P[0], SIG_P[1], SIG_R[0], SIG_R[1]]] * 2


def test_point_mul_inputs_hold_the_known_product(p224_double):
    from test_wide_fields import EC_POINT, EC_PRODUCT, EC_SCALAR
    curve = curve224(PrimeField(backend=p224_double))
    raw, assertions = point_mul_inputs(curve, [EC_POINT], [EC_SCALAR])
    assert raw == [[EC_POINT[0]], [EC_POINT[1]], [to_bits(EC_SCALAR)]]
    assert assertions == [{'step': 255, 'register': 2, 'value': EC_PRODUCT[0]}, {'step': 255, 'register': 3, 'value': EC_PRODUCT[1]}]
    _, two = point_mul_inputs(curve, [EC_POINT, EC_PRODUCT], [EC_SCALAR, 3])
    assert two[:2] == assertions and [a['step'] for a in two[2:]] == [511, 511] and (two[2]['value'], two[3]['value']) == ec_multiply(P224, EC_PRODUCT, 3)
    with pytest.raises(ValueError):
        point_mul_inputs(curve, [EC_POINT], [ORDER_224])


def test_sign_and_verify_round_trip(p224_double):
    curve = curve224(PrimeField(backend=p224_double))
    rng = random.Random(0x5C)
    secrets, nonces, hashes = ([rng.randrange(1, ORDER_224) for _ in range(8)] for _ in range(3))
    publics = schnorr_public_keys(curve, secrets)
    assert publics == [ec_multiply(P224, G_224, x) for x in secrets]
    signatures = schnorr_sign_many(curve, secrets, nonces, hashes)
    assert [R for R, _ in signatures] == [ec_multiply(P224, G_224, k) for k in nonces]
    assert [s for _, s in signatures] == [(k + h * x) % ORDER_224 for k, h, x in zip(nonces, hashes, secrets)]
    assert schnorr_verify_many(curve, publics, hashes, signatures) == [True] * 8
    assert schnorr_verify_many(curve, publics[1:] + publics[:1], hashes, signatures) == [False] * 8


# the curve y^2 = x^3 - 3x + 28 over the 96 769 field: 97 200 = 2^4 * 3^5 * 5^2 points, infinity included
SMALL_B, SMALL_POINTS = 28, 97200
SMALL_ORDERS = {(48282, 0): 2, (58531, 0): 2, (86725, 0): 2, (32774, 27387): 3, (39030, 20046): 4, (8989, 21131): 5, (28061, 6164): 6, (28714, 25592): 8,
                (94989, 63655): 10, (71180, 29588): 12, (12004, 36445): 5400}
OTHER_POINT = (12004, 36445)


def test_small_curve_points_have_the_listed_orders(q17_double):
    curve = Curve(PrimeField(backend=q17_double), -3, SMALL_B)
    assert not curve.onDevice and curve.field.modulus == MODULUS_17
    for point, order in SMALL_ORDERS.items():
        assert curve.contains(point)
        assert curve.mul(point, order) is None and curve.mul(point, SMALL_POINTS) is None, point
        for prime in (2, 3, 5):
            if order % prime == 0:
                assert curve.mul(point, order // prime) is not None, (point, prime)
    assert curve.add((48282, 0), (48282, 0)) is None                         # the doubling of a point with y = 0


def test_bad_shapes_raise(p224_double, oracle_backend):
    curve = curve224(PrimeField(backend=p224_double))
    G = curve.G
    for bad in ([(G[0], G[1] + 1)], [(P224, 0)], [None], [(1, 2, 3)]):
        with pytest.raises(GstarkError):
            curve.mulMany(bad, [1])
    with pytest.raises(GstarkError, match='not on the curve'):
        curve.mulMany(G, [1], addends=[(G[0], G[1] + 1)])
    for bad in (1 << 256, -1):
        with pytest.raises(GstarkError, match='scalar'):
            curve.mulMany(G, [bad])
    with pytest.raises(GstarkError, match='one point for all'):
        curve.mulMany([G, G], [1, 2, 3])
    with pytest.raises(GstarkError, match='addends'):
        curve.mulMany(G, [1, 2], addends=[G])
    for bits in (0, 257):
        with pytest.raises(GstarkError, match='bits'):
            curve.mulMany(G, [1], bits=bits)
    with pytest.raises(GstarkError, match='2 columns'):
        curve.mulMany(curve.field.newMatrixFrom([[1, 2, 3]]), [1])
    with pytest.raises(GstarkError, match='curve224'):
        curve224(PrimeField(backend=oracle_backend))
    with pytest.raises(GstarkError, match='one of each'):
        schnorr_sign_many(curve, [1], [2, 3], [4])
    with pytest.raises(GstarkError, match='base point'):
        schnorr_public_keys(Curve(curve.field, -3, B_224), [1])


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------
def small_scalars(rng):
    return list(range(41)) + [97199, 97200, 97201, 1 << 255, (1 << 256) - 1] + [rng.getrandbits(256) for _ in range(64)]


@pytest.mark.gpu
def test_special_cases_on_the_small_curve():
    """every listed point x every scalar x bits 256, 1, 7, 255 x every kind of addend: 24 launches of 1 210 rows"""
    be = Backend(device=0, modulus=MODULUS_17)
    try:
        curve = Curve(PrimeField(backend=be), -3, SMALL_B)
        assert curve.onDevice
        host = Curve(host_field(MODULUS_17), -3, SMALL_B)
        rng = random.Random(0x17)
        scalars = small_scalars(rng)
        rows = [(pt, k) for pt in SMALL_ORDERS for k in scalars]
        points, ks = [pt for pt, _ in rows], [k for _, k in rows]
        memo = {}

        def product(pt, k):
            if (pt, k) not in memo:
                memo[pt, k] = host._hostMul(pt, k)
            return memo[pt, k]
        seen = set()
        for bits in (256, 1, 7, 255):
            mask = (1 << bits) - 1
            products = [product(pt, k & mask) for pt, k in rows]
            kinds = {'none': None, 'infinity': [None] * len(rows), 'kP': products, '-kP': [host.neg(pt) for pt in products], 'P': points,
                     'other': [OTHER_POINT] * len(rows)}
            for kind, addends in kinds.items():
                want = products if addends is None else [host.add(q, pt) for q, pt in zip(addends, products)]
                got = curve.mulMany(points, ks, addends=addends, bits=bits)
                assert got == want, (bits, kind, [(r, g, w) for r, g, w in zip(rows, got, want) if g != w][:3])
                seen.update(('infinity' if w is None else 'finite', kind) for w in want)
        assert {('infinity', kind) for kind in ('none', 'infinity', 'kP', '-kP', 'P', 'other')} <= seen      # (the test bed does meet them)
    finally:
        be.close()


def host_field(modulus):
    from genstark_amd.hostfield import HostField
    return HostField(modulus)


SEAM_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)      # the seams of a wave (64 lanes, one workgroup of the kernel) and of 256 threads


@pytest.mark.gpu
def test_seams_on_the_224_bit_curve(golden):
    be = Backend(device=0, modulus=MODULUS_224)
    try:
        curve = curve224(PrimeField(backend=be))
        assert curve.onDevice
        scalars = golden.scalars
        points = curve.mulMany(curve.G, golden.multipliers)                  # the random points of the variable-base rows
        assert same_as_recorded(golden, 'points', points, [(curve.G, r) for r in golden.multipliers])
        for count in SEAM_COUNTS:
            assert same_as_recorded(golden, 'variable', curve.mulMany(points[:count], scalars[:count]), list(zip(points, scalars)))
            assert same_as_recorded(golden, 'fixed', curve.mulMany(curve.G, scalars[:count]), [(curve.G, k) for k in scalars])
        for base, name in ((curve.field.newMatrixFrom([list(pt) for pt in points[:257]]), 'variable'), (curve.G, 'fixed')):
            out, flags = curve.mulMany(base, scalars[:257], device=True)
            assert isinstance(out, Matrix) and (out.rowCount, out.colCount) == (257, 2) and isinstance(flags, Vector) and flags.length == 257
            read = [None if inf else tuple(row) for row, inf in zip(out.toValues(), flags.toBuffer())]
            assert golden.digest(read) == golden.want[name]['257']
            assert all(row == [0, 0] for row, inf in zip(out.toValues(), flags.toBuffer()) if inf) and set(flags.toBuffer()) <= {0, 1}
        assert curve.mul(curve.G, curve.order) is None and curve.mul(curve.G, curve.order - 1) == curve.neg(curve.G)
    finally:
        be.close()


def check_random_curve(be, rng, rows=300):
    """a random curve through a random point (b := y^2 - x^3 - a*x), a random and not -3; variable and fixed base, half the rows with an
    addend, against the host law"""
    f = PrimeField(backend=be)
    p = f.modulus
    a = rng.randrange(1, p - 3)
    x, y = rng.randrange(p), rng.randrange(1, p)
    curve, host = Curve(f, a, y * y - x ** 3 - a * x), Curve(host_field(p), a, y * y - x ** 3 - a * x)
    assert curve.onDevice and curve.contains((x, y))
    scalars = [0, 1, 2, (1 << 256) - 1] + [rng.getrandbits(256) for _ in range(rows - 4)]
    points = [host._hostMul((x, y), rng.randrange(1, 1 << 64)) for _ in range(rows)]
    addends = [points[(k + 1) % rows] if k % 2 else None for k in range(rows)]
    assert curve.mulMany(points, scalars, addends=addends) == [host.add(q, host._hostMul(pt, k)) for q, pt, k in zip(addends, points, scalars)]
    assert curve.mulMany((x, y), scalars[:64], bits=200) == [host._hostMul((x, y), k & ((1 << 200) - 1)) for k in scalars[:64]]
    flags = curve.containsMany(points[:10] + [(points[0][0], points[0][1] ^ 1)])
    assert flags == [True] * 10 + [False]


flavour = flavour_fixture('p128', 'q64')


@pytest.mark.gpu
def test_random_curves_in_other_flavours(flavour):
    check_random_curve(flavour, random.Random(flavour.modulus % 65521))


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(MODULUS_224)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'runtime curve: modulus {MODULUS_224} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
def test_contains_many(golden):
    be = Backend(device=0, modulus=MODULUS_224)
    try:
        curve = curve224(PrimeField(backend=be))
        rows = [list(pt) for pt in curve.mulMany(curve.G, golden.multipliers[:257])]
        for k in range(0, 257, 3):                                           # every third row perturbed, in x and in y by turns
            rows[k][(k // 3) % 2] ^= 1
        want = [k % 3 != 0 for k in range(257)]
        assert [curve.contains(tuple(r)) for r in rows] == want              # (host integers agree that the perturbed rows left the curve)
        assert curve.containsMany(curve.field.newMatrixFrom(rows)) == want
        assert curve.containsMany([tuple(r) for r in rows]) == want
    finally:
        be.close()


@pytest.mark.gpu
def test_refused_calls_enqueue_nothing(hip_backend):
    f = PrimeField(backend=hip_backend)
    p = f.modulus
    curve = Curve(f, 5, (4 - 1 - 5) % p)                                     # through (1, 2)
    call, a = hip_backend.call, f.le(curve.a)
    points, out = f.newMatrixFrom([[1, 2]] * 3), f.newMatrixFrom([[7, 7]] * 3)
    ks, flags = Vector(hip_backend, 96, element_size=1), Vector(hip_backend, 3, element_size=1)
    hip_backend.upload(ks.ptr, b''.join(k.to_bytes(32, 'little') for k in (1, 2, 3)))
    hip_backend.upload(flags.ptr, b'\x07\x07\x07')
    ptr = lambda v: C.c_void_p(v.ptr)
    for npoints, bits, count, match in ((1, 256, (1 << 20) + 1, '2\\^20'), (3, 0, 3, 'bits'), (3, 257, 3, 'bits'), (2, 256, 3, 'one for all')):
        with pytest.raises(GstarkError, match=match):
            call('gs_curve_mul', a, ptr(points), npoints, ptr(ks), bits, None, None, count, ptr(out), ptr(flags))
    with pytest.raises(GstarkError, match='required'):
        call('gs_curve_mul', a, None, 3, ptr(ks), 256, None, None, 3, ptr(out), ptr(flags))
    with pytest.raises(GstarkError, match='required'):
        call('gs_curve_mul', None, ptr(points), 3, ptr(ks), 256, None, None, 3, ptr(out), ptr(flags))
    with pytest.raises(GstarkError, match='2\\^20'):
        call('gs_curve_contains', a, f.le(curve.b), ptr(points), (1 << 20) + 1, ptr(flags))
    call('gs_curve_mul', a, ptr(points), 3, ptr(ks), 256, None, None, 0, ptr(out), ptr(flags))          # count 0: a no-op success
    assert out.toValues() == [[7, 7]] * 3 and flags.toBuffer() == b'\x07\x07\x07'                          # nothing was enqueued
    call('gs_curve_mul', a, ptr(points), 3, ptr(ks), 256, None, None, 3, ptr(out), ptr(flags))          # ... and a valid call succeeds
    host = Curve(host_field(p), curve.a, curve.b)
    assert [tuple(r) for r in out.toValues()] == [host._hostMul((1, 2), k) for k in (1, 2, 3)] and flags.toBuffer() == bytes(3)


@pytest.mark.gpu
def test_device_keys_and_signatures_feed_the_starks():
    from genstark_amd._mirror.stark import Stark
    from genstark_amd.errors import StarkError
    small = {'hashAlgorithm': 'sha256', 'extensionFactor': 16, 'exeQueryCount': 20, 'friQueryCount': 12}      # test_lib224's small options
    be = Backend(device=0, modulus=MODULUS_224)
    try:
        f = PrimeField(backend=be)
        curve = curve224(f)
        rng = random.Random(0xFEED)
        secrets, nonces, hashes = ([rng.randrange(1, ORDER_224) for _ in range(4)] for _ in range(3))
        publics = schnorr_public_keys(curve, secrets)
        signatures = schnorr_sign_many(curve, secrets, nonces, hashes)
        assert schnorr_verify_many(curve, publics, hashes, signatures) == [True] * 4
        assert schnorr_verify_many(curve, publics, hashes[1:] + hashes[:1], signatures) == [False] * 4
        air = lib224.verify_schnorr_signature_air(f, 4)
        raw, assertions = schnorr_inputs(curve, publics, hashes, signatures)
        stark = Stark(air, small)
        proof = stark.parse(stark.serialize(stark.prove(assertions, air.expandInputs(raw), air.segmentSeeds(raw))))
        assert stark.verify(assertions, proof)
        with pytest.raises(StarkError):
            stark.verify(assertions[:-1] + [dict(assertions[-1], value=assertions[-1]['value'] ^ 1)], proof)
        air = point_mul_air(f, 4)
        raw, assertions = point_mul_inputs(curve, publics, hashes)
        assert [(assertions[2 * s]['value'], assertions[2 * s + 1]['value']) for s in range(4)] == [ec_multiply(P224, pt, k) for pt, k in zip(publics, hashes)]
        stark = Stark(air, small)
        proof = stark.parse(stark.serialize(stark.prove(assertions, air.expandInputs(raw), air.segmentSeeds(raw))))
        assert stark.verify(assertions, proof)
        with pytest.raises(StarkError):                                      # a flipped product
            stark.verify([dict(assertions[0], value=assertions[0]['value'] ^ 1)] + assertions[1:], proof)
    finally:
        be.close()


# ---- node ---------------------------------------------------------------------------------------------------------------------------
def js_expectations(path):
    """what tests/js_curve.js must find, from host integers: the 224-bit curve (fixed and variable base, an addend, infinity) and the small
    curve's special cases"""
    rng = random.Random(0x15C)
    c224 = Curve(host_field(MODULUS_224), -3, B_224)
    scalars = [0, 1, 2, ORDER_224 - 1, ORDER_224, ORDER_224 + 1, (1 << 256) - 1] + [rng.getrandbits(256) for _ in range(63)]
    points = [c224._hostMul(G_224, rng.randrange(1, ORDER_224)) for _ in scalars]
    addends = [points[(k + 1) % len(points)] if k % 2 else None for k in range(len(points))]
    small = Curve(host_field(MODULUS_17), -3, SMALL_B)
    rows = [(pt, k) for pt in SMALL_ORDERS for k in list(range(13)) + [97199, 97200, 97201]]
    text = lambda pt: None if pt is None else [str(pt[0]), str(pt[1])]
    perturbed = [[pt[0], pt[1] ^ (k % 3 == 0)] for k, pt in enumerate(points)]
    out = {'p224': {'modulus': str(MODULUS_224), 'b': str(B_224), 'G': text(G_224), 'order': str(ORDER_224), 'scalars': [str(k) for k in scalars],
                    'points': [text(pt) for pt in points], 'addends': [text(pt) for pt in addends],
                    'fixed': [text(c224._hostMul(G_224, k)) for k in scalars],
                    'variable': [text(c224.add(q, c224._hostMul(pt, k))) for q, pt, k in zip(addends, points, scalars)],
                    'perturbed': [text(pt) for pt in perturbed], 'contains': [k % 3 != 0 for k in range(len(points))]},
           'q17': {'modulus': str(MODULUS_17), 'b': str(SMALL_B), 'points': [text(pt) for pt, _ in rows], 'scalars': [str(k) for _, k in rows],
                   'products': [text(small._hostMul(pt, k)) for pt, k in rows]}}
    with open(path, 'w') as fh:
        json.dump(out, fh)


@needs_node
def test_js_on_a_library_without_the_entries(tmp_path):
    """the host members equal the Python host; the device members throw an Error that names what is missing"""
    run_js('curve', 'double', tmp_path, js_expectations)


@needs_node
@pytest.mark.gpu
def test_js_on_hip(tmp_path):
    run_js('curve', 'hip', tmp_path, js_expectations)


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q, lib_path=_abi.HIP_LIB_PATH_RUNTIME)     # the modulus of the 224-bit build, given at run time
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    check_random_curve(be, random.Random(q % 65521), rows=200)
    if q == MODULUS_224:
        curve = curve224(PrimeField(backend=be))
        P, h, (R, s) = known_signature()
        assert schnorr_verify_many(curve, [P, P], [h, h ^ 1], [(R, s), (R, s)]) == [True, False]
        assert curve.mul(curve.G, curve.order) is None
    print(f'runtime curve: modulus {q} ok')
