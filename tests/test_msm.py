"""Sums of scalar multiples of curve points on the device: include/gstark_msm.h, csrc/msm_plan.h, csrc/msm.hip, Curve.msm / Curve.sumMany /
schnorr_verify_batch (genstark_amd/curve.py), msm / sumMany of js/curve.js.

Every comparison is equality with host integers.  CPU tier: the header, the binding table, the host plan on its own under the sanitizers
(tests/host_harness/msm_plan_host.cpp), and the whole Python layer on the tests' double (which lacks the entry: the host fallback).  GPU
tier: every window width the plan admits on the curve of 97 200 points over the 96 769 field, where buckets meet equal points, opposite
points, points with y = 0 and infinite partial sums all the time; skewed and cancelling batches; the 224-bit curve at the seams of a wave,
a slice and a workgroup against ONE ec_multiply per count (the points are known multiples of G); device inputs; other flavours; refused
calls; the batch check of Schnorr signatures; node.  `python tests/test_msm.py runtime <q>` is the check of the runtime-modulus flavour
(one modulus per process)."""
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

from genstark_amd import _abi
from genstark_amd._abi import MODULUS_17, MODULUS_224, Backend, GstarkError
from genstark_amd.curve import (B_224, G_224, ORDER_224, Curve, curve224, schnorr_public_keys, schnorr_sign_many, schnorr_verify_batch,
                                schnorr_verify_many)
from genstark_amd.field import Matrix, PrimeField, Vector
from genstark_amd.pointmul import ec_multiply
from sponge_common import ROOT, check_header_is_plain_c, check_symbol_table, flavour_fixture, needs_node, run_js
from test_curve import SMALL_B, SMALL_ORDERS, SMALL_POINTS, golden, host_field, known_signature, p224_double, q17_double      # noqa: F401 (fixtures)

P224 = MODULUS_224
COUNTS = (1, 2, 63, 64, 65, 257, 1000, 4097)
SPECIAL_SCALARS = [0, 1, 97199, 97200, 97201, 1 << 255, (1 << 256) - 1]


def host_sum(host, points, scalars, bits=256, modulo=None):
    """the sum on host integers, term by term; modulo: a multiple of every point's order, to shorten the host's multiplications"""
    mask, total = (1 << bits) - 1, None
    for pt, k in zip(points, scalars):
        if pt is not None:
            total = host.add(total, host._hostMul(pt, (k & mask) % modulo if modulo else k & mask))
    return total


# ---- CPU tier: header, binding table, plan ----------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    check_header_is_plain_c('msm')


def test_symbol_table_matches_the_header():
    assert _abi.MSM_SYMBOLS == ('gs_curve_msm',)
    check_symbol_table('msm', _abi.MSM_SYMBOLS, (_abi.EXPORTED_SYMBOLS, _abi.OPTIONAL_SYMBOLS, _abi.HADES_SYMBOLS, _abi.RESCUE_SYMBOLS, _abi.TREE_UPDATE_SYMBOLS,
                                                _abi.TREE_VERIFY_SYMBOLS, _abi.SPARSE_TREE_SYMBOLS, _abi.MIMC_SYMBOLS, _abi.CURVE_SYMBOLS, _abi.DIAGNOSE_SYMBOLS))
    header = open(os.path.join(ROOT, 'include', 'gstark_msm.h')).read()
    assert '2^20' in header and '512 MiB' in header                          # the caps are part of the contract


def test_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'msm_plan_host')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-omit-frame-pointer', os.path.join(ROOT, 'tests', 'host_harness', 'msm_plan_host.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'combinations ok' in r.stdout and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


# ---- CPU tier: the Python layer on the host fallback ------------------------------------------------------------------------------------
def test_the_double_lacks_the_entry_and_falls_back(p224_double):
    assert not hasattr(p224_double.lib, 'gs_curve_msm')
    curve = curve224(PrimeField(backend=p224_double))
    assert not curve.sumsOnDevice
    rng = random.Random(0x35)
    multipliers = [rng.randrange(1, ORDER_224) for _ in range(20)]
    points = [ec_multiply(P224, G_224, r) for r in multipliers]
    scalars = [0, 1, ORDER_224, (1 << 256) - 1] + [rng.getrandbits(256) for _ in range(16)]
    want = ec_multiply(P224, G_224, sum(k * r for k, r in zip(scalars, multipliers)) % ORDER_224)
    assert curve.msm(points, scalars) == want
    assert curve.msm(points, scalars, window=5) == want                      # (the fallback has no windows: the same sum)
    holes = [None if k % 3 == 0 else pt for k, pt in enumerate(points)]
    assert curve.msm(holes, scalars) == ec_multiply(P224, G_224, sum(k * r for j, (k, r) in enumerate(zip(scalars, multipliers)) if j % 3) % ORDER_224)
    assert curve.msm(points[:5], scalars[:5], bits=100) == host_sum(curve, points[:5], scalars[:5], bits=100)
    assert curve.msm(curve.field.newMatrixFrom([list(pt) for pt in points[:4]]), scalars[:4]) == host_sum(curve, points[:4], scalars[:4])
    assert curve.msm(points[:4], curve.field.newVectorFrom(multipliers[:4])) == host_sum(curve, points[:4], multipliers[:4])
    assert curve.msm([], []) is None and curve.msm([None], [5]) is None and curve.msm(points[:1], [0]) is None and curve.msm([G_224, curve.neg(G_224)], [7, 7]) is None
    assert curve.sumMany(points) == ec_multiply(P224, G_224, sum(multipliers) % ORDER_224) and curve.sumMany([]) is None and curve.sumMany([None, G_224]) == G_224
    for got, value in ((curve.msm(points, scalars, device=True), want), (curve.msm(points[:1], [ORDER_224], device=True), None), (curve.sumMany(points[:2], device=True), curve.add(points[0], points[1]))):
        out, flag = got                                                      # the fallback's device=True: the same shapes from host values
        assert isinstance(out, Matrix) and (out.rowCount, out.colCount) == (1, 2) and isinstance(flag, Vector) and flag.length == 1
        assert out.toValues() == [list(value or (0, 0))] and flag.toBuffer() == bytes([value is None])


def test_the_fallback_on_the_small_curve(q17_double):
    curve = Curve(PrimeField(backend=q17_double), -3, SMALL_B)
    assert not curve.sumsOnDevice
    host = Curve(host_field(MODULUS_17), -3, SMALL_B)
    rng = random.Random(0x300)
    bases = list(SMALL_ORDERS)
    points = [host._hostMul(bases[k % len(bases)], 1 + rng.randrange(SMALL_ORDERS[bases[k % len(bases)]] - 1)) for k in range(300)]
    scalars = SPECIAL_SCALARS + [rng.getrandbits(256) for _ in range(300 - len(SPECIAL_SCALARS))]
    want = host_sum(host, points, scalars, modulo=SMALL_POINTS)
    assert curve.msm(points, scalars) == want == host.msm(points, [k % SMALL_POINTS for k in scalars]) and want is not None
    assert curve.sumMany(points) == host_sum(host, points, [1] * 300)
    assert host.msm(points, scalars, bits=7) == host_sum(host, points, scalars, bits=7)


def test_a_device_library_without_the_entry_is_an_error(p224_double):
    """no quiet host path where a HIP library lacks only this entry: the double's library under the product backend's name"""
    import types
    field = types.SimpleNamespace(modulus=MODULUS_224, backend=types.SimpleNamespace(name='hip-gfx950', lib=p224_double.lib))
    curve = Curve(field, -3, B_224)
    for attempt in (lambda: curve.msm([G_224], [1]), lambda: curve.sumMany([G_224])):
        with pytest.raises(GstarkError, match=r'no gs_curve_msm \(include/gstark_msm\.h\)'):
            attempt()


def test_bad_shapes_raise(p224_double):
    curve = curve224(PrimeField(backend=p224_double))
    G = curve.G
    with pytest.raises(GstarkError, match='2 points and 3 scalars'):
        curve.msm([G, G], [1, 2, 3])
    with pytest.raises(GstarkError, match='1 points and 2 scalars'):
        curve.msm(curve.field.newMatrixFrom([list(G)]), [1, 2])
    for bad in (1 << 256, -1):
        with pytest.raises(GstarkError, match='scalar'):
            curve.msm([G], [bad])
    for bits in (0, 257):
        with pytest.raises(GstarkError, match='bits'):
            curve.msm([G], [1], bits=bits)
    for window in (17, -1):
        with pytest.raises(GstarkError, match='window'):
            curve.msm([G], [1], window=window)
    with pytest.raises(GstarkError, match='not on the curve'):
        curve.msm([(G[0], G[1] + 1)], [1])
    with pytest.raises(GstarkError, match='not on the curve'):
        curve.sumMany([G, (G[0], G[1] + 1)])
    with pytest.raises(GstarkError, match='2 columns'):
        curve.msm(curve.field.newMatrixFrom([[1, 2, 3]]), [1])
    sig = known_signature()
    with pytest.raises(GstarkError, match=r'2\^19 - 1 signatures'):
        schnorr_verify_batch(curve, [sig[0]] * (1 << 19), [sig[1]] * (1 << 19), [sig[2]] * (1 << 19))
    with pytest.raises(GstarkError, match='base point'):
        schnorr_verify_batch(Curve(curve.field, -3, B_224), [sig[0]], [sig[1]], [sig[2]])
    with pytest.raises(GstarkError, match='one of each'):
        schnorr_verify_batch(curve, [sig[0]], [sig[1], sig[1]], [sig[2]])


def corrupted_batches(curve, publics, hashes, signatures):
    """(name, publics, hashes, signatures, expected answer): the valid batch, one s off by one, two keys swapped, one R off the curve"""
    (R1, s1), (R2, _) = signatures[1], signatures[2]
    return (('valid', publics, hashes, signatures, True),
            ('s off by one', publics, hashes, signatures[:1] + [(R1, (s1 + 1) % curve.order)] + signatures[2:], False),
            ('swapped key', [publics[1], publics[0]] + publics[2:], hashes, signatures, False),
            ('R off the curve', publics, hashes, signatures[:2] + [((R2[0], R2[1] ^ 1), signatures[2][1])] + signatures[3:], False))


def check_batches(curve, count, rng):
    secrets, nonces, hashes = ([rng.randrange(1, ORDER_224) for _ in range(count)] for _ in range(3))
    publics = schnorr_public_keys(curve, secrets)
    signatures = schnorr_sign_many(curve, secrets, nonces, hashes)
    for name, keys, hs, sigs, want in corrupted_batches(curve, publics, hashes, signatures):
        assert schnorr_verify_batch(curve, keys, hs, sigs, rng=rng) is want, name
        assert schnorr_verify_batch(curve, keys, hs, sigs) is want, name     # (the `secrets` module draws the z)
        assert all(schnorr_verify_many(curve, keys, hs, sigs)) is want, name
    assert schnorr_verify_batch(curve, [], [], []) is True


def test_batch_check_on_the_fallback(p224_double):
    check_batches(curve224(PrimeField(backend=p224_double)), 3, random.Random(0xBA7C))


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------
def small_terms(rng, count):
    """multiples of every point of SMALL_ORDERS (none infinite) by turns, and scalars: the special ones first"""
    host = Curve(host_field(MODULUS_17), -3, SMALL_B)
    bases = list(SMALL_ORDERS)
    points = [host._hostMul(bases[k % len(bases)], 1 + rng.randrange(SMALL_ORDERS[bases[k % len(bases)]] - 1)) for k in range(count)]
    scalars = (SPECIAL_SCALARS + [rng.getrandbits(256) for _ in range(count)])[:count]
    return host, points, scalars


def prefix_sums(host, points, scalars, bits):
    """want[count] for every count: the running sum of the terms on host integers (scalars reduced mod the group order: exact, every
    point's order divides it)"""
    mask, total, sums = (1 << bits) - 1, None, [None]
    for pt, k in zip(points, scalars):
        total = host.add(total, host._hostMul(pt, (k & mask) % SMALL_POINTS))
        sums.append(total)
    return sums


@pytest.mark.gpu
def test_every_window_width_on_the_small_curve():
    be = Backend(device=0, modulus=MODULUS_17)
    try:
        f = PrimeField(backend=be)
        curve = Curve(f, -3, SMALL_B)
        assert curve.sumsOnDevice
        host, points, scalars = small_terms(random.Random(0x1717), max(COUNTS))
        want = {bits: prefix_sums(host, points, scalars, bits) for bits in (256, 1, 7, 255)}
        seen = set()
        for count in COUNTS:
            src = f.newMatrixFrom([list(pt) for pt in points[:count]])
            for window in range(17):                                         # 0: the plan's choice.  4 097 terms x 256 windows stay far below the workspace cap: every width is admitted
                got = curve.msm(src, scalars[:count], window=window)
                assert got == want[256][count], (count, window, got, want[256][count])
                seen.add(got is None)
            if count == 1000:
                for bits in (1, 7, 255):
                    for window in (0, 1, 3, 8, 16):
                        got = curve.msm(src, scalars[:count], bits=bits, window=window)
                        assert got == want[bits][count], (count, bits, window, got, want[bits][count])
        assert seen == {True, False}                                         # (count 1 has the scalar 0: infinity)
    finally:
        be.close()


@pytest.mark.gpu
def test_skew_and_cancellation_on_the_small_curve():
    be = Backend(device=0, modulus=MODULUS_17)
    try:
        curve = Curve(PrimeField(backend=be), -3, SMALL_B)
        rng = random.Random(0x5CE3)
        host, points, scalars = small_terms(rng, 4097)
        k = rng.getrandbits(256) | 1
        everything = host_sum(host, points, [1] * 4097)
        pairs = [pt if j % 2 == 0 else host.neg(pt) for pt in points[:2048] for j in (0, 1)]
        top = [rng.randrange(1, 1 << 4) << 252 for _ in range(4097)]
        cases = {'equal scalars': (points, [k] * 4097, host._hostMul(everything, k % SMALL_POINTS)),
                 'zero scalars': (points, [0] * 4097, None),
                 'equal points': ([points[10]] * 4097, scalars, host._hostMul(points[10], sum(scalars) % SMALL_POINTS)),
                 'opposite pairs': (pairs, [s for s in scalars[:2048] for _ in (0, 1)], None),
                 'top window only': (points, top, host_sum(host, points, top, modulo=SMALL_POINTS))}
        for name, (pts, ks, want) in cases.items():
            for window in (0, 4, 13):
                for _ in range(2):                                           # twice in a row: the same answer whatever order the atomics gave
                    assert curve.msm(pts, ks, window=window) == want, (name, window)
        assert curve.sumMany(points) == everything and curve.sumMany(pairs) is None
    finally:
        be.close()


SEAM_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)


@pytest.mark.gpu
def test_seams_on_the_224_bit_curve(golden):
    be = Backend(device=0, modulus=MODULUS_224)
    try:
        f = PrimeField(backend=be)
        curve = curve224(f)
        assert curve.sumsOnDevice
        n, scalars, multipliers = ORDER_224, golden.scalars, golden.multipliers
        points = curve.mulMany(curve.G, multipliers)
        assert golden.digest(points) == golden.want['points'][str(len(points))]
        for count in SEAM_COUNTS:
            want = ec_multiply(P224, G_224, sum(k * r for k, r in zip(scalars[:count], multipliers[:count])) % n)
            for window in (0, 1, 7, 16):
                assert curve.msm(points[:count], scalars[:count], window=window) == want, (count, window)
        # 2^14 + 1 points made on the device: the plan's own choice cuts its buckets into several slices and combines them over levels
        rng = random.Random(0x4001)
        count = (1 << 14) + 1
        rs, ks = [rng.randrange(1, n) for _ in range(count)], [rng.getrandbits(256) for _ in range(count)]
        made, flags = curve.mulMany(curve.G, rs, device=True)
        assert not any(flags.toBuffer())
        want = ec_multiply(P224, G_224, sum(k * r for k, r in zip(ks, rs)) % n)
        assert curve.msm(made, ks) == want
        assert curve.msm(made, [ks[0]] * count) == ec_multiply(P224, G_224, ks[0] * sum(rs) % n)      # every term in one bucket per window
        assert curve.sumMany(made) == ec_multiply(P224, G_224, sum(rs) % n)
    finally:
        be.close()


def check_device_inputs(be, rng, rows=300):
    """a random curve through a random point; points as a Matrix, scalars as a Vector of field elements, results left on the device"""
    f = PrimeField(backend=be)
    p = f.modulus
    a = rng.randrange(1, p - 3)
    x, y = rng.randrange(p), rng.randrange(1, p)
    curve, host = Curve(f, a, y * y - x ** 3 - a * x), Curve(host_field(p), a, y * y - x ** 3 - a * x)
    assert curve.sumsOnDevice
    points = [host._hostMul((x, y), rng.randrange(1, 1 << 64)) for _ in range(rows)]
    elements = [0, 1, p - 1] + [rng.randrange(p) for _ in range(rows - 3)]
    bits = 8 * be.element_size if be.element_size == 16 else 256
    want = host_sum(host, points, elements)
    matrix, vector = f.newMatrixFrom([list(pt) for pt in points]), f.newVectorFrom(elements)
    assert vector.elementSize == be.element_size
    assert curve.msm(points, elements) == want
    for pts in (matrix, points):
        assert curve.msm(pts, vector, bits=bits) == want
        out, flag = curve.msm(pts, vector, bits=bits, device=True)
        assert isinstance(out, Matrix) and (out.rowCount, out.colCount) == (1, 2) and isinstance(flag, Vector) and flag.length == 1 and flag.elementSize == 1
        assert out.toValues() == [list(want)] and flag.toBuffer() == b'\x00'
    assert curve.msm(matrix, vector, bits=64, window=6) == host_sum(host, points, elements, bits=64)
    assert curve.sumMany(matrix) == curve.msm(matrix, [1] * rows) == host_sum(host, points, [1] * rows)
    out, flag = curve.msm([points[0], host.neg(points[0])], f.newVectorFrom([5, 5]), bits=bits, device=True)
    assert out.toValues() == [[0, 0]] and flag.toBuffer() == b'\x01'
    out, flag = curve.msm([], [], device=True)                               # the empty sum
    assert out.toValues() == [[0, 0]] and flag.toBuffer() == b'\x01'
    if be.element_size == 16:
        with pytest.raises(GstarkError, match='bits'):
            curve.msm(matrix, vector, bits=129)
    return curve, host, points, (x, y)


device_flavour = flavour_fixture('p128', 'p224')


@pytest.mark.gpu
def test_device_inputs(device_flavour):
    check_device_inputs(device_flavour, random.Random(device_flavour.modulus % 65519))


def check_random_curve(be, rng, rows=300):
    curve, host, points, base = check_device_inputs(be, rng, rows)
    scalars = [0, 1, 2, (1 << 256) - 1] + [rng.getrandbits(256) for _ in range(rows - 4)]
    for window in (0, 2, 11):
        assert curve.msm(points, scalars, window=window) == host_sum(host, points, scalars), window
    assert curve.msm(points[:65], scalars[:65], bits=200) == host_sum(host, points[:65], scalars[:65], bits=200)
    if be.element_size == 16:
        # 2^15 + 1 terms: where the plan's own choice for 16-byte elements is multiply_then_sum (csrc/msm_plan.h), more than one launch of
        # its sum.  The points are known multiples of `base`, made on the device: ONE host multiplication is the reference
        count = (1 << 15) + 1
        rs, ks = [rng.randrange(1, 1 << 64) for _ in range(count)], [0, 1] + [rng.getrandbits(128) % be.modulus for _ in range(count - 2)]
        made, flags = curve.mulMany(base, rs, device=True)
        assert not any(flags.toBuffer())
        want = host._hostMul(base, sum(k * r for k, r in zip(ks, rs)))
        assert curve.msm(made, ks) == want                                   # 32-byte scalars
        assert curve.msm(made, curve.field.newVectorFrom(ks), bits=128) == want      # a column of elements: 16-byte scalars, widened in workspace
        assert curve.msm(made, ks, window=9) == want                         # ... and the bucket route agrees
        assert curve.sumMany(made) == host._hostMul(base, sum(rs))


flavour = flavour_fixture('p128', 'q64')


@pytest.mark.gpu
def test_random_curves_in_other_flavours(flavour):
    check_random_curve(flavour, random.Random(flavour.modulus % 65521))


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(MODULUS_224)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'runtime msm: modulus {MODULUS_224} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
def test_refused_calls_enqueue_nothing(hip_backend):
    f = PrimeField(backend=hip_backend)
    p = f.modulus
    curve = Curve(f, 5, (4 - 1 - 5) % p)                                     # through (1, 2)
    call, a = hip_backend.call, f.le(curve.a)
    points, out = f.newMatrixFrom([[1, 2]] * 3), f.newMatrixFrom([[7, 7]])
    ks, flag = Vector(hip_backend, 96, element_size=1), Vector(hip_backend, 1, element_size=1)
    hip_backend.upload(ks.ptr, b''.join(k.to_bytes(32, 'little') for k in (1, 2, 3)))
    hip_backend.upload(flag.ptr, b'\x07')
    ptr = lambda v: C.c_void_p(v.ptr)
    for stride, bits, count, window, match in ((32, 256, (1 << 20) + 1, 0, 'count: at most'), (8, 64, 3, 0, 'scalar_stride: 16 or 32'), (64, 256, 3, 0, 'scalar_stride: 16 or 32'), (32, 0, 3, 0, 'bits: outside'),
                                               (32, 257, 3, 0, 'bits: outside'), (16, 129, 3, 0, 'bits: above 128'), (32, 256, 3, 17, 'window: outside'), (32, 256, 1 << 20, 1, 'window: the workspace.*cap')):
        with pytest.raises(GstarkError, match=match):
            call('gs_curve_msm', a, ptr(points), ptr(ks), stride, bits, count, window, ptr(out), ptr(flag))
    for args in ((None, ptr(points), ptr(ks), 32, 256, 3, 0, ptr(out), ptr(flag)), (a, None, ptr(ks), 32, 256, 3, 0, ptr(out), ptr(flag)),
                 (a, ptr(points), None, 32, 256, 3, 0, ptr(out), ptr(flag)), (a, ptr(points), ptr(ks), 32, 256, 3, 0, None, ptr(flag)),
                 (a, ptr(points), ptr(ks), 32, 256, 3, 0, ptr(out), None), (a, None, None, 32, 256, 0, 0, None, ptr(flag))):
        with pytest.raises(GstarkError, match='required'):
            call('gs_curve_msm', *args)
    with pytest.raises(GstarkError, match='canonical'):
        call('gs_curve_msm', b'\xff' * hip_backend.element_size, ptr(points), ptr(ks), 32, 256, 3, 0, ptr(out), ptr(flag))
    assert out.toValues() == [[7, 7]] and flag.toBuffer() == b'\x07'          # nothing was enqueued
    host = Curve(host_field(p), curve.a, curve.b)
    call('gs_curve_msm', a, ptr(points), ptr(ks), 32, 256, 3, 0, ptr(out), ptr(flag))      # ... and a valid call succeeds
    assert tuple(out.toValues()[0]) == host._hostMul((1, 2), 6) and flag.toBuffer() == b'\x00'
    call('gs_curve_msm', a, None, None, 32, 256, 0, 0, ptr(out), ptr(flag))               # the empty sum writes infinity
    assert out.toValues() == [[0, 0]] and flag.toBuffer() == b'\x01'


@pytest.mark.gpu
def test_batch_check_of_schnorr_signatures():
    be = Backend(device=0, modulus=MODULUS_224)
    try:
        curve = curve224(PrimeField(backend=be))
        assert curve.sumsOnDevice
        check_batches(curve, 64, random.Random(0xBA7C64))
    finally:
        be.close()


# ---- node -------------------------------------------------------------------------------------------------------------------------------
def js_expectations(path):
    """what tests/js_msm.js must find, from host integers: sums on the 224-bit curve (with infinite points among the terms, by bits, of
    no term) and on the small curve under forced windows"""
    rng = random.Random(0x15D)
    c224 = Curve(host_field(MODULUS_224), -3, B_224)
    multipliers = [rng.randrange(1, ORDER_224) for _ in range(70)]
    scalars = [0, 1, 2, ORDER_224 - 1, ORDER_224, ORDER_224 + 1, (1 << 256) - 1] + [rng.getrandbits(256) for _ in range(63)]
    points = [c224._hostMul(G_224, r) for r in multipliers]
    holes = [None if k % 5 == 0 else pt for k, pt in enumerate(points)]
    small, spoints, sscalars = small_terms(rng, 300)
    text = lambda pt: None if pt is None else [str(pt[0]), str(pt[1])]
    lincomb = lambda pairs: ec_multiply(P224, G_224, sum(k * r for k, r in pairs) % ORDER_224)
    out = {'p224': {'modulus': str(MODULUS_224), 'scalars': [str(k) for k in scalars], 'points': [text(pt) for pt in points], 'holes': [text(pt) for pt in holes],
                    'sum': text(lincomb(zip(scalars, multipliers))), 'sum_holes': text(lincomb((k, r) for j, (k, r) in enumerate(zip(scalars, multipliers)) if j % 5)),
                    'sum_100_bits': text(lincomb((k & ((1 << 100) - 1), r) for k, r in zip(scalars, multipliers))), 'sum_points': text(lincomb((1, r) for r in multipliers))},
           'q17': {'modulus': str(MODULUS_17), 'b': str(SMALL_B), 'points': [text(pt) for pt in spoints], 'scalars': [str(k) for k in sscalars],
                   'sum': text(host_sum(small, spoints, sscalars, modulo=SMALL_POINTS)), 'sum_points': text(host_sum(small, spoints, [1] * 300))}}
    with open(path, 'w') as fh:
        json.dump(out, fh)


@needs_node
def test_js_on_a_library_without_the_entry(tmp_path):
    """msm and sumMany throw an Error that names what is missing"""
    run_js('msm', 'double', tmp_path, js_expectations)


@needs_node
@pytest.mark.gpu
def test_js_on_hip(tmp_path):
    run_js('msm', 'hip', tmp_path, js_expectations)


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q, lib_path=_abi.HIP_LIB_PATH_RUNTIME)     # the modulus of the 224-bit build, given at run time
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    check_random_curve(be, random.Random(q % 65521), rows=200)
    if q == MODULUS_224:
        curve = curve224(PrimeField(backend=be))
        P, h, (R, s) = known_signature()
        assert schnorr_verify_batch(curve, [P, P], [h, h], [(R, s), (R, s)]) is True and schnorr_verify_batch(curve, [P, P], [h, h ^ 1], [(R, s), (R, s)]) is False
    print(f'runtime msm: modulus {q} ok')
