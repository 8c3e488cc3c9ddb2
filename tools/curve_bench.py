"""tools/curve_bench.py [--out profiles/curve.md] — scalar multiplications on the MI355X (include/gstark_curve.h), written as a profile.

  multiplications/s  the 224-bit curve of pointmul.aa / lib224.aa, 256-bit scalars, 2^12, 2^16 and 2^20 multiplications per launch,
                     variable base (one point per row) and fixed base (G for all); the same at 2^20 on a random curve over the 128-bit
                     field
  host               pointmul.ec_multiply on Python integers, one core, same machine
  product roof       field products per multiplication, counted from the formulas of csrc/curve.hip (a doubling 10, a mixed addition 11,
                     per bit; the final inversion; the four products that make the result affine), over the rate at which THIS flavour
                     of the library multiplies when nothing else limits it: gs_vec_exp over 2^20 elements with an exponent of all ones,
                     two products per exponent bit with both chains in registers.  The fraction is roof time / measured time.

Times are host clock around `reps` back-to-back launches that end in one gs_sync, after a warm-up of the same shape; every window is at
least --window seconds long and is taken --rounds times (the table has the median and the fastest).  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from genstark_amd import _abi                                    # noqa: E402
from genstark_amd._abi import Backend                            # noqa: E402
from genstark_amd.curve import Curve, curve224                   # noqa: E402
from genstark_amd.field import Matrix, PrimeField, Vector        # noqa: E402
from genstark_amd.pointmul import ec_multiply                    # noqa: E402
from sponge_bench import timed                                   # noqa: E402

BITS, DOUBLE, ADD, AFFINE = 256, 10, 11, 4
# products of fe_inv: the wide flavours run fe_pow over all 256 exponent bits (256 squarings + one product per set bit of p - 2, 223 for
# 2^224 - 2^96 + 1); the 128-bit field has an addition chain (gf128.h: 139 squarings + 12 products)
INVERSION = {'p224': 256 + 223, 'p128': 139 + 12}
# waves per SIMD of k_curve_mul<fixed> / <variable>, from -Rpass-analysis=kernel-resource-usage
OCCUPANCY = {'p224': (3, 3), 'p128': (6, 5)}
SIZES = {'p224': (12, 16, 20), 'p128': (20,)}


def products_per_multiplication(name):
    return BITS * (DOUBLE + ADD) + INVERSION[name] + AFFINE


def rounds_of(be, launch, window, rounds):
    times = [timed(be, launch, window) for _ in range(rounds)]
    return statistics.median(t for t, _ in times), min(t for t, _ in times), times[0][1]


def product_rate(be, f, window, rounds):
    """products per second of this flavour's fe_mul on the whole chip: fe_pow with an exponent of all ones"""
    n, ebits = 1 << 20, 8 * f.elementSize
    src, out = f.getPowerSeries(3, n), f.newVector(n)
    e = bytes([0xFF]) * f.elementSize
    med, best, _ = rounds_of(be, lambda: be.call('gs_vec_exp', C.c_void_p(src.ptr), e, n, C.c_void_p(out.ptr)), window, rounds)
    return n * 2 * ebits / med, n * 2 * ebits / best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'curve.md'))
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    rng = random.Random(0xC0FFEE)
    lines = ['# Scalar multiplications on the device (tools/curve_bench.py)', '',
             f'{BITS}-bit scalars, one thread per multiplication (csrc/curve.hip).  Time per launch: host clock around back-to-back launches ending in one synchronise,',
             f'after a warm-up of the same shape; windows of at least {args.window} s, {args.rounds} rounds: the median, and the fastest in brackets.',
             'Product roof: products per multiplication (counted from the formulas) over the rate of `gs_vec_exp` with an exponent of all ones in the same',
             'flavour (two register-only product chains per element, 2^20 elements): what the chip does when it only multiplies.', '']
    for name, modulus in (('p224', _abi.MODULUS_224), ('p128', None)):
        be = Backend(device=0, modulus=modulus)
        f = PrimeField(backend=be)
        p = f.modulus
        if name == 'p224':
            curve = curve224(f)
            G = curve.G
        else:
            a = rng.randrange(1, p - 3)
            G = (rng.randrange(p), rng.randrange(1, p))
            curve = Curve(f, a, G[1] * G[1] - G[0] ** 3 - a * G[0])
        per = products_per_multiplication(name)
        rate, rate_best = product_rate(be, f, args.window, args.rounds)
        n = 1 << max(SIZES[name])
        ks = Vector(be, n * 32, element_size=1)
        be.upload(ks.ptr, rng.randbytes(n * 32))
        base = f.newMatrixFrom([list(G)])
        # the points of the variable-base rows: k * G, made by the kernel itself
        points, flags = Matrix(be, n, 2), Vector(be, n, element_size=1)
        a_le = f.le(curve.a)
        be.call('gs_curve_mul', a_le, C.c_void_p(base.ptr), 1, C.c_void_p(ks.ptr), BITS, None, None, n, C.c_void_p(points.ptr), C.c_void_p(flags.ptr))
        assert not any(be.download(flags.ptr, n)), 'a random multiple of the base point is infinity'
        assert curve.containsMany(Matrix(be, 4096, 2, owner=points._owner)) == [True] * 4096
        out = Matrix(be, n, 2)
        lines += [f'## {name}: {per} products per multiplication = {BITS} x ({DOUBLE} + {ADD}) + {INVERSION[name]} (inversion) + {AFFINE}', '',
                  f'This flavour multiplies at {rate / 1e9:.1f} G products/s ({rate_best / 1e9:.1f} at best) in `gs_vec_exp`: {per / rate * 1e9:.1f} ns of the whole chip per multiplication.', '',
                  '| base | multiplications | waves per SIMD | reps | ms per launch | M multiplications/s | G products/s | fraction of product roof |', '|---|---|---|---|---|---|---|---|']
        fastest = {}
        for kind, src, npoints, occ in (('variable', points, None, OCCUPANCY[name][1]), ('fixed', base, 1, OCCUPANCY[name][0])):
            for log in SIZES[name]:
                count = 1 << log
                launch = lambda: be.call('gs_curve_mul', a_le, C.c_void_p(src.ptr), npoints or count, C.c_void_p(ks.ptr), BITS, None, None, count, C.c_void_p(out.ptr),
                                         C.c_void_p(flags.ptr))
                med, best, reps = rounds_of(be, launch, args.window, args.rounds)
                fastest[kind] = count / med
                lines.append(f'| {kind} | 2^{log} | {occ} | {reps} | {med * 1e3:.3f} ({best * 1e3:.3f}) | {count / med / 1e6:.3f} | {count * per / med / 1e9:.1f} | {count * per / rate / med:.3f} |')
        lines.append('')
        if name == 'p224':
            sample = [rng.getrandbits(BITS) for _ in range(8)]
            t0 = time.perf_counter()
            want = [ec_multiply(p, G, k) for k in sample]
            host = (time.perf_counter() - t0) / len(sample)
            assert curve.mulMany(G, sample) == want
            lines += [f'Host integers (pointmul.ec_multiply, Python, one core): {host * 1e3:.1f} ms per multiplication = {1 / host:.1f} multiplications/s; the device at 2^20 is '
                      f'{fastest["variable"] * host:,.0f} x (variable base) and {fastest["fixed"] * host:,.0f} x (fixed base) that.', '']
        be.close()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write(text)
    print(text)


if __name__ == '__main__':
    main()
