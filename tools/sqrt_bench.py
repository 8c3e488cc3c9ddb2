"""tools/sqrt_bench.py [--out profiles/sqrt.md] — square roots and lifts on the MI355X (include/gstark_sqrt.h), written as a profile.

  roots/s, lifts/s   the 128- and 224-bit fields, 2^12, 2^16 and 2^20 elements per launch; flags only (Euler's criterion) at 2^20
  products           per flavour, the plan's products per root (gs_field_sqrt_plan) next to the textbook Tonelli-Shanks loop's count on
                     the same 256 random squares: the initial exponentiation by binary square-and-multiply, then per pass the squarings
                     that find the order of b, the squarings that raise c, and three products; as the mean over the elements and as the
                     mean over groups of 64 of the group's maximum (what a wave with one lane per root would run).  Host integers.
  product roof       the plan's products per root over the rate at which THIS flavour of the library multiplies when nothing else limits
                     it: gs_vec_exp over 2^20 elements with an exponent of all ones, two products per exponent bit with both chains in
                     registers — the roof profiles/curve.md states its 0.92 against.  The fraction is roof time / measured time.
  host               genstark_amd.field.host_sqrt (Tonelli-Shanks on Python integers), one core, same machine
  registers          VGPRs, scratch bytes per lane and waves per SIMD of the kernel each flavour launches, from the compiler
                     (-Rpass-analysis=kernel-resource-usage; RESOURCES below is copied from its report)

Times are device events on the context's stream around `reps` back-to-back launches, after a warm-up of the same shape; every window is
at least --window seconds long and is taken --rounds times (the table has the median and the fastest).  Needs the GPU: no fallback."""
import argparse
import ctypes as C
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from genstark_amd import _abi                                    # noqa: E402
from genstark_amd._abi import Backend                            # noqa: E402
from genstark_amd.curve import Curve, curve224                   # noqa: E402
from genstark_amd.field import PrimeField, Vector, host_sqrt     # noqa: E402

FLAVOURS = (('p128', None), ('q64', _abi.MODULUS_64), ('q32', _abi.MODULUS_32), ('q17', _abi.MODULUS_17), ('p256', _abi.MODULUS_256), ('p224', _abi.MODULUS_224))
TIMED = ('p128', 'p224')
LOGS = (12, 16, 20)
# kernel each flavour launches: (form, VGPRs + AGPRs, scratch bytes per lane, waves per SIMD) of k_field_sqrt | k_curve_lift_x | k_field_is_square
RESOURCES = {'p128': ('chain<4>', (58, 0, 8), (62, 0, 8), (54, 0, 8)), 'q64': ('chain<4>', (34, 0, 8), (36, 0, 8), (30, 0, 8)),
             'q32': ('chain<4>', (27, 0, 8), (29, 0, 8), (20, 0, 8)), 'q17': ('chain<2>', (23, 0, 8), (25, 0, 8), (18, 0, 8)),
             'p256': ('chain<4>', (124, 0, 4), (146, 0, 3), (92, 0, 5)), 'p224': ('chain<12>', (226, 0, 2), (263, 0, 1), (84, 0, 5)),
             'runtime modulus': ('window', (86, 208, 5), (86, 272, 5), (82, 208, 5))}

try:
    hip = C.CDLL('libamdhip64.so')
except OSError:
    hip = C.CDLL(os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'libamdhip64.so'))


class Events:
    def __init__(self, be):
        self.be, self.stream = be, C.c_void_p(be.stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(self.a)) == 0 and hip.hipEventCreate(C.byref(self.b)) == 0

    def seconds(self, launch, reps):
        assert hip.hipEventRecord(self.a, self.stream) == 0
        for _ in range(reps):
            launch()
        assert hip.hipEventRecord(self.b, self.stream) == 0 and hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value / 1e3 / reps

    def timed(self, launch, window, rounds):
        launch()
        self.be.sync()
        once = max(self.seconds(launch, 1), 1e-6)
        reps = max(3, int(window / once) + 1)
        times = [self.seconds(launch, reps) for _ in range(rounds)]
        return statistics.median(times), min(times), reps


def binary_products(e):
    return max(e.bit_length() - 1, 0) + max(bin(e).count('1') - 1, 0)


def textbook_products(a, p, s, t, c):
    """field products of plain Tonelli-Shanks for the square a: (exponentiations, loop)"""
    first = binary_products((t + 1) // 2) + binary_products(t)
    loop, b, m = 0, pow(a, t, p), s
    while b != 1:
        i, sq = 0, b
        while sq != 1:
            sq, i, loop = sq * sq % p, i + 1, loop + 1
        f = pow(c, 1 << (m - i - 1), p)
        loop += (m - i - 1) + 3
        c = f * f % p
        b, m = b * c % p, i
    return first, loop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sqrt.md'))
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    rng = random.Random(0x5157)
    lines = ['# Square roots and lifts on the device (tools/sqrt_bench.py)', '',
             'One thread per element (csrc/sqrt.hip), the schedule of csrc/sqrt_plan.h.  Time per launch: device events around back-to-back launches after a warm-up of',
             f'the same shape; windows of at least {args.window} s, {args.rounds} rounds: the median, and the fastest in brackets.  Product roof: the plan\'s products per root over',
             'the rate of `gs_vec_exp` with an exponent of all ones in the same flavour (two register-only product chains per element, 2^20 elements), as in',
             'profiles/curve.md; `bench.py --full` measures its `second_roof` for the 128-bit field only, so that figure is not used here.', '']
    plans, table = {}, []
    for name, modulus in FLAVOURS:
        be = Backend(device=0, modulus=modulus)
        f = PrimeField(backend=be)
        ev = Events(be)
        p = f.modulus
        plan = plans[name] = f.sqrtPlan()
        s = plan['twoAdicity']
        t = (p - 1) >> s
        z = next(z for z in range(2, 1000) if pow(z, (p - 1) // 2, p) == p - 1)
        squares = [pow(rng.randrange(1, p), 2, p) for _ in range(256)]
        counts = [textbook_products(a, p, s, t, pow(z, t, p)) for a in squares]
        loops = [loop for _, loop in counts]
        per64 = [max(loops[k:k + 64]) for k in range(0, 256, 64)]
        roots, flags = f.sqrtVectorElements(squares)                         # ... and the device agrees with the definition on them
        assert all(r * r % p == a and r % 2 == 0 for r, a in zip(roots.toValues(), squares)) and all(flags.toBuffer())
        table.append(f'| {name} | {s} | {plan["windows"]} x {plan["windowBits"]} | {RESOURCES[name][0]} | {plan["productsPerRoot"]} | {counts[0][0]} + {statistics.mean(loops):.0f} | '
                     f'{counts[0][0]} + {statistics.mean(per64):.0f} |')
        if name in TIMED:
            n = 1 << max(LOGS)
            src, out = f.getPowerSeries(3, n), f.newVector(n)
            e = bytes([0xFF]) * f.elementSize
            med, best, _ = ev.timed(lambda: be.call('gs_vec_exp', C.c_void_p(src.ptr), e, n, C.c_void_p(out.ptr)), args.window, args.rounds)
            rate = n * 2 * 8 * f.elementSize / med
            if name == 'p224':
                curve = curve224(f)
            else:
                curve = Curve(f, rng.randrange(1, p), rng.randrange(1, p))
            per, per_flag = plan['productsPerRoot'], None
            points, lflags, rflags = f.newMatrix(n, 2), Vector(be, n, element_size=1), Vector(be, n, element_size=1)
            a_le, b_le = f.le(curve.a), f.le(curve.b)
            lines += [f'## {name}: {per} products per root ({RESOURCES[name][0]}, {plan["windows"]} windows of {plan["windowBits"]} bits over s = {s})', '',
                      f'This flavour multiplies at {rate / 1e9:.1f} G products/s in `gs_vec_exp`: {per / rate * 1e9:.2f} ns of the whole chip per root.', '',
                      '| call | elements | waves per SIMD | reps | ms per launch | M elements/s | G products/s | fraction of product roof |', '|---|---|---|---|---|---|---|---|']
            be.traffic(True)
            be.call('gs_field_sqrt', C.c_void_p(src.ptr), 64, None, C.c_void_p(rflags.ptr))
            per_flag = [v['units'] for k, v in be.traffic().items() if k == 'k_field_is_square'][0] // 64
            be.traffic(False)
            for kind, products, occ, launch_of in (
                    ('roots', per, RESOURCES[name][1][2], lambda c: lambda: be.call('gs_field_sqrt', C.c_void_p(src.ptr), c, C.c_void_p(out.ptr), C.c_void_p(rflags.ptr))),
                    ('lifts', per + 2, RESOURCES[name][2][2], lambda c: lambda: be.call('gs_curve_lift_x', a_le, b_le, C.c_void_p(src.ptr), None, c, C.c_void_p(points.ptr), C.c_void_p(lflags.ptr))),
                    ('flags only', per_flag, RESOURCES[name][3][2], lambda c: lambda: be.call('gs_field_sqrt', C.c_void_p(src.ptr), c, None, C.c_void_p(rflags.ptr)))):
                for log in (LOGS if kind != 'flags only' else LOGS[-1:]):
                    count = 1 << log
                    med, best, reps = ev.timed(launch_of(count), args.window, args.rounds)
                    lines.append(f'| {kind} | 2^{log} | {occ} | {reps} | {med * 1e3:.3f} ({best * 1e3:.3f}) | {count / med / 1e6:.3f} | {count * products / med / 1e9:.1f} | '
                                 f'{count * products / rate / med:.3f} |')
                    if kind == 'roots' and log == max(LOGS):
                        device_rate = count / med
            sample = squares[:64]
            t0 = time.perf_counter()
            want = [host_sqrt(a, p) for a in sample]
            host = (time.perf_counter() - t0) / len(sample)
            assert f.sqrtVectorElements(sample)[0].toValues() == want
            lines += ['', f'Host integers (genstark_amd.field.host_sqrt, Python, one core): {host * 1e6:.0f} us per root = {1 / host:,.0f} roots/s; the device at 2^20 is '
                      f'{device_rate * host:,.0f} x that.', '']
        be.close()
    lines += ['Where `lifts` fall behind `roots` in the same flavour the difference is occupancy, not products (a lift is two products more): in the 224-bit flavour',
              '`k_curve_lift_x<12>` holds x beside the twelve kept powers and the product\'s temporaries in 263 registers, ONE wave per SIMD where `k_field_sqrt<12>` runs two',
              '(the table of registers below).  Nothing was tuned after this measurement.', '',
              '## Products per root, per flavour', '',
              'The plan against textbook Tonelli-Shanks on the same 256 random squares (host integers): exponentiations + loop, the loop as the mean over the',
              'elements and as the mean over groups of 64 of the slowest element of the group.', '',
              '| flavour | s | windows | form | plan: products per root | textbook: mean | textbook: mean of per-64 maxima |', '|---|---|---|---|---|---|---|'] + table
    lines += ['', '## Registers (from the compiler)', '', '| flavour | form | k_field_sqrt: VGPRs, scratch, waves/SIMD | k_curve_lift_x | k_field_is_square |', '|---|---|---|---|---|']
    for name, (form, *kernels) in RESOURCES.items():
        lines.append(f'| {name} | {form} | ' + ' | '.join(f'{v}, {sc} B, {occ}' for v, sc, occ in kernels) + ' |')
    lines += ['', 'The runtime-modulus flavour\'s product is a function call (csrc/gf_wide.h) whose operands travel by reference: those are its scratch bytes, in every',
              'kernel of that flavour that multiplies; no fixed flavour uses scratch.', '']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write(text)
    print(text)


if __name__ == '__main__':
    main()
