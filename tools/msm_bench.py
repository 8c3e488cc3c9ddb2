"""tools/msm_bench.py [--out profiles/msm.md] — sums of scalar multiples on the MI355X (include/gstark_msm.h), written as a profile.

  msm                gs_curve_msm with the plan's own choice (window 0) over 2^12 ... 2^20 terms, 256-bit scalars, in the 224-bit and
                     the 128-bit flavour: uniform random scalars, and the batch whose scalars are all equal (every term of a window in one
                     bucket)
  baseline           gs_curve_mul (variable base) of the same count in the same run: the device part of what a caller without the entry
                     does, a lower bound of it (the read-back and the host's fold come on top)
  routes, windows    the same sum with each route forced (GSTARK_MSM_ROUTE, read by the entry per call) and with the window widths around
                     the plan's choice forced: what the thresholds of csrc/msm_plan.h are read from
  product roof       field products of the call as the plan counts them (the traffic tally's work units: every digit taken as non-zero)
                     over the rate of gs_vec_exp in the same flavour, as in tools/curve_bench.py

Times are host clock around `reps` back-to-back calls that end in one gs_sync, after a warm-up of the same shape; every window is at
least --window seconds long and is taken --rounds times (the table has the median and the fastest).  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from genstark_amd import _abi                                    # noqa: E402
from genstark_amd._abi import Backend                            # noqa: E402
from genstark_amd.curve import Curve, curve224                   # noqa: E402
from genstark_amd.field import Matrix, PrimeField, Vector        # noqa: E402
from curve_bench import product_rate, rounds_of                  # noqa: E402

BITS = 256
LOGS = (12, 14, 16, 18, 20)      # 2^12, 2^16 and 2^20 are the shapes the conditions are stated for; the two between place the crossover


def plan_window(count):
    """msm_choose_window of csrc/msm_plan.h, restated to label the rows (the timing of the forced width beside it shows they agree)"""
    lg = max(count - 1, 0).bit_length()
    return min(max(lg - 6, 7), 13)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'msm.md'))
    ap.add_argument('--json', default=None, help='also write the raw figures here')
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--spread', type=int, default=2, help='forced window widths on either side of the plan\'s choice')
    args = ap.parse_args()
    rng = random.Random(0x5C0FFEE)
    raw = {}
    lines = ['# Sums of scalar multiples on the device (tools/msm_bench.py)', '',
             f'{BITS}-bit scalars.  Time per call: host clock around back-to-back calls ending in one synchronise, after a warm-up of the same shape;',
             f'windows of at least {args.window} s, {args.rounds} rounds: the median, and the fastest in brackets.  `mul` is `gs_curve_mul` (variable base) of the same',
             'count in the same run: the device part of the multiply, read back and fold that a caller without `gs_curve_msm` does.  Products: the',
             'plan\'s count for the call (every digit taken as non-zero); the roof is that count over the rate of `gs_vec_exp` in the same flavour.', '']
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
        rate, rate_best = product_rate(be, f, args.window, args.rounds)
        n = 1 << max(LOGS)
        uniform, equal = Vector(be, n * 32, element_size=1), Vector(be, n * 32, element_size=1)
        be.upload(uniform.ptr, rng.randbytes(n * 32))
        be.upload(equal.ptr, rng.randbytes(32) * n)
        base = f.newMatrixFrom([list(G)])
        points, flags = Matrix(be, n, 2), Vector(be, n, element_size=1)
        a_le = f.le(curve.a)
        be.call('gs_curve_mul', a_le, C.c_void_p(base.ptr), 1, C.c_void_p(uniform.ptr), BITS, None, None, n, C.c_void_p(points.ptr), C.c_void_p(flags.ptr))
        assert not any(be.download(flags.ptr, n)), 'a random multiple of the base point is infinity'
        products, out, flag = Matrix(be, n, 2), Matrix(be, 1, 2), Vector(be, 1, element_size=1)

        def msm(count, scalars, window=0):
            return lambda: be.call('gs_curve_msm', a_le, C.c_void_p(points.ptr), C.c_void_p(scalars.ptr), 32, BITS, count, window, C.c_void_p(out.ptr), C.c_void_p(flag.ptr))

        def units(launch):
            be.traffic(True)
            launch()
            be.sync()
            tally = be.traffic()
            be.traffic(False)
            return sum(e['units'] for e in tally.values())

        def measure(launch, route=None):
            if route:
                os.environ['GSTARK_MSM_ROUTE'] = route
            try:
                med, best, reps = rounds_of(be, launch, args.window, args.rounds)
                return {'ms': med * 1e3, 'best_ms': best * 1e3, 'reps': reps, 'products': units(launch)}
            finally:
                os.environ.pop('GSTARK_MSM_ROUTE', None)

        # the sum agrees between the routes and with the all-equal identity before anything is timed
        check = {}
        for route in ('buckets', 'multiply_then_sum'):
            os.environ['GSTARK_MSM_ROUTE'] = route
            msm(1 << 12, uniform)()
            check[route] = (out.toValues(), flag.toBuffer())
            os.environ.pop('GSTARK_MSM_ROUTE')
        assert check['buckets'] == check['multiply_then_sum'] and check['buckets'][1] == b'\x00', check

        lines += [f'## {name}', '', f'This flavour multiplies at {rate / 1e9:.1f} G products/s ({rate_best / 1e9:.1f} at best) in `gs_vec_exp`.', '',
                  '| terms | what | ms per call | x mul | M products | fraction of product roof |', '|---|---|---|---|---|---|']
        raw[name] = {'rate': rate, 'rows': {}}
        for log in LOGS:
            count = 1 << log
            c0 = plan_window(count)
            rows = {'mul': measure(lambda: be.call('gs_curve_mul', a_le, C.c_void_p(points.ptr), count, C.c_void_p(uniform.ptr), BITS, None, None, count,
                                                   C.c_void_p(products.ptr), C.c_void_p(flags.ptr))),
                    'msm (plan), uniform': measure(msm(count, uniform)),
                    'msm (plan), all scalars equal': measure(msm(count, equal)),
                    'route buckets': measure(msm(count, uniform), 'buckets'),
                    'route multiply_then_sum': measure(msm(count, uniform), 'multiply_then_sum')}
            for c in range(max(1, c0 - args.spread), min(16, c0 + args.spread) + 1):
                rows[f'window {c}' + (' (the plan\'s width)' if c == c0 else '')] = measure(msm(count, uniform, c))
            mul = rows['mul']['ms']
            for what, r in rows.items():
                lines.append(f'| 2^{log} | {what} | {r["ms"]:.3f} ({r["best_ms"]:.3f}) | {r["ms"] / mul:.3f} | {r["products"] / 1e6:.1f} | {r["products"] / rate / (r["ms"] / 1e3):.3f} |')
            raw[name]['rows'][log] = rows
        lines.append('')
        be.close()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write(text)
    if args.json:
        json.dump(raw, open(args.json, 'w'), indent=1)
    print(text)


if __name__ == '__main__':
    main()
