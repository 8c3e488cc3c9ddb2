"""tools/scan_bench.py [--out profiles/scan.md] — running sums, products and linear recurrences on the MI355X (include/gstark_scan.h),
written as a profile.

  cases          each op (sum, product, the recurrence with a vector of factors) at 2^24 elements in the 128-bit field and at 2^22 in
                 the 224-bit field: one segment, 2^12 uniform segments, flagged segments of mean length 7
  bytes          algorithmic: every input read twice (the tile pass and the apply pass), the output written once
  copy roof      those bytes over the rate of `gs_copy` in the same run, moving the same number of bytes (a copy of half as many: every
                 byte is read once and written once)
  product roof   the field products the launches report to the traffic tally (per lane, kept or not) over the rate at which THIS flavour
                 multiplies when nothing else limits it: `gs_vec_exp` over 2^20 elements with an exponent of all ones, as
                 tools/sqrt_bench.py and profiles/curve.md use
  before         the host-integer fallback at 2^20 elements of the 128-bit field: one read-back, a Python loop, one upload
  registers      VGPRs, scratch bytes per lane and waves per SIMD of every kernel in every flavour, from the compiler
                 (-Rpass-analysis=kernel-resource-usage; RESOURCES below is copied from its report)

Times are device events on the context's stream around `reps` back-to-back calls (each call is its one to three launches), after a warm-up
of the same shape; every window is at least --window seconds long and is taken --rounds times (the table has the median and the
fastest).  Needs the GPU: no fallback."""
import argparse
import ctypes as C
import itertools
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from genstark_amd import _abi                                    # noqa: E402
from genstark_amd._abi import Backend                            # noqa: E402
from genstark_amd.field import PrimeField, Vector                # noqa: E402

TIMED = (('p128', None, 24), ('p224', _abi.MODULUS_224, 22))
SEGMENTS_LOG = 12
MEAN_RUN = 7
BEFORE_LOG = 20
# (VGPRs, scratch bytes per lane, waves per SIMD) of k_scan_tiles | k_scan_totals | k_scan_apply, for the sum, the product and the recurrence
RESOURCES = {
    'p128': (((26, 0, 8), (22, 0, 8), (41, 0, 8)), ((54, 0, 8), (48, 0, 8), (64, 0, 8)), ((68, 0, 7), (55, 0, 8), (91, 0, 5))),
    'q64': (((22, 0, 8), (20, 0, 8), (32, 0, 8)), ((28, 0, 8), (30, 0, 8), (36, 0, 8)), ((38, 0, 8), (46, 0, 8), (52, 0, 8))),
    'q32': (((22, 0, 8), (20, 0, 8), (32, 0, 8)), ((22, 0, 8), (20, 0, 8), (28, 0, 8)), ((35, 0, 8), (28, 0, 8), (46, 0, 8))),
    'q17': (((22, 0, 8), (20, 0, 8), (32, 0, 8)), ((22, 0, 8), (20, 0, 8), (28, 0, 8)), ((35, 0, 8), (28, 0, 8), (46, 0, 8))),
    'p256': (((72, 0, 7), (60, 0, 8), (92, 0, 5)), ((58, 0, 8), (70, 0, 7), (74, 0, 6)), ((107, 0, 4), (88, 0, 5), (137, 0, 3))),
    'p224': (((72, 0, 7), (60, 0, 8), (92, 0, 5)), ((56, 0, 8), (70, 0, 7), (70, 0, 7)), ((96, 0, 5), (74, 0, 6), (128, 0, 4))),
    'runtime modulus': (((68, 0, 7), (56, 0, 8), (88, 0, 5)), ((64, 240, 8), (65, 176, 7), (69, 240, 7)), ((84, 464, 5), (85, 336, 5), (107, 496, 4))),
}

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


def host_before(f, vec, avec):
    """seconds of the three ops the way a caller had them before: read back, loop on Python integers, upload"""
    p, out = f.modulus, {}
    for op in ('sum', 'product', 'affine'):
        t0 = time.perf_counter()
        values = vec.toValues()
        if op == 'sum':
            res = list(itertools.accumulate(values, lambda x, y: (x + y) % p))
        elif op == 'product':
            res = list(itertools.accumulate(values, lambda x, y: x * y % p))
        else:
            res, x = [], 0
            for a, b in zip(avec.toValues(), values):
                x = (a * x + b) % p
                res.append(x)
        f.newVectorFrom(res)
        f.backend.sync()
        out[op] = time.perf_counter() - t0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scan.md'))
    ap.add_argument('--window', type=float, default=0.2)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    lines = ['# Running sums, products and linear recurrences on the device (tools/scan_bench.py)', '',
             'Reduce-then-scan in three launches (csrc/scan.hip, the schedule of csrc/scan_plan.h); each thread owns the consecutive elements that fill 64 bytes.  Time per',
             f'call (its three launches): device events around back-to-back calls after a warm-up of the same shape; windows of at least {args.window} s, {args.rounds} rounds: the median, and',
             'the fastest in brackets.  Bytes: every input read twice, the output written once.  Copy roof: `gs_copy` moving the same number of bytes (a copy of half as',
             'many) in the same run.  Product roof: the products the launches report (per lane, kept or not) over the rate of `gs_vec_exp` with an exponent of all ones in',
             'the same flavour (2^20 elements), as in profiles/sqrt.md.  A fraction is roof time / measured time.', '']
    slow = []
    for name, modulus, log in TIMED:
        be = Backend(device=0, modulus=modulus)
        f = PrimeField(backend=be)
        ev = Events(be)
        es, n = f.elementSize, 1 << log
        plan = f.scanPlan(n)
        src, out = f.getPowerSeries(3, 1 << 20), f.newVector(1 << 20)
        e = bytes([0xFF]) * es
        med, _, _ = ev.timed(lambda: be.call('gs_vec_exp', C.c_void_p(src.ptr), e, 1 << 20, C.c_void_p(out.ptr)), args.window, args.rounds)
        rate = (1 << 20) * 2 * 8 * es / med
        values, factors, out = f.getPowerSeries(3, n), f.getPowerSeries(5, n), f.newVector(n)
        spare = f.newVector(n)
        heads = Vector(be, n, element_size=1)
        flags = (np.random.default_rng(0x5CA9).random(n) < 1.0 / MEAN_RUN).astype(np.uint8)
        be.upload(heads.ptr, flags.tobytes())
        rows, cols = 1 << SEGMENTS_LOG, n >> SEGMENTS_LOG
        lines += [f'## {name}: 2^{log} elements of {es} bytes, tiles of {plan["tile"]} ({plan["elementsPerThread"]} per thread), {plan["launches"]} launches', '',
                  f'This flavour multiplies at {rate / 1e9:.1f} G products/s in `gs_vec_exp`.  Flagged segments: {int(flags.sum())} heads, mean run {n / max(int(flags.sum()), 1):.2f}.', '',
                  '| op | segments | MB moved | products per element | reps | ms per call | G elements/s | TB/s | copy of the same bytes: ms, TB/s | fraction of copy roof | fraction of product roof |',
                  '|---|---|---|---|---|---|---|---|---|---|---|']
        ptr = lambda v: C.c_void_p(v.ptr)
        for op in ('sum', 'product', 'affine'):
            for form, hd, r, c in (('one', None, 1, n), (f'2^{SEGMENTS_LOG} uniform', None, rows, cols), (f'flagged, mean {MEAN_RUN}', heads, 1, n)):
                if op == 'affine':
                    launch = lambda hd=hd, r=r, c=c: be.call('gs_scan_affine', 0, ptr(factors), None, ptr(values), None, ptr(hd) if hd else None, r, c, ptr(out))
                else:
                    launch = lambda hd=hd, r=r, c=c, code=0 if op == 'sum' else 1: be.call('gs_scan', code, 0, ptr(values), ptr(hd) if hd else None, r, c, ptr(out), None)
                be.traffic(True)
                launch()
                tally = be.traffic()
                be.traffic(False)
                products = sum(v['units'] for k, v in tally.items() if k.startswith('k_scan_'))
                assert sum(v['launches'] for k, v in tally.items() if k.startswith('k_scan_')) == plan['launches']
                moved = n * es * ((2 if op == 'affine' else 1) * 2 + 1) + (2 * n if hd else 0)
                med, best, reps = ev.timed(launch, args.window, args.rounds)
                half = moved // 2 // es * es
                pieces = [(k * n * es, min(n * es, half - k * n * es)) for k in range((half + n * es - 1) // (n * es))]     # a copy of `half` bytes, from buffers of n elements
                bufs = ((values, out), (factors, spare), (out, spare))
                copy = lambda: [be.call('gs_copy', C.c_void_p(bufs[k][1].ptr), C.c_void_p(bufs[k][0].ptr), size) for k, (_, size) in enumerate(pieces)]
                cmed, _, _ = ev.timed(copy, args.window, args.rounds)
                copy_fraction, product_fraction = cmed / med, products / rate / med
                lines.append(f'| {op} | {form} | {moved / 1e6:.0f} | {products / n:.2f} | {reps} | {med * 1e3:.3f} ({best * 1e3:.3f}) | {n / med / 1e9:.2f} | {moved / med / 1e12:.2f} | '
                             f'{cmed * 1e3:.3f}, {2 * half / cmed / 1e12:.2f} | {copy_fraction:.2f} | {product_fraction:.2f} |')
                if copy_fraction < 0.5 and product_fraction < 0.5:
                    slow.append(f'{name} {op}, {form}: {copy_fraction:.2f} of the copy roof and {product_fraction:.2f} of the product roof')
        lines.append('')
        if name == 'p128':
            m = 1 << BEFORE_LOG
            vec, avec, res = f.getPowerSeries(3, m), f.getPowerSeries(5, m), f.newVector(m)
            before = host_before(f, vec, avec)
            lines += [f'Before (the host-integer fallback at 2^{BEFORE_LOG} elements: one read-back, a Python loop, one upload) against one call on the device at the same length:', '',
                      '| op | before: s | device: ms | ratio |', '|---|---|---|---|']
            for op in ('sum', 'product', 'affine'):
                if op == 'affine':
                    launch = lambda: be.call('gs_scan_affine', 0, ptr(avec), None, ptr(vec), None, None, 1, m, ptr(res))
                else:
                    launch = lambda code=0 if op == 'sum' else 1: be.call('gs_scan', code, 0, ptr(vec), None, 1, m, ptr(res), None)
                med, _, _ = ev.timed(launch, args.window, args.rounds)
                lines.append(f'| {op} | {before[op]:.2f} | {med * 1e3:.3f} | {before[op] / med:,.0f} x |')
            lines.append('')
        be.close()
    lines += ['## What was found', '',
              'The sum runs at one rate in all three segment forms and is bound by memory: it multiplies nothing, and the flags cost the bytes of `heads` and nothing else.  The',
              'product and the recurrence are bound by products in both flavours.  With E elements per thread a lane issues (E + 7) / E products per element in the tile pass (its',
              'fold, six steps over the lanes of its wave, the prefix of its wave and lane) and (2E + 8) / E in the apply pass (the same, and the walk over its elements), twice',
              'that for the recurrence: 6.75 and 13.5 at E = 4, 10.5 and 21 at E = 2, where the floor is 3 and 6.  Six of them are the steps over the lanes, which every lane',
              'issues for ONE aggregate whether it keeps the result or not.  Twice the elements per thread (128 bytes per lane) would make that 4.9 and 6.75 products per element;',
              'that form was not built or measured, and neither was the coalesced load with a transpose through LDS.  Nothing was tuned after this measurement.', '']
    lines += ['## Cases under half of both roofs', ''] + ([f'- {s}' for s in slow] if slow else ['None.']) + ['']
    lines += ['## Registers (from the compiler)', '', 'VGPRs, scratch bytes per lane, waves per SIMD of k_scan_tiles / k_scan_totals / k_scan_apply.', '',
              '| flavour | sum | product | recurrence |', '|---|---|---|---|']
    for name, ops in RESOURCES.items():
        lines.append(f'| {name} | ' + ' | '.join(' / '.join(f'{v}, {sc} B, {occ}' for v, sc, occ in kernels) for kernels in ops) + ' |')
    lines += ['', 'The runtime-modulus flavour\'s product is a function call (csrc/gf_wide.h) whose operands travel by reference: those are its scratch bytes, in every',
              'kernel of that flavour that multiplies; no fixed flavour uses scratch.', '']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write(text)
    print(text)


if __name__ == '__main__':
    main()
