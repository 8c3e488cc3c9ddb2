"""tools/poly_bench.py [--out profiles/poly.md] — long polynomials at arbitrary points on the MI355X (include/gstark_poly.h), written as a
profile.

  entries            gs_poly_from_roots, gs_poly_div (n coefficients by n / 2 + 1), gs_poly_eval_points (n coefficients at n points) and
                     gs_poly_interpolate_points at n = 2^8 ... 2^20 in the 128-bit and the 224-bit flavour
  against            code this family does not touch, in the same run: gs_small_interpolate (host, up to 4 096 points),
                     gs_eval_polys_at_points (Horner, n coefficients at n points, up to 2^16) and gs_boundary_polys on n points of a
                     domain of 2n (what interpolation costs when the points ARE domain points: a lower bound)
  switch-over        evaluation and interpolation with the tree's schoolbook switch-over forced to 2^4 ... 2^10 (gs_poly_schoolbook_log2)

Times are host clock around back-to-back calls that end in one gs_sync, after a warm-up of the same shape; every window is at least
--window seconds long and is taken --rounds times (the table has the median and min..max).  A cell over --budget seconds per call at the
size before is not measured at the next ("-").  Reads nothing outside the tree.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import json
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
from genstark_amd.field import PrimeField, Vector                # noqa: E402
from sponge_bench import timed                                   # noqa: E402

SWITCHES = (4, 5, 6, 7, 8, 9, 10)


def cell(be, launch, window, rounds):
    times = [timed(be, launch, window)[0] for _ in range(rounds)]
    return {'ms': statistics.median(times) * 1e3, 'min_ms': min(times) * 1e3, 'max_ms': max(times) * 1e3}


def host_cell(call, rounds):
    times = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return {'ms': statistics.median(times) * 1e3, 'min_ms': min(times) * 1e3, 'max_ms': max(times) * 1e3}


def show(c):
    return '-' if c is None else f'{c["ms"]:.3f} ({c["min_ms"]:.3f}..{c["max_ms"]:.3f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'poly.md'))
    ap.add_argument('--json', default=None, help='also write the raw figures here')
    ap.add_argument('--window', type=float, default=0.2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--logs', default='8,10,12,14,15,16,18,20')
    ap.add_argument('--switch-logs', default='12,16')
    ap.add_argument('--budget', type=float, default=0.5, help='seconds per call above which a reference is not measured at larger sizes')
    args = ap.parse_args()
    logs = [int(x) for x in args.logs.split(',')]
    switch_logs = [int(x) for x in args.switch_logs.split(',')]
    rng = random.Random(0x901BE)
    raw = {}
    lines = ['# Long polynomials at arbitrary points on the device (tools/poly_bench.py)', '',
             'ms per call: host clock around back-to-back calls ending in one synchronise, after a warm-up of the same shape; windows of at least',
             f'{args.window} s, {args.rounds} rounds: the median (min..max).  n random points; `from roots`: n roots; `div`: n coefficients by n / 2 + 1; `eval`: n coefficients at',
             'n points; `interpolate`: n points.  References, in the same run: `Horner` is `gs_eval_polys_at_points` (n coefficients at n points),',
             '`host` is `gs_small_interpolate` (one host core), `domain` is `gs_boundary_polys` through n points of a domain of 2n — interpolation',
             'when the points are domain points, a lower bound.  "-": not measured (outside the reference\'s range, or over the budget of',
             f'{args.budget} s per call one size earlier).', '']
    for name, modulus in (('p128', None), ('p224', _abi.MODULUS_224)):
        be = Backend(device=0, modulus=modulus)
        f = PrimeField(backend=be)
        p, es = f.modulus, f.elementSize
        omega, omega_log2 = f._polyOmega()
        setter = be.lib.gs_poly_schoolbook_log2
        top = 1 << max(logs)
        xs, ys, poly = Vector(be, top), Vector(be, top), Vector(be, top)
        be.call('gs_power_series', f.le(rng.randrange(2, p)), top, C.c_void_p(xs.ptr))         # distinct unless the base has a small order
        be.call('gs_power_series', f.le(rng.randrange(2, p)), top, C.c_void_p(ys.ptr))
        be.call('gs_power_series', f.le(rng.randrange(2, p)), top, C.c_void_p(poly.ptr))
        out, out2, flag = Vector(be, top + 1), Vector(be, top + 1), Vector(be, 1, element_size=1)
        ptr = lambda v: C.c_void_p(v.ptr)

        def entries(n):
            return {'from roots': lambda: be.call('gs_poly_from_roots', omega, omega_log2, ptr(xs), n, ptr(out)),
                    'div': lambda: be.call('gs_poly_div', omega, omega_log2, ptr(poly), n, ptr(ys), n // 2 + 1, ptr(out), ptr(out2)),
                    'eval': lambda: be.call('gs_poly_eval_points', omega, omega_log2, ptr(poly), n, ptr(xs), n, ptr(out)),
                    'interpolate': lambda: be.call('gs_poly_interpolate_points', omega, omega_log2, ptr(xs), ptr(ys), n, ptr(out), ptr(flag))}

        # the routes agree before anything is timed: tree against Horner, interpolation evaluated back
        n = 1 << min(logs)
        entries(n)['eval']()
        tree_values = out.toBuffer(0, n)
        points = be.download(xs.ptr, n * es)
        lens = (C.c_uint64 * 1)(n)
        be.call('gs_eval_polys_at_points', ptr(poly), 1, n, lens, points, n, ptr(out2))
        assert out2.toBuffer(0, n) == tree_values, 'tree and Horner disagree'
        entries(n)['interpolate']()
        assert flag.toBuffer() == b'\x00'
        be.call('gs_eval_polys_at_points', ptr(out), 1, n, lens, points, n, ptr(out2))
        assert out2.toBuffer(0, n) == ys.toBuffer(0, n), 'the interpolant misses its points'

        lines += [f'## {name}', '', '| n | from roots | div | eval | Horner | interpolate | host | domain |', '|---|---|---|---|---|---|---|---|']
        raw[name] = {'rows': {}, 'switch': {}}
        over = set()
        for log in logs:
            n = 1 << log
            row = {what: cell(be, launch, args.window, args.rounds) for what, launch in entries(n).items()}
            row['Horner'] = row['host'] = row['domain'] = None
            if log <= 16 and 'Horner' not in over:
                points = be.download(xs.ptr, n * es)
                lens = (C.c_uint64 * 1)(n)
                row['Horner'] = cell(be, lambda: be.call('gs_eval_polys_at_points', ptr(poly), 1, n, lens, points, n, ptr(out)), args.window, args.rounds)
            if n <= 4096 and 'host' not in over:
                xb, yb = be.download(xs.ptr, n * es), be.download(ys.ptr, n * es)
                res = C.create_string_buffer(n * es)
                row['host'] = host_cell(lambda: be.lib.gs_small_interpolate(xb, yb, n, C.cast(res, C.c_void_p)), args.rounds)
            if hasattr(be.lib, 'gs_boundary_polys') and 2 * n <= (1 << omega_log2) // 2 and 'domain' not in over:
                w = f.le(pow(int.from_bytes(omega, 'little'), (1 << omega_log2) // (4 * n), p))
                steps = (C.c_uint64 * n)(*rng.sample(range(2 * n), n))
                values, per_row = be.download(ys.ptr, n * es), (C.c_uint32 * 1)(n)
                row['domain'] = cell(be, lambda: be.call('gs_boundary_polys', w, 4 * n, 2 * n, steps, values, per_row, 1, n, ptr(out), ptr(out2)), args.window, args.rounds)
            for what in ('Horner', 'host', 'domain'):
                if row[what] and row[what]['ms'] > args.budget * 1e3:
                    over.add(what)
            lines.append(f'| 2^{log} | ' + ' | '.join(show(row[what]) for what in ('from roots', 'div', 'eval', 'Horner', 'interpolate', 'host', 'domain')) + ' |')
            raw[name]['rows'][log] = row
            print(name, lines[-1], file=sys.stderr, flush=True)
        lines += ['', 'The tree\'s switch-over forced (slots of at most 2^s elements are schoolbook), ms per call:', '',
                  '| n | entry | ' + ' | '.join(f's = {s}' for s in SWITCHES) + ' |', '|---|---|' + '---|' * len(SWITCHES)]
        before = setter(8)
        try:
            for log in switch_logs:
                n = 1 << log
                for what in ('eval', 'interpolate'):
                    cells = []
                    for s in SWITCHES:
                        setter(s)
                        cells.append(cell(be, entries(n)[what], args.window, args.rounds))
                    raw[name]['switch'][f'{log} {what}'] = cells
                    lines.append(f'| 2^{log} | {what} | ' + ' | '.join(f'{c["ms"]:.3f}' for c in cells) + ' |')
                    print(name, lines[-1], file=sys.stderr, flush=True)
        finally:
            setter(before)
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
