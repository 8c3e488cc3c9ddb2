"""tools/diagnose_bench.py [--out profiles/diagnose.md] — the statement diagnosis on the MI355X (include/gstark_diagnose.h), as a profile.

  scan      gs_nonzero_spans over 8 rows x 2^24 elements of the 128-bit field (2 GiB read), dense non-zero and all zero, in GB/s of the
            bytes it has to read, next to gs_copy of the same bytes (which reads AND writes them) in the same run
  diagnose  Prover.diagnose next to Prover.prove_bytes, in ms, for poseidon_seg_256 and poseidon_c4_65536 (tests/generic_cases.py)

Times are host clock around back-to-back calls that end in a device synchronise (gs_nonzero_spans synchronises itself: it returns with
its results), after a warm-up of the same shape; every window is at least --window seconds long and is taken --rounds times (median,
fastest in brackets).  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from genstark_amd._abi import Backend                            # noqa: E402
from genstark_amd.prover import Prover                           # noqa: E402
from sponge_bench import timed                                   # noqa: E402

ROWS, LOG_N = 8, 24


def rounds_of(be, launch, window, rounds):
    times = [timed(be, launch, window)[0] for _ in range(rounds)]
    return statistics.median(times), min(times)


def wall(fn, window, rounds):
    """seconds per call of a function that returns with the device idle"""
    fn()
    out = []
    for _ in range(rounds):
        t0, reps = time.perf_counter(), 0
        while reps < 3 or time.perf_counter() - t0 < window:
            fn()
            reps += 1
        out.append((time.perf_counter() - t0) / reps)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'diagnose.md'))
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    be = Backend(device=0).jit(False)
    assert be.name == 'hip-gfx950'
    es, n = be.element_size, 1 << LOG_N
    nbytes = ROWS * n * es
    src, dst = be.alloc(nbytes), be.alloc(nbytes)
    out = [(C.c_uint64 * ROWS)() for _ in range(3)]
    scan = lambda: be.call('gs_nonzero_spans', C.c_void_p(src), ROWS, n, n, *out)
    copy = lambda: be.call('gs_copy', C.c_void_p(dst), C.c_void_p(src), nbytes)
    lines = ['# The statement diagnosis on the device (tools/diagnose_bench.py)', '',
             f'Host clock around back-to-back calls ending in a device synchronise, after a warm-up of the same shape; windows of at least {args.window} s,',
             f'{args.rounds} rounds: the median, and the fastest in brackets.', '',
             f'## gs_nonzero_spans: {ROWS} rows x 2^{LOG_N} elements of the 128-bit field ({nbytes / 2**30:.0f} GiB)', '',
             'GB/s of the bytes the scan reads; `gs_copy` of the same bytes reads and writes them, so its traffic is twice its size.', '',
             '| pass | ms | GB/s of the matrix | GB/s of traffic |', '|---|---|---|---|']
    rates = {}
    for label, fill in (('dense non-zero', b'\x01' + bytes(es - 1)), ('all zero', bytes(es))):
        chunk = fill * (1 << 16)                                          # one upload, then doubled on the device
        be.upload(src, chunk)
        have = len(chunk)
        while have < nbytes:
            be.call('gs_copy', C.c_void_p(src + have), C.c_void_p(src), min(have, nbytes - have))
            have *= 2
        be.sync()
        med, best = rounds_of(be, scan, args.window, args.rounds)
        want = (n, 0, n - 1) if fill[0] else (0, n, n)
        assert all((out[0][r], out[1][r], out[2][r]) == want for r in range(ROWS)), 'the scan is wrong'
        rates[label] = nbytes / med / 1e9
        lines.append(f'| gs_nonzero_spans, {label} | {med * 1e3:.3f} ({best * 1e3:.3f}) | {nbytes / med / 1e9:.0f} ({nbytes / best / 1e9:.0f}) | the same |')
    med, best = rounds_of(be, copy, args.window, args.rounds)
    rates['copy'] = 2 * nbytes / med / 1e9
    lines.append(f'| gs_copy | {med * 1e3:.3f} ({best * 1e3:.3f}) | {nbytes / med / 1e9:.0f} ({nbytes / best / 1e9:.0f}) | {2 * nbytes / med / 1e9:.0f} ({2 * nbytes / best / 1e9:.0f}) |')
    be.free(src)
    be.free(dst)
    lines += ['', f'The scan moves {min(rates["dense non-zero"], rates["all zero"]) / rates["copy"]:.2f} of the traffic rate of the copy '
                  f'({min(rates["dense non-zero"], rates["all zero"]):.0f} against {rates["copy"]:.0f} GB/s).', '']

    from generic_cases import POSEIDON_OPTS, build
    lines += ['## diagnose next to prove', '', 'One call each on one context, interpreted AIR programs (the mode a context has when no code object is cached).', '',
              '| statement | prove ms | diagnose ms |', '|---|---|---|']
    for name in ('poseidon_seg_256', 'poseidon_c4_65536'):
        air, _stark, seed, assertions = build(name, be)
        p = Prover(air, POSEIDON_OPTS)
        packed = p.pack_seed(seed)
        pm, pb = wall(lambda: p.prove_bytes(assertions, None, packed), args.window, args.rounds)
        d = p.diagnose(assertions, None, packed)
        assert d.ok, str(d)
        dm, db = wall(lambda: p.diagnose(assertions, None, packed), args.window, args.rounds)
        lines.append(f'| {name} | {pm * 1e3:.2f} ({pb * 1e3:.2f}) | {dm * 1e3:.2f} ({db * 1e3:.2f}) |')
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text)
    print(text)


if __name__ == '__main__':
    main()
