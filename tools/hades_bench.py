"""tools/hades_bench.py [--out profiles/hades.md] [--detail bench_detail.json] — Poseidon permutations and trees on the MI355X
(include/gstark_hades.h), written as a profile.

  permutations/s   width 6 over the 128-bit field and width 3 over the 224-bit field (x^5, 8 + 55 rounds: lib128 / lib224), 2^10 .. 2^20
                   hashes per launch
  tree             2^20 leaves: the whole build, and the one-workgroup top launch alone (a tree of 2 * top leaves already in place);
                   the wide levels are the difference
  host             HadesHash.hash on Python integers, 2^10 hashes, same machine
  product roof     products per permutation x the per-product issue cost of the `second_roof` table of bench_detail.json (bench.py
                   writes it: ns per wave-wide product at 1 .. 4 waves per SIMD, registers only), spread over the chip's 1 024 SIMDs;
                   the fraction is roof time / measured time.  The table measures the 128-bit product only: the 224-bit rows carry no
                   fraction.

Times are host clock around `reps` back-to-back launches that end in one gs_sync, after a warm-up of the same shape; every window is at
least --window seconds long.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from genstark_amd import _abi, lib128, lib224          # noqa: E402
from genstark_amd._abi import Backend                  # noqa: E402
from genstark_amd.field import Matrix, PrimeField      # noqa: E402
from sponge_bench import LANES, SIMDS, product_cost, timed      # noqa: E402

# waves per SIMD of the kernels timed here, from -Rpass-analysis=kernel-resource-usage
OCCUPANCY = {('p128', 6): 4, ('p224', 3): 3}


def products(h):
    per_pow = sum(1 + (e & 1) for e in iter_bits(h.alpha))
    w = h.width
    return h.fullRounds * (w * per_pow + w * w) + h.partialRounds * (per_pow + w * w)


def iter_bits(e):
    while e > 1:
        yield e
        e >>= 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hades.md'))
    ap.add_argument('--detail', default=os.path.join(ROOT, 'bench_detail.json'))
    ap.add_argument('--window', type=float, default=0.25)
    args = ap.parse_args()
    cost, cost_from = product_cost(args.detail)
    lines = ['# Poseidon permutations and trees on the device (tools/hades_bench.py)', '',
             'x^5, 8 full + 55 partial rounds.  Time per launch: host clock around back-to-back launches ending in one synchronise, after a warm-up.',
             f'Product roof: per-product cost from `{cost_from}` (`second_roof`, canonical 128-bit product, ns per wave at the kernel\'s waves per SIMD) / 64 lanes / 1 024 SIMDs.'
             if cost else 'Product roof: no `second_roof` table was found: no fractions.', '']
    for name, lib, modulus, width, arity, digest in (('p128', lib128, None, 6, 4, 2), ('p224', lib224, _abi.MODULUS_224, 3, 2, 1)):
        be = Backend(device=0, modulus=modulus)
        f = PrimeField(backend=be)
        h = lib.poseidon_tree(f, [0, 0] if digest == 1 else [(0, 0), (0, 0)]).hash
        per = products(h)
        occ = OCCUPANCY[(name, width)]
        ns = cost[min(occ, 4) - 1] if cost and name == 'p128' else None
        roof = (lambda count: count * per * ns * 1e-9 / (LANES * SIMDS)) if ns else (lambda count: None)
        frac = lambda count, t: f'{roof(count) / t:.3f}' if ns else 'n/a'
        lines += [f'## {name}: width {width}, {per} products per permutation, {occ} waves per SIMD', '',
                  '| hashes | reps | ms per launch | M permutations/s | G products/s | fraction of product roof |', '|---|---|---|---|---|---|']
        series = f.getPowerSeries(3, (1 << 20) * arity)                 # inputs made on the device: distinct non-trivial elements
        src = Matrix(be, 1 << 20, arity, owner=series._owner)
        out = Matrix(be, 1 << 20, digest)
        for log in range(10, 21, 2):
            count = 1 << log
            t, reps = timed(be, lambda: be.call('gs_hades_hash', h.handle(), C.c_void_p(src.ptr), count, arity, digest, C.c_void_p(out.ptr)), args.window)
            lines.append(f'| 2^{log} | {reps} | {t * 1e3:.4f} | {count / t / 1e6:.2f} | {count * per / t / 1e9:.1f} | {frac(count, t)} |')
        # the tree: leaves in place (no copy in the timed window)
        n, top = 1 << 20, be.lib.gs_hades_merkle_top()
        nodes = Matrix(be, 2 * n, digest)
        be.call('gs_copy', C.c_void_p(nodes.ptr + n * digest * f.elementSize), C.c_void_p(src.ptr), n * digest * f.elementSize)
        build = lambda m: be.call('gs_hades_merkle', h.handle(), C.c_void_p(nodes.ptr + m * digest * f.elementSize), m, digest, C.c_void_p(nodes.ptr))
        t_all, reps_all = timed(be, lambda: build(n), args.window)
        t_top, reps_top = timed(be, lambda: build(2 * top), args.window)     # (overwrites nodes 0 .. 4 top - 1 with another small tree: timing only)
        wide = n - 2 * top
        lines += ['', f'Tree of 2^20 leaves of {digest} element(s) ({n - 1} permutations; levels above {top} nodes are one launch each, the rest one workgroup):', '',
                  '| part | reps | ms | fraction of product roof |', '|---|---|---|---|',
                  f'| whole build | {reps_all} | {t_all * 1e3:.3f} | {frac(n - 1, t_all)} |',
                  f'| top launch alone ({2 * top - 1} permutations, one workgroup, {top.bit_length()} dependent levels) | {reps_top} | {t_top * 1e3:.3f} | not a throughput kernel |',
                  f'| wide levels (difference, {wide} permutations) | | {(t_all - t_top) * 1e3:.3f} | {frac(wide, t_all - t_top)} |', '']
        rows = [[pow(3, i * arity + j, f.modulus) for j in range(arity)] for i in range(1 << 10)]
        t0 = time.perf_counter()
        for r in rows:
            h.hash(r)
        host = time.perf_counter() - t0
        lines += [f'Host integers (HadesHash.hash, Python, one core): 2^10 hashes in {host * 1e3:.1f} ms = {1024 / host / 1e3:.2f} k permutations/s.', '']
        be.close()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, 'w').write(text)
    print(text)


if __name__ == '__main__':
    main()
