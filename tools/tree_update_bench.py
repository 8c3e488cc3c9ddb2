"""tools/tree_update_bench.py [--out profiles/tree_update.md] [--detail bench_detail.json] — batched updates of a device Merkle tree on
the MI355X (include/gstark_tree_update.h), written as a profile.

  tree          lib128's Poseidon tree (width 6, nodes of two elements, x^5, 8 + 55 rounds) over 2^20 leaves
  updates       gs_hades_merkle_update at k = 1, 2^6, 2^10, 2^14, 2^18 random leaves per call: time per call, per update and per level
  rebuild       one gs_hades_merkle of the same tree, leaves in place: what a changed leaf cost before
  product roof  k * log2 n permutations x products per permutation x the per-product issue cost of the `second_roof` table of
                bench_detail.json (as tools/hades_bench.py uses it), spread over the chip's 1 024 SIMDs
  host plan     tree_update_plan_build alone (csrc/tree_update_plan.h compiled into a helper library here), apart from the device time;
                "in the entry" is the host clock from the call to its return: the plan, the uploads and the enqueues

Times are host clock around `reps` back-to-back calls that end in one gs_sync, after a warm-up of the same shape; every window is at
least --window seconds long.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from genstark_amd import lib128                         # noqa: E402
from genstark_amd._abi import Backend                  # noqa: E402
from genstark_amd.field import Matrix, PrimeField      # noqa: E402
from hades_bench import OCCUPANCY, products            # noqa: E402
from sponge_bench import LANES, SIMDS, product_cost, timed      # noqa: E402

PLAN_HELPER = '''#include "%s"
extern "C" unsigned long long plan_once(unsigned long long n, const unsigned long long *indexes, unsigned long long count) {
    tree_update_plan plan;
    tree_update_plan_build(n, (const uint64_t *)indexes, count, plan);
    return plan.last.size() + plan.pred.size();
}
'''


def plan_library(tmp):
    src, so = os.path.join(tmp, 'plan.cpp'), os.path.join(tmp, 'plan.so')
    open(src, 'w').write(PLAN_HELPER % os.path.join(ROOT, 'genstark_amd', 'csrc', 'tree_update_plan.h'))
    subprocess.check_call(['g++', '-O3', '-std=c++17', '-shared', '-fPIC', src, '-o', so])
    lib = C.CDLL(so)
    lib.plan_once.restype, lib.plan_once.argtypes = C.c_uint64, [C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tree_update.md'))
    ap.add_argument('--detail', default=os.path.join(ROOT, 'bench_detail.json'))
    ap.add_argument('--window', type=float, default=0.25)
    ap.add_argument('--log-leaves', type=int, default=20)
    args = ap.parse_args()
    cost, cost_from = product_cost(args.detail)
    be = Backend(device=0)
    f = PrimeField(backend=be)
    h = lib128.poseidon_tree(f, [(0, 0), (0, 0)]).hash
    per, digest, depth, n = products(h), 2, args.log_leaves, 1 << args.log_leaves
    ns = cost[min(OCCUPANCY[('p128', 6)], 4) - 1] if cost else None
    roof = (lambda count: count * per * ns * 1e-9 / (LANES * SIMDS)) if ns else (lambda count: None)
    es = f.elementSize
    series = f.getPowerSeries(3, 2 * n * digest)        # leaves and new leaves made on the device: distinct non-trivial elements
    nodes = Matrix(be, 2 * n, digest)
    be.call('gs_copy', C.c_void_p(nodes.ptr + n * digest * es), C.c_void_p(series.ptr), n * digest * es)
    build = lambda: be.call('gs_hades_merkle', h.handle(), C.c_void_p(nodes.ptr + n * digest * es), n, digest, C.c_void_p(nodes.ptr))
    t_build, reps_build = timed(be, build, args.window)
    lines = ['# Batched updates of a device Merkle tree (tools/tree_update_bench.py)', '',
             f'lib128\'s Poseidon tree: width 6, nodes of two elements, x^5, 8 + 55 rounds = {per} products per permutation; 2^{depth} leaves.',
             'Time per call: host clock around back-to-back calls ending in one synchronise, after a warm-up; random indexes, new leaves already on the device.',
             f'Product roof: k x {depth} permutations at the per-product cost from `{cost_from}` (`second_roof`, canonical 128-bit product) / 64 lanes / 1 024 SIMDs.'
             if ns else 'Product roof: no `second_roof` table was found: no fractions.', '',
             f'One rebuild of the tree (`gs_hades_merkle`, {n - 1} permutations, leaves in place): {t_build * 1e3:.3f} ms ({reps_build} reps)'
             + (f', {roof(n - 1) / t_build:.3f} of its product roof.' if ns else '.'), '',
             '| updates per call | reps | ms per call | us per update | ms per level | rebuilds it replaces (k x rebuild / call) | fraction of product roof | host: plan alone, ms | host: in the entry, ms |',
             '|---|---|---|---|---|---|---|---|---|']
    rng = random.Random(20)
    with tempfile.TemporaryDirectory() as tmp:
        plan = plan_library(tmp)
        for log in (0, 6, 10, 14, 18):
            k = 1 << log
            indexes = (C.c_uint64 * k)(*[rng.randrange(n) for _ in range(k)])
            leaves = C.c_void_p(series.ptr + n * digest * es)
            before, roots = Matrix(be, k * (depth + 1), digest), Matrix(be, k, digest)
            in_entry = [0.0, 0]

            def update():
                t0 = time.perf_counter()
                be.call('gs_hades_merkle_update', h.handle(), C.c_void_p(nodes.ptr), n, digest, indexes, leaves, k, C.c_void_p(before.ptr), C.c_void_p(roots.ptr))
                in_entry[0] += time.perf_counter() - t0
                in_entry[1] += 1
            t, reps = timed(be, update, args.window)
            t0 = time.perf_counter()
            plan_reps = max(3, min(1000, int(0.05 / max(t, 1e-6))))
            for _ in range(plan_reps):
                plan.plan_once(n, indexes, k)
            t_plan = (time.perf_counter() - t0) / plan_reps
            frac = f'{roof(k * depth) / t:.4f}' if ns else 'n/a'
            lines.append(f'| 2^{log} | {reps} | {t * 1e3:.3f} | {t / k * 1e6:.2f} | {t / depth * 1e3:.4f} | {k * t_build / t:.1f} | {frac} | {t_plan * 1e3:.4f} | {in_entry[0] / in_entry[1] * 1e3:.4f} |')
    lines += ['', 'A call of few updates is `log2 n` dependent launches of one or a few waves each: every level costs one thread-per-permutation Hades',
              'permutation whatever the batch holds ("ms per level" at k = 1), so a single update of a deep tree is latency-bound; the batches are where',
              'the work is paid at throughput.  Follow-up, not done here: a lane-per-element form of the Hades permutation for narrow launches (what',
              '`k_rescue_spread` is for Rescue) would shorten the per-level time.', '']
    be.close()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, 'w').write(text)
    print(text)


if __name__ == '__main__':
    main()
