"""tools/sparse_tree_bench.py [--out profiles/sparse_tree.md] [--detail bench_detail.json] — batched updates and paths of a sparse device
Merkle tree on the MI355X (include/gstark_sparse_tree.h), written as a profile.

  tree          lib128's Poseidon tree (width 6, nodes of two elements, x^5, 8 + 55 rounds), depth 32, 2^20 stored leaves at random keys
  updates       gs_sparse_update at k = 1, 2^6, 2^10, 2^14, 2^18 random keys per call: time per call, per update and per level.  The keys
                of a call are drawn once: the warm-up stores them, the timed calls update stored keys
  paths         gs_sparse_paths at the same k, keys drawn from the whole key space (mostly non-membership paths)
  dense         gs_hades_merkle_update on a dense tree of 2^20 leaves at the same k: what the slot gather and commit are compared with
  hash alone    one gs_hades_hash launch over k rows of four elements: a level without its gather; (level - hash) / level is the share of
                the gather and, spread over the levels, of the commit
  product roof  k * depth permutations x products per permutation x the per-product issue cost of the `second_roof` table of
                bench_detail.json (as tools/hades_bench.py uses it), spread over the chip's 1 024 SIMDs
  host          sparse_plan_update / sparse_plan_paths alone on an index of the same 2^20 keys (csrc/sparse_tree_plan.h compiled into a
                helper library here), apart from the device time; "in the entry" is the host clock from the call to its return, over the timed calls only

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
static sparse_tree_index *tree;
extern "C" unsigned long long plan_fill(unsigned depth, const unsigned long long *indexes, unsigned long long count) {
    tree = new sparse_tree_index(depth);
    sparse_update_plan plan;
    if (!sparse_plan_update(*tree, (const uint64_t *)indexes, count, plan)) return 0;
    sparse_plan_commit(*tree, plan);
    return tree->slots;
}
extern "C" void plan_store(const unsigned long long *indexes, unsigned long long count) {       // what the warm-up call does to the index
    sparse_update_plan plan;
    if (sparse_plan_update(*tree, (const uint64_t *)indexes, count, plan)) sparse_plan_commit(*tree, plan);
}
extern "C" unsigned long long plan_once(const unsigned long long *indexes, unsigned long long count) {
    sparse_update_plan plan;
    sparse_plan_update(*tree, (const uint64_t *)indexes, count, plan);
    return sparse_plan_update_in_bounds(plan) ? plan.slots_after : 0;
}
extern "C" unsigned long long paths_once(const unsigned long long *indexes, unsigned long long count) {
    std::vector<uint32_t> slots;
    sparse_plan_paths(*tree, (const uint64_t *)indexes, count, slots);
    return sparse_plan_slots_below(slots, tree->slots) ? slots.size() : 0;
}
'''


def plan_library(tmp):
    src, so = os.path.join(tmp, 'plan.cpp'), os.path.join(tmp, 'plan.so')
    open(src, 'w').write(PLAN_HELPER % os.path.join(ROOT, 'genstark_amd', 'csrc', 'sparse_tree_plan.h'))
    subprocess.check_call(['g++', '-O3', '-std=c++17', '-shared', '-fPIC', src, '-o', so])
    lib = C.CDLL(so)
    lib.plan_fill.restype, lib.plan_fill.argtypes = C.c_uint64, [C.c_uint32, C.POINTER(C.c_uint64), C.c_uint64]
    lib.plan_store.restype, lib.plan_store.argtypes = None, [C.POINTER(C.c_uint64), C.c_uint64]
    for fn in (lib.plan_once, lib.paths_once):
        fn.restype, fn.argtypes = C.c_uint64, [C.POINTER(C.c_uint64), C.c_uint64]
    return lib


def host_time(call, device_time):
    reps = max(3, min(1000, int(0.05 / max(device_time, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sparse_tree.md'))
    ap.add_argument('--detail', default=os.path.join(ROOT, 'bench_detail.json'))
    ap.add_argument('--window', type=float, default=0.25)
    ap.add_argument('--depth', type=int, default=32)
    ap.add_argument('--log-stored', type=int, default=20)
    args = ap.parse_args()
    cost, cost_from = product_cost(args.detail)
    be = Backend(device=0)
    f = PrimeField(backend=be)
    depth, stored, digest, dense_depth = args.depth, 1 << args.log_stored, 2, 20
    sparse = lib128.poseidon_sparse_tree(f, depth, slots_hint=1 << 20)
    h, per = sparse.hash, products(sparse.hash)
    ns = cost[min(OCCUPANCY[('p128', 6)], 4) - 1] if cost else None
    roof = (lambda count: count * per * ns * 1e-9 / (LANES * SIMDS)) if ns else (lambda count: None)
    es, top = f.elementSize, 1 << 18
    series = f.getPowerSeries(3, (stored + top) * digest)            # leaves made on the device: distinct non-trivial elements
    rng = random.Random(32)
    keys = [rng.randrange(1 << depth) for _ in range(stored)]
    key_array = (C.c_uint64 * stored)(*keys)
    before, roots = Matrix(be, stored, (depth + 1) * digest), Matrix(be, stored, digest)
    t0 = time.perf_counter()
    be.call('gs_sparse_update', sparse._tree, key_array, C.c_void_p(series.ptr), stored, C.c_void_p(before.ptr), C.c_void_p(roots.ptr))
    be.sync()
    t_fill, nodes_stored = time.perf_counter() - t0, sum(sparse.stored)
    dense_n = 1 << dense_depth
    dense = Matrix(be, 2 * dense_n, digest)
    be.call('gs_hades_merkle', h.handle(), C.c_void_p(series.ptr), dense_n, digest, C.c_void_p(dense.ptr))
    new = C.c_void_p(series.ptr + stored * digest * es)
    lines = ['# Sparse device Merkle trees: batched updates and paths (tools/sparse_tree_bench.py)', '',
             f'lib128\'s Poseidon tree: width 6, nodes of two elements, x^5, 8 + 55 rounds = {per} products per permutation; depth {depth}, 2^{args.log_stored} stored leaves at',
             f'random keys = {nodes_stored} stored nodes ({nodes_stored / stored:.2f} per leaf, {nodes_stored * digest * es / 2**20:.0f} MiB of store).  Filling the tree, ONE call of 2^{args.log_stored} updates, first use of',
             f'every buffer included: {t_fill * 1e3:.1f} ms.',
             'Time per call: host clock around back-to-back calls ending in one synchronise, after a warm-up that stores the call\'s keys; random keys, new leaves already on the device.',
             f'Product roof: k x {depth} permutations at the per-product cost from `{cost_from}` (`second_roof`, canonical 128-bit product) / 64 lanes / 1 024 SIMDs.'
             if ns else 'Product roof: no `second_roof` table was found: no fractions.', '',
             f'## `gs_sparse_update`, depth {depth}, beside `gs_hades_merkle_update`, depth {dense_depth}', '',
             '| updates per call | reps | ms per call | us per update | ms per level | fraction of product roof | dense: ms per call | dense: ms per level | hash launch alone, ms | gather + commit share of a level | host: plan alone, ms | host: in the entry, ms |',
             '|---|---|---|---|---|---|---|---|---|---|---|---|']
    path_lines = ['', f'## `gs_sparse_paths`, depth {depth}', '', '| paths per call | reps | ms per call | us per path | host: slots alone, ms | host: in the entry, ms |', '|---|---|---|---|---|---|']
    shares, host_bound = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        plan = plan_library(tmp)
        assert plan.plan_fill(depth, key_array, stored) == nodes_stored
        for log in (0, 6, 10, 14, 18):
            k = 1 << log
            indexes = (C.c_uint64 * k)(*[rng.randrange(1 << depth) for _ in range(k)])
            dense_indexes = (C.c_uint64 * k)(*[rng.randrange(dense_n) for _ in range(k)])
            in_entry = []                                                # one sample per call; the last `reps` are the measured window's

            def update():
                t0 = time.perf_counter()
                be.call('gs_sparse_update', sparse._tree, indexes, new, k, C.c_void_p(before.ptr), C.c_void_p(roots.ptr))
                in_entry.append(time.perf_counter() - t0)
            t, reps = timed(be, update, args.window)
            t_entry = sum(in_entry[-reps:]) / reps                       # (the warm-up calls store the keys and grow the store: not counted)
            plan.plan_store(indexes, k)                                  # the helper's index follows the device tree's: the keys are stored now
            t_plan = host_time(lambda: plan.plan_once(indexes, k), t)
            t_dense, _ = timed(be, lambda: be.call('gs_hades_merkle_update', h.handle(), C.c_void_p(dense.ptr), dense_n, digest, dense_indexes, new, k,
                                                   C.c_void_p(before.ptr), C.c_void_p(roots.ptr)), args.window)
            t_hash, _ = timed(be, lambda: be.call('gs_hades_hash', h.handle(), C.c_void_p(series.ptr), k, 2 * digest, digest, C.c_void_p(roots.ptr)), args.window)
            shares[log] = share = 1 - t_hash / (t / depth)
            if t_entry > 0.5 * t:
                host_bound.append(f'2^{log}')
            frac = f'{roof(k * depth) / t:.4f}' if ns else 'n/a'
            lines.append(f'| 2^{log} | {reps} | {t * 1e3:.3f} | {t / k * 1e6:.2f} | {t / depth * 1e3:.4f} | {frac} | {t_dense * 1e3:.3f} | {t_dense / dense_depth * 1e3:.4f} | {t_hash * 1e3:.4f} | '
                         f'{share:.3f} | {t_plan * 1e3:.4f} | {t_entry * 1e3:.4f} |')
            in_paths = []

            def paths():
                t0 = time.perf_counter()
                be.call('gs_sparse_paths', sparse._tree, indexes, k, C.c_void_p(before.ptr))
                in_paths.append(time.perf_counter() - t0)
            t, reps = timed(be, paths, args.window)
            t_slots = host_time(lambda: plan.paths_once(indexes, k), t)
            path_lines.append(f'| 2^{log} | {reps} | {t * 1e3:.3f} | {t / k * 1e6:.3f} | {t_slots * 1e3:.4f} | {sum(in_paths[-reps:]) / reps * 1e3:.4f} |')
    lines += path_lines
    lines += ['', '"ms per call" contains the host plan: the entry returns when every launch is enqueued, and the plan runs before the first of them.  "gather + commit',
              'share of a level" is 1 - (hash launch alone) / (ms per level): at small k it also holds the launch gaps between a level\'s two kernels.']
    if host_bound:
        lines += [f'At k = {", ".join(host_bound)} the host holds the call for more than half of its time ("host: in the entry" against "ms per call"): the plan of',
                  '`tree_update_plan.h`, a hash-map probe per level and update on top of it, and the upload of six plan arrays all precede the first launch, and the',
                  'device waits for them.']
    if shares.get(14, 0) > 0.2:
        lines += [f'At k = 2^14 that share is {shares[14]:.2f}, above a fifth: compare "host: plan alone" and "host: in the entry" with "ms per call" in that row — what is not the',
                  'hash launches is the host resolving slots (a hash-map probe per level and update) and uploading six plan arrays before the first launch, not the two',
                  'kernels, which move 5 elements per update and level.']
    lines += ['', 'A call of few updates is `depth` dependent launches of one or a few waves each, as for the dense tree (`profiles/tree_update.md`): a single update of a',
              'deep tree is latency-bound; the batches are where the work is paid at throughput.  Follow-up, not done here: a lane-per-element form of the Hades',
              'permutation for narrow launches (what `k_rescue_spread` is for Rescue) would shorten the per-level time.', '']
    del sparse
    be.close()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, 'w').write(text)
    print(text)


if __name__ == '__main__':
    main()
