"""tools/tree_verify_bench.py [--out profiles/tree_verify.md] [--resources FILE] — the roots that batches of Merkle paths imply on the
MI355X (include/gstark_tree_verify.h), written as a profile.

  trees         lib128's Poseidon tree (width 6, nodes of two elements, x^5, 8 + 55 rounds) and the Rescue 4 x 128 tree (x^3 and its
                inverse, 32 rounds, nodes of one element), 2^20 leaves each: depth 20
  fused         gs_hades_merkle_path_roots / gs_rescue_merkle_path_roots at 1, 2^6, 2^10, 2^14, 2^18, 2^20 paths per call, the paths
                gathered on the device from random indexes: time per call, per path and per permutation
  hashMany      the family's own gs_*_hash over the same number of permutations (count x depth rows of two nodes) in the same process:
                the rate the walk is held against
  per level     the only device route without the entries, driven from Python: per level one upload of the rows (the running node and
                the sibling side by side, assembled with numpy from the paths read back once, which is not timed), one hashMany, one
                read-back of the nodes.  Its last level must equal the fused roots, and both the tree's root: the tool asserts it.
  resources     --resources FILE: the compiler's resource usage of the two kernels (the kernel-resource-usage remarks of a build of
                hades.hip / rescue.hip with -Rpass-analysis=kernel-resource-usage), copied into the profile as it stands

Times are host clock around `reps` back-to-back calls that end in one gs_sync, after a warm-up of the same shape; every window is at
least --window seconds long (the per-level route: one run after one warm-up run up to 2^10 paths, one run above).  Needs the GPU: there is
no fallback."""
import argparse
import ctypes as C
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from genstark_amd import lib128                          # noqa: E402
from genstark_amd._abi import Backend                   # noqa: E402
from genstark_amd.field import Matrix, PrimeField, Vector      # noqa: E402
from genstark_amd.rescue_hash import RescueMerkleTree, rescue4x128      # noqa: E402
from hades_bench import products                        # noqa: E402
from sponge_bench import timed                          # noqa: E402

LOGS = (0, 6, 10, 14, 18, 20)


def per_level(be, h, hash_many, paths, indexes, depth, digest):
    """the composition a caller without the entries is left with; -> (seconds, the last level's nodes as bytes)"""
    count, nb = len(indexes), digest * be.element_size
    walk = np.frombuffer(paths.toBuffer(), dtype=np.uint8).reshape(count, depth + 1, nb)       # (read back once, before the clock starts)
    idx = np.array(indexes, dtype=np.uint64)
    t0 = time.perf_counter()
    node = walk[:, 0, :]
    for l in range(depth):
        right = ((idx >> np.uint64(l)) & np.uint64(1)).astype(bool)[:, None]
        sibling = walk[:, l + 1, :]
        rows = np.where(right, np.concatenate([sibling, node], axis=1), np.concatenate([node, sibling], axis=1))
        m = Matrix(be, count, 2 * digest)
        be.upload(m.ptr, rows.tobytes())
        node = np.frombuffer(hash_many(m).toBuffer(), dtype=np.uint8).reshape(count, nb)
    return time.perf_counter() - t0, node.tobytes()


def family(be, f, name, tree, entry, digest_args, hash_launch, hash_many, products, window, lines):
    h, depth, digest, n, es = tree.hash, tree.depth, tree.digest, tree.leafCount, be.element_size
    rng = random.Random(21)
    top = 1 << LOGS[-1]
    everything = [rng.randrange(n) for _ in range(top)]
    gathered = Matrix(be, top, (depth + 1) * digest)
    be.call('gs_hades_merkle_paths', C.c_void_p(tree.deviceNodes.ptr), n, digest, (C.c_uint64 * top)(*everything), top, C.c_void_p(gathered.ptr))
    root = bytes(tree.deviceNodes.row(1).toBuffer() if isinstance(tree.deviceNodes, Matrix) else tree.deviceNodes.toBuffer(1, 1))
    rows_in = Matrix(be, top * depth, 2 * digest)        # the input of the hashMany runs: the gathered nodes, twice over
    whole, once = top * depth * 2 * digest * es, top * (depth + 1) * digest * es
    be.call('gs_copy', C.c_void_p(rows_in.ptr), C.c_void_p(gathered.ptr), once)
    be.call('gs_copy', C.c_void_p(rows_in.ptr + once), C.c_void_p(gathered.ptr), whole - once)
    rows_out = Matrix(be, top * depth, digest)
    lines += [f'## {name}: {products} products per permutation, depth {depth}', '',
              '| paths per call | reps | ms per call | us per path | ns per permutation | M permutations/s fused | M permutations/s hashMany | fused / hashMany | per-level route, ms | per-level / fused |',
              '|---|---|---|---|---|---|---|---|---|---|']
    for log in LOGS:
        k = 1 << log
        indexes = everything[:k]
        c_idx = (C.c_uint64 * k)(*indexes)
        paths, roots = Matrix(be, k, gathered.colCount, owner=gathered._owner), Matrix(be, k, digest)
        fused = lambda: be.call(entry, h.handle(), C.c_void_p(paths.ptr), depth, *digest_args, c_idx, None, k, C.c_void_p(roots.ptr))
        t, reps = timed(be, fused, window)
        got = roots.toBuffer()
        assert got == root * k, f'{name}: the fused roots of 2^{log} paths are not the root'
        t_hash, _ = timed(be, lambda: hash_launch(rows_in, k * depth, rows_out), window)
        if log <= 10:
            per_level(be, h, hash_many, paths, indexes, depth, digest)
        t_level, last = per_level(be, h, hash_many, paths, indexes, depth, digest)
        assert last == got, f'{name}: the per-level route and the fused walk differ at 2^{log} paths'
        perms = k * depth
        lines.append(f'| 2^{log} | {reps} | {t * 1e3:.3f} | {t / k * 1e6:.3f} | {t / perms * 1e9:.1f} | {perms / t / 1e6:.3f} | {perms / t_hash / 1e6:.3f} | {t_hash / t:.3f} | '
                     f'{t_level * 1e3:.2f} | {t_level / t:.1f} |')
        print(lines[-1], flush=True)
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tree_verify.md'))
    ap.add_argument('--resources', default=None)
    ap.add_argument('--window', type=float, default=0.25)
    ap.add_argument('--log-leaves', type=int, default=20)
    args = ap.parse_args()
    be = Backend(device=0)
    f = PrimeField(backend=be)
    n = 1 << args.log_leaves
    lines = ['# The roots that batches of Merkle paths imply (tools/tree_verify_bench.py)', '',
             'Time per call: host clock around back-to-back calls ending in one synchronise, after a warm-up; random indexes, the paths already on the device',
             '(gathered there).  "hashMany": the family\'s own hash launch over the same number of permutations, same process.  "per-level route": what a caller',
             'without the entries is left with — per level an upload of the rows, a hashMany, a read-back — with the paths read back beforehand.', '']
    series = f.getPowerSeries(3, 2 * n)                  # leaves made on the device: distinct non-trivial elements
    poseidon = lib128.poseidon_tree(f, Matrix(be, n, 2, owner=series._owner))
    hp = poseidon.hash
    family(be, f, "Poseidon (lib128's parameters, `k_hades_path_roots<6>`)", poseidon, 'gs_hades_merkle_path_roots', (2,),
           lambda src, count, out: be.call('gs_hades_hash', hp.handle(), C.c_void_p(src.ptr), count, 4, 2, C.c_void_p(out.ptr)),
           lambda m: hp.hashMany(m, 2), products(hp), args.window, lines)
    del poseidon
    hr = rescue4x128(f)
    rescue = RescueMerkleTree(hr, Vector(be, n, owner=series._owner))
    be.traffic(True)
    hr.hashMany(Matrix(be, 1, 2, owner=series._owner), 1)
    units = [v['units'] for v in be.traffic().values()]
    be.traffic(False)
    family(be, f, 'Rescue 4 x 128 (`k_rescue_path_roots<4>`)', rescue, 'gs_rescue_merkle_path_roots', (),
           lambda src, count, out: be.call('gs_rescue_hash', hr.handle(), C.c_void_p(src.ptr), count, 2, 1, 1, 0, C.c_void_p(out.ptr)),
           lambda m: hr.hashMany(m, 1), units[0] if units else 'n/a', args.window, lines)
    if args.resources:
        lines += ['## Resource usage (the compiler\'s kernel-resource-usage remarks for gfx950)', '', open(args.resources).read().rstrip(), '']
    be.close()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, 'w').write(text)
    print(text)


if __name__ == '__main__':
    main()
