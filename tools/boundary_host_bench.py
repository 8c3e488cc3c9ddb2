"""tools/boundary_host_bench.py — the verifier's two forms of the boundary values (csrc/verifier.h: boundary_values_direct /
boundary_values_tree) on one host core, 128 queried points, T = 2^13: milliseconds per register by assertion count.  No GPU needed."""
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from boundary_common import host_driver, root_of_unity      # noqa: E402
from genstark_amd import _abi                                             # noqa: E402

if __name__ == '__main__':
    p, T, E = _abi.MODULUS_128, 1 << 13, 16
    nat = host_driver(p)
    omega = root_of_unity(p, T * E)
    rng = random.Random(1)
    points = [pow(omega, rng.randrange(T) * E + 1, p) for _ in range(128)]
    print('m, direct ms, tree ms')
    for m in (4, 8, 16, 24, 32, 48, 64, 128, 256, 1024, 4096):
        at, ys = rng.sample(range(T), m), [rng.randrange(p) for _ in range(m)]
        row = []
        for method in (0, 1):
            best = 1e9
            for _ in range(5 if m <= 256 else 2):
                t = time.perf_counter()
                nat.boundary_at(omega, T * E, T, at, ys, points, method)
                best = min(best, time.perf_counter() - t)
            row.append(best * 1e3)
        print(f'{m}, {row[0]:.3f}, {row[1]:.3f}')
