"""tests/golden/make_curve_products.py — what tests/test_curve.py compares the device's multiplications on the 224-bit curve against,
computed ONCE by the control `genstark_amd.pointmul.ec_multiply` (Python integers, two Fermat inversions per bit: 40 ms a product,
minutes for the batch — too long to repeat in every run of the suite); writes tests/golden/curve224_products.json.

The rows come from a seed (rows()): 1000 scalars — the seam scalars first, random 256-bit after — and 1000 random multipliers r below n.
Recorded per count of COUNTS, as the SHA-256 of the first `count` results (digest()):

    points      ec_multiply(G, r): the random points of the variable-base rows
    fixed       ec_multiply(G, scalar): what the fixed-base rows must give
    variable    ec_multiply(point, scalar): what the variable-base rows must give

    python tests/golden/make_curve_products.py

tests/test_curve.py recomputes the digests of the smallest counts with ec_multiply in the CPU tier."""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

ROWS = 1000
COUNTS = (1, 16, 63, 64, 65, 255, 256, 257, 1000)      # 16: the sample the CPU tier recomputes; the rest: the seams of the GPU test


def seam_scalars(n):
    return [0, 1, 2, n - 2, n - 1, n, n + 1, n + 2, 2 * n, 2 * n + 1, 1 << 224, 1 << 255, (1 << 256) - 1]


def rows(n):
    """(scalars, multipliers)"""
    rng = random.Random(0xEC224)
    scalars = seam_scalars(n)
    scalars += [rng.getrandbits(256) for _ in range(ROWS - len(scalars))]
    return scalars, [rng.randrange(1, n) for _ in range(ROWS)]


def digest(points):
    """points: (x, y) or None (infinity)"""
    return hashlib.sha256('\n'.join('inf' if pt is None else f'{pt[0]:x},{pt[1]:x}' for pt in points).encode()).hexdigest()


if __name__ == '__main__':
    from genstark_amd._abi import MODULUS_224 as P
    from genstark_amd.curve import G_224, ORDER_224
    from genstark_amd.pointmul import ec_multiply
    scalars, multipliers = rows(ORDER_224)
    lists = {'points': [ec_multiply(P, G_224, r) for r in multipliers], 'fixed': [ec_multiply(P, G_224, k) for k in scalars]}
    lists['variable'] = [ec_multiply(P, pt, k) for pt, k in zip(lists['points'], scalars)]
    with open(os.path.join(HERE, 'curve224_products.json'), 'w') as fh:
        json.dump({name: {str(count): digest(values[:count]) for count in COUNTS} for name, values in lists.items()}, fh, indent=1)
        fh.write('\n')
