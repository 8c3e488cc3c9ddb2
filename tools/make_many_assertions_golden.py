"""tools/make_many_assertions_golden.py [out] — proves the statement of tests/golden/many_assertions_quintic_2p13.proof on the GPU: the
two-register quintic AIR, 2^13 steps, 5 000 assertions on register 0 and three on register 1
(tests/boundary_common.py: golden_statement).  The host path cannot produce it (gs_small_interpolate stops at 4 096)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from boundary_common import GOLDEN, Statement as _Statement, golden_statement, quintic_air      # noqa: E402
from genstark_amd._abi import Backend                                                            # noqa: E402
from genstark_amd.field import PrimeField                                                        # noqa: E402
from genstark_amd.native import NativeProver                                                     # noqa: E402

if __name__ == '__main__':
    f = PrimeField(backend=Backend(device=0))
    nat = NativeProver(_Statement(quintic_air(f, 1 << 13)))
    a = golden_statement(f.modulus)
    blob = nat.prove_bytes(a, [], [5, 9])
    assert nat.verify_bytes(a, blob) is True
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    open(out, 'wb').write(blob)
    print(f'{out}: {len(blob)} bytes')
