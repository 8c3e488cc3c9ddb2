"""tools/boundary_prove_bench.py [quick] — what many assertions cost on the GPU (profiles/boundary_polys.md):
  1. gs_boundary_polys alone (4 rows x 4 096 assertions, T = 2^16) by schoolbook / NTT switch-over of the product tree;
  2. whole proofs of the two-register quintic AIR, m assertions on one register, T in 2^13, 2^16, 2^20: device path vs host path
     (gs_prover_host_boundary: the path every such proof took before gs_boundary_polys existed);
  3. the Rescue statement with 4 x 4 096 assertions (and its 2-assertion form): prove, phases, native verify.
Warm, median of the repetitions, min..max as the spread."""
import ctypes as C
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from boundary_common import OPTS, Statement, quintic_air, quintic_trace, rescue_statement      # noqa: E402
from genstark_amd._abi import Backend                                                          # noqa: E402
from genstark_amd.field import PrimeField                                                      # noqa: E402
from genstark_amd.native import NativeProver                                                   # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return f'{statistics.median(ts):.3f} ({min(ts):.3f}..{max(ts):.3f})'


if __name__ == '__main__':
    be = Backend(device=0)
    be.jit()
    f = PrimeField(backend=be)
    p, es = f.modulus, f.elementSize
    rng = random.Random(7)
    print('## 1. gs_boundary_polys, 4 rows x 4096 assertions, T = 2^16, by switch-over (slot = 2^k elements), ms', flush=True)
    T, rows, m = 1 << 16, 4, 4096
    omega = f.getRootOfUnity(2 * T)
    steps = (C.c_uint64 * (rows * m))(*[s for _ in range(rows) for s in rng.sample(range(T), m)])
    vals = b''.join(f.le(rng.randrange(p)) for _ in range(rows * m))
    per_row = (C.c_uint32 * rows)(*[m] * rows)
    i_out, z_out = be.alloc(rows * m * es), be.alloc(rows * (m + 1) * es)

    def call():
        be.call('gs_boundary_polys', f.le(omega), 2 * T, T, steps, vals, per_row, rows, m, C.c_void_p(i_out), C.c_void_p(z_out))
        be.sync()
    for k in (2, 3, 4, 5, 6, 7, 8, 9, 10):
        before = be.lib.gs_boundary_schoolbook_log2(k)
        print(f'k = {k}: {timed(call, 20)}', flush=True)
        be.lib.gs_boundary_schoolbook_log2(before)
    print('## 2. quintic AIR, m assertions on register 0: prove ms, device path | host path', flush=True)
    for log_t in (13, 16) if 'quick' in sys.argv else (13, 16, 20):
        T = 1 << log_t
        rows_ = quintic_trace(p, T, [5, 9])
        nat = NativeProver(Statement(quintic_air(f, T)))
        for m in (5, 8, 16, 32, 64, 128, 256, 1024, 4096):
            a = [{'step': s, 'register': 0, 'value': rows_[s][0]} for s in rng.sample(range(T), m)]
            out = []
            for host in (False, True):
                nat.host_boundary(host)
                out.append(timed(lambda: nat.prove_bytes(a, [], [5, 9]), 9 if m <= 1024 else 3))
            nat.host_boundary(False)
            print(f'T = 2^{log_t}, m = {m}: {out[0]} | {out[1]}', flush=True)
    print('## 3. Rescue 4x128, 2^16 steps, 2048 chains', flush=True)
    air, a, seeds = rescue_statement(f, 2048)
    nat = NativeProver(Statement(air, dict(OPTS, exeQueryCount=68, friQueryCount=24)))
    packed = nat.pack_seed(seeds)
    few = [a[3], a[-1]]
    print('2 assertions: prove', timed(lambda: nat.prove_bytes(few, [], packed), 9), flush=True)
    for host in (False, True):
        nat.host_boundary(host)
        print('4 x 4096 assertions,', 'host path:' if host else 'device path:', 'prove', timed(lambda: nat.prove_bytes(a, [], packed), 9 if not host else 3), flush=True)
        print('   phases', nat.last_stats()['phases_ms'], flush=True)
    nat.host_boundary(False)
    blob = nat.prove_bytes(a, [], packed)
    print('4 x 4096 assertions: native verify', timed(lambda: nat.verify_bytes(a, blob), 5), flush=True)
    blob2 = nat.prove_bytes(few, [], packed)
    print('2 assertions: native verify', timed(lambda: nat.verify_bytes(few, blob2), 5), flush=True)
