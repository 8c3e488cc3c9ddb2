"""tools/verify_device_bench.py [quick] — gs_prover_verify against gs_prover_verify_device on the same proofs (profiles/verify_device.md):
  1. the two-register quintic AIR, m assertions on register 0, T = 2^13 and 2^16;
  2. Rescue 4x128, 2^16 steps: 4 x 4 096 assertions, and its 2-assertion form (nothing is large: the two entries run the same code);
  3. the ledger component with a public input register of 256 .. 16 384 values (T = 2 x that).
The job is packed once; what is timed is the driver's entry alone.  The device column has the providers FORCED (gs_prover_verify_device_min(1, 1)):
the thresholds are where it first beats the host column.  Warm, one process, median of the repetitions and min..max, ms."""
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


def both(nat, assertions, blob, public=None, reps=9):
    """'host | device forced | device at the default thresholds'"""
    job, keep = nat._verify_job(assertions, public)
    err = C.create_string_buffer(512)

    def host():
        assert nat.lib.gs_prover_verify_on(nat.binding, C.byref(job), blob, len(blob), err, 512) == 0, err.value

    def device():
        assert nat.lib.gs_prover_verify_device_on(nat.binding, nat.backend.ctx, C.byref(job), blob, len(blob), err, 512) == 0, err.value
    out = [timed(host, reps)]
    nat.verify_device_min(1, 1)
    out.append(timed(device, reps))
    nat.verify_device_min(0, 0)
    out.append(timed(device, reps))
    return ' | '.join(out)


if __name__ == '__main__':
    quick = 'quick' in sys.argv
    be = Backend(device=0)
    be.jit()
    f = PrimeField(backend=be)
    p = f.modulus
    rng = random.Random(7)
    print('columns: host entry | device entry, providers forced | device entry, default thresholds; ms, median (min..max)', flush=True)
    print('## 1. quintic AIR, m assertions on register 0', flush=True)
    for log_t in (13,) if quick else (13, 16):
        T = 1 << log_t
        rows = quintic_trace(p, T, [5, 9])
        nat = NativeProver(Statement(quintic_air(f, T)))
        for m in (64, 128, 256, 1024, 4096):
            a = [{'step': s, 'register': 0, 'value': rows[s][0]} for s in rng.sample(range(T), m)]
            blob = nat.prove_bytes(a, [], [5, 9])
            print(f'T = 2^{log_t}, m = {m}: {both(nat, a, blob, reps=9 if m <= 1024 else 5)}', flush=True)
    print('## 2. Rescue 4x128, 2^16 steps, 2048 chains', flush=True)
    air, a, seeds = rescue_statement(f, 2048)
    nat = NativeProver(Statement(air, dict(OPTS, exeQueryCount=68, friQueryCount=24)))
    packed = nat.pack_seed(seeds)
    few = [a[3], a[-1]]
    print('4 x 4096 assertions: prove', timed(lambda: nat.prove_bytes(a, [], packed), 5), flush=True)
    print('4 x 4096 assertions: verify', both(nat, a, nat.prove_bytes(a, [], packed), reps=5), flush=True)
    print('2 assertions: verify', both(nat, few, nat.prove_bytes(few, [], packed), reps=15), flush=True)
    print('## 3. ledger.aa, `runs` runs of 4 public deposits: a public column of 8 x runs steps', flush=True)
    from genstark_amd import airassembly
    from genstark_amd.prover import Prover
    from test_airassembly import AA, ledger_model
    air = airassembly.AssemblyAir(open(os.path.join(AA, 'ledger.aa')).read(), 'default', None, f)
    nat = Prover(air, {'hashAlgorithm': 'sha256', 'exeQueryCount': 68, 'friQueryCount': 24})._native
    for runs in (64, 512) if quick else (64, 128, 256, 512, 1024, 4096):
        balances, factors = [100 + 7 * i for i in range(runs)], [3 + i for i in range(runs)]
        deposits = [[5 + i + 2 * j for j in range(4)] for i in range(runs)]
        model = ledger_model(p, balances, factors, deposits)
        last = 8 * runs - 1
        a = [{'step': 0, 'register': 0, 'value': balances[0]}, {'step': last, 'register': 2, 'value': model[last][2]}]
        blob = nat.prove_bytes(a, [balances, factors, deposits], None)
        print(f'runs = {runs} (column of {8 * runs} steps, {4 * runs} public values): {both(nat, a, blob, [deposits])}', flush=True)
