"""tests/boundary_worker.py — child processes of tests/test_boundary_many_assertions.py.
  sanitized            under the instrumented driver (tools/build_sanitized.sh; GSTARK_PROVER_LIB_DIR): the verifier's product-tree form of
                       the boundary values on malformed assertion sets (repeated steps, a step >= T, m > T), both forms on random sets, the
                       5 000-assertion golden proof intact, with altered assertions and with corrupted bytes.  CPU only.
  runtime <q>          the runtime-modulus flavour on the GPU for ONE prime (one modulus per process): gs_boundary_polys against Python
                       integers, and a proof through the device path == the forced host path, verified."""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from boundary_common import GOLDEN, Statement, golden_statement, quintic_air, quintic_trace, root_of_unity      # noqa: E402
from genstark_amd._abi import Backend                          # noqa: E402
from genstark_amd.errors import StarkError                     # noqa: E402
from genstark_amd.field import PrimeField                      # noqa: E402
from genstark_amd.native import NativeProver                   # noqa: E402


def refused(fn, needle):
    try:
        fn()
    except StarkError as e:
        assert needle in str(e), (needle, str(e))
        return 1
    raise AssertionError(f'accepted: expected "{needle}"')


def sanitized_mode():
    from sanitizer_worker import loaded_instrumented_driver
    be = Backend(lib_path=os.path.join(ROOT, 'oracle', 'liboracle.so'), allow_test_double=True)
    f = PrimeField(backend=be)
    p = f.modulus
    n = 0
    T = 256
    nat = NativeProver(Statement(quintic_air(f, T)))
    omega = root_of_unity(p, T * 4)
    points = [pow(omega, 4 * k + 1, p) for k in range(5)]
    n += refused(lambda: nat.boundary_at(omega, T * 4, T, list(range(100)) + [7], [1] * 101, points, 1), 'asserted more than once')
    n += refused(lambda: nat.boundary_at(omega, T * 4, T, list(range(100)) + [T], [1] * 101, points, 1), 'outside of execution trace')
    n += refused(lambda: nat.boundary_at(omega, T * 4, T, list(range(100)) + [2**63], [1] * 101, points, 1), 'outside of execution trace')
    n += refused(lambda: nat.boundary_at(omega, T * 4, T, list(range(T)) + [0], [1] * (T + 1), points, 1), 'assertions, the execution trace')
    rng = random.Random(11)
    for log_t, m in ((8, 1), (8, 65), (8, 256), (10, 129), (11, 300), (13, 257)):
        T = 1 << log_t
        omega = root_of_unity(p, T * 4)
        at, ys = rng.sample(range(T), m), [rng.randrange(p) for _ in range(m)]
        points = [pow(omega, 4 * rng.randrange(T) + rng.randrange(1, 4), p) for _ in range(4)]
        assert nat.boundary_at(omega, T * 4, T, at, ys, points, 0) == nat.boundary_at(omega, T * 4, T, at, ys, points, 1), (log_t, m)
        assert nat.boundary_at(omega, T * 4, T, at, ys, [], 1) == ([], [])
        n += 1
    nat = NativeProver(Statement(quintic_air(f, 1 << 13)))
    a = golden_statement(p)
    data = open(GOLDEN, 'rb').read()
    assert nat.verify_bytes(a, data) is True
    n += refused(lambda: nat.verify_bytes(a + [a[10]], data), 'asserted more than once')
    n += refused(lambda: nat.verify_bytes(a + [{'step': 1 << 13, 'register': 0, 'value': 1}], data), 'outside of execution trace')
    n += refused(lambda: nat.verify_bytes(a[:2500] + a[2501:], data), 'Verification of linear combination correctness failed')
    wrong = [dict(x) for x in a]
    wrong[77]['value'] = (wrong[77]['value'] + 1) % p
    n += refused(lambda: nat.verify_bytes(wrong, data), 'Verification of linear combination correctness failed')
    for _ in range(200):
        bad = bytearray(data)
        kind = rng.randrange(3)
        if kind == 0:
            bad[rng.randrange(len(bad))] ^= 1 << rng.randrange(8)
        elif kind == 1:
            bad = bad[:rng.randrange(len(bad))]
        else:
            at_ = rng.randrange(len(bad))
            bad[at_:at_ + 4] = bytes(rng.randrange(256) for _ in range(4))
        if bytes(bad) == data:
            continue
        n += refused(lambda: nat.verify_bytes(a, bytes(bad)), '')
    loaded_instrumented_driver()
    print(f'sanitized boundary: {n} cases, no report')


def runtime_mode(q):
    from test_boundary_many_assertions import _check_entry_point
    be = Backend(device=0, modulus=q)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    ran = _check_entry_point(be, random.Random(q % 65521))
    # 65 536 assertions need a domain of 2^17 points: every listed size where the prime's two-adicity reaches that, all but that one otherwise
    adicity = ((q - 1) & -(q - 1)).bit_length() - 1
    assert adicity >= 16 and ran == [5, 63, 64, 65, 1000, 4096, 4097, 20000] + ([65536] if adicity >= 17 else []), (adicity, ran)
    f = PrimeField(backend=be)
    steps = 1 << 10
    rows = quintic_trace(q, steps, [5, 9])
    rng = random.Random(3)
    a = [{'step': s, 'register': 0, 'value': rows[s][0]} for s in rng.sample(range(steps), 700)] + \
        [{'step': s, 'register': 1, 'value': rows[s][1]} for s in rng.sample(range(steps), 33)]
    nat = NativeProver(Statement(quintic_air(f, steps)))
    blob = nat.prove_bytes(a, [], [5, 9])
    nat.host_boundary(True)
    assert nat.prove_bytes(a, [], [5, 9]) == blob, 'device path != host path'
    nat.host_boundary(False)
    assert nat.verify_bytes(a, blob) is True
    print(f'runtime boundary: modulus {q} ok')


if __name__ == '__main__':
    if sys.argv[1] == 'sanitized':
        sanitized_mode()
    else:
        runtime_mode(int(sys.argv[2]))
