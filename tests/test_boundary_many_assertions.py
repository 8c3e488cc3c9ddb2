"""Statements with thousands of assertions per register (include/gstark_boundary.h).

CPU tier: the verifier's two forms of the boundary values agree; a proof with 5 000 assertions on one register verifies and every
tampering is refused with the reference's message; malformed assertion sets are errors.
GPU tier: gs_boundary_polys against Python integers and gs_small_interpolate; proofs through the device path, the forced host path
and the oracle double are the same bytes; statements beyond the old cap of 4 096 assertions per register prove and verify."""
import ctypes as C
import os
import random

import pytest

from conftest import ROOT
from genstark_amd import _abi
from genstark_amd._abi import Backend
from genstark_amd.errors import StarkError
from genstark_amd.field import PrimeField
from genstark_amd.native import NativeProver

from boundary_common import (GOLDEN, OPTS, Statement as _Statement, golden_statement, host_driver, poseidon_statement, quad_air, quad_trace,  # noqa: E402
                             quintic_air, quintic_trace, rescue_statement, root_of_unity)


# ---------------------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize('modulus', [_abi.MODULUS_128, _abi.MODULUS_64, _abi.MODULUS_256], ids=['p128', 'q64', 'p256'])
def test_verifier_boundary_forms_agree(modulus):
    """I_r(x), Z_r(x) at points outside the execution domain by the reference's quadratic form and by the product tree: equal element
    for element, m in {1, 4, 5, 64, 1000, 4096} on T in 2^8 .. 2^13."""
    nat = host_driver(modulus)
    rng = random.Random(modulus % 9973)
    p = modulus
    for log_t in range(8, 14):
        T, E = 1 << log_t, 4
        omega = root_of_unity(p, T * E)
        for m in (1, 4, 5, 64, 1000, 4096):
            if m > T:
                continue
            at = rng.sample(range(T), m)
            ys = [rng.randrange(p) for _ in range(m)]
            points = [pow(omega, rng.randrange(T) * E + rng.randrange(1, E), p) for _ in range(6)]
            old = nat.boundary_at(omega, T * E, T, at, ys, points, 0)
            new = nat.boundary_at(omega, T * E, T, at, ys, points, 1)
            assert old == new, (log_t, m)
            if m <= 64:      # ... and both against the definition
                for q, x in enumerate(points):
                    z = 1
                    for s in at:
                        z = z * (x - pow(omega, s * E, p)) % p
                    assert new[1][q] == z


def test_verifier_accepts_5000_assertions_and_refuses_tampering(oracle_backend):
    """A proof of the quintic AIR (2^13 steps) asserting 5 000 cells of register 0 (beyond gs_small_interpolate's 4 096) and three of
    register 1, produced once on the GPU (tests/golden), verified natively on the host."""
    f = PrimeField(backend=oracle_backend)
    nat = NativeProver(_Statement(quintic_air(f, 1 << 13)))
    assertions = golden_statement(f.modulus)
    data = open(GOLDEN, 'rb').read()
    assert nat.verify_bytes(assertions, data) is True
    wrong = [dict(a) for a in assertions]
    wrong[1234]['value'] = (wrong[1234]['value'] + 1) % f.modulus
    with pytest.raises(StarkError, match='Verification of linear combination correctness failed'):
        nat.verify_bytes(wrong, data)
    with pytest.raises(StarkError, match='Verification of linear combination correctness failed'):
        nat.verify_bytes(assertions[:2500] + assertions[2501:], data)
    bad = bytearray(data)
    bad[len(bad) // 2] ^= 0x10                       # (the middle of this proof lies in the first FRI layer's polynomial proof)
    with pytest.raises(StarkError, match='Verification of polynomial Merkle proof failed at depth 0'):
        nat.verify_bytes(assertions, bytes(bad))
    bad = bytearray(data)
    bad[40] ^= 0x10                                  # ... and byte 40 in the evaluation proof's first leaf
    with pytest.raises(StarkError, match='Verification of evaluation Merkle proof failed'):
        nat.verify_bytes(assertions, bytes(bad))


def test_verifier_refuses_malformed_large_assertion_sets(oracle_backend):
    """duplicate steps on one register, a step outside the trace, more assertions than steps: errors with a message, not crashes"""
    f = PrimeField(backend=oracle_backend)
    T = 256
    nat = NativeProver(_Statement(quintic_air(f, T)))
    omega = root_of_unity(f.modulus, T * 4)
    points = [pow(omega, 5, f.modulus)]
    with pytest.raises(StarkError, match='asserted more than once'):
        nat.boundary_at(omega, T * 4, T, list(range(100)) + [7], [1] * 101, points, 1)
    with pytest.raises(StarkError, match='outside of execution trace'):
        nat.boundary_at(omega, T * 4, T, list(range(100)) + [T], [1] * 101, points, 1)
    with pytest.raises(StarkError, match='assertions, the execution trace'):
        nat.boundary_at(omega, T * 4, T, list(range(T)) + [0], [1] * (T + 1), points, 1)
    # ... and through verify(): a proof checked against an assertion list with a repeated cell
    nat13 = NativeProver(_Statement(quintic_air(f, 1 << 13)))
    assertions = golden_statement(f.modulus)
    with pytest.raises(StarkError, match='asserted more than once'):
        nat13.verify_bytes(assertions + [assertions[10]], open(GOLDEN, 'rb').read())


def test_optional_entry_points_are_optional(oracle_backend):
    """the oracle double lacks gs_boundary_polys: the library loads, the driver binds, and include/gstark.h does not list it"""
    assert not hasattr(oracle_backend.lib, 'gs_boundary_polys')
    assert set(_abi.OPTIONAL_SYMBOLS).isdisjoint(_abi.EXPORTED_SYMBOLS)
    header = open(os.path.join(ROOT, 'include', 'gstark_boundary.h')).read()
    for name in _abi.OPTIONAL_SYMBOLS:
        assert name + '(' in header


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def _kronecker_mul(a, b, p):
    """product of two coefficient lists over Z_p through one big-integer product"""
    w = (2 * p.bit_length() + max(len(a), len(b)).bit_length() + 7) // 8 + 1
    A = int.from_bytes(b''.join(c.to_bytes(w, 'little') for c in a), 'little')
    B = int.from_bytes(b''.join(c.to_bytes(w, 'little') for c in b), 'little')
    n = len(a) + len(b) - 1
    raw = (A * B).to_bytes(w * n + w, 'little')
    return [int.from_bytes(raw[i * w:(i + 1) * w], 'little') % p for i in range(n)]


def _zero_poly_ints(xs, p):
    level = [[(-x) % p, 1] for x in xs]
    while len(level) > 1:
        nxt = [_kronecker_mul(level[i], level[i + 1], p) for i in range(0, len(level) - 1, 2)]
        if len(level) & 1:
            nxt.append(level[-1])
        level = nxt
    return level[0]


def _boundary_polys(be, f, omega, n, T, rows):
    """rows: [(steps, values)] -> [(I coefficients, Z coefficients)] from gs_boundary_polys"""
    es, width = f.elementSize, max(len(s) for s, _ in rows)
    steps = (C.c_uint64 * (len(rows) * width))()
    vals = bytearray(len(rows) * width * es)
    for r, (s, v) in enumerate(rows):
        for k in range(len(s)):
            steps[r * width + k] = s[k]
            vals[(r * width + k) * es:(r * width + k + 1) * es] = f.le(v[k])
    per_row = (C.c_uint32 * len(rows))(*[len(s) for s, _ in rows])
    i_out, z_out = be.alloc(len(rows) * width * es), be.alloc(len(rows) * (width + 1) * es)
    be.call('gs_boundary_polys', f.le(omega), n, T, steps, bytes(vals), per_row, len(rows), width, C.c_void_p(i_out), C.c_void_p(z_out))
    iraw, zraw = be.download(i_out, len(rows) * width * es), be.download(z_out, len(rows) * (width + 1) * es)
    be.free(i_out), be.free(z_out)
    un = lambda raw, base, count: [int.from_bytes(raw[(base + k) * es:(base + k + 1) * es], 'little') for k in range(count)]
    return [(un(iraw, r * width, width), un(zraw, r * (width + 1), width + 1)) for r in range(len(rows))]


def _check_entry_point(be, rng, sizes=(5, 63, 64, 65, 1000, 4096, 4097, 20000, 65536)):
    f = PrimeField(backend=be)
    p, es = f.modulus, f.elementSize
    adicity = ((p - 1) & -(p - 1)).bit_length() - 1
    ran = []
    for m in sizes:
        T = 1 << max((m - 1).bit_length(), 3)
        if 2 * T > 1 << adicity:            # the field has no domain of 2 T points: the caller checks which sizes did run
            continue
        ran.append(m)
        n = 2 * T
        omega = f.getRootOfUnity(n)
        g = pow(omega, 2, p)
        k = max(T // m, 1)
        # one call: random steps, every k-th step, every step of a shorter domain prefix, and a short row
        rows = [rng.sample(range(T), m), list(range(0, k * m, k))[:m], list(range(min(m, T))), rng.sample(range(T), min(5, m))]
        rows = [(s, [rng.randrange(p) for _ in s]) for s in rows]
        got = _boundary_polys(be, f, omega, n, T, rows)
        width = max(len(s) for s, _ in rows)
        for (steps, ys), (icoef, zcoef) in zip(rows, got):
            mm = len(steps)
            xs = [pow(g, s, p) for s in steps]
            assert zcoef[mm] == 1 and not any(zcoef[mm + 1:]) and not any(icoef[mm:]), (m, mm)
            assert zcoef[:mm + 1] == _zero_poly_ints(xs, p), ('Z', m, mm)
            # I_r over the whole execution domain with the library's transform: y_i at every asserted step
            poly = be.alloc(T * es)
            be.upload(poly, b''.join(f.le(c) for c in icoef[:mm]) + bytes((T - mm) * es))
            ev = be.alloc(T * es)
            be.call('gs_eval_polys_at_roots', C.c_void_p(poly), 1, T, f.le(g), T, C.c_void_p(ev))
            raw = be.download(ev, T * es)
            be.free(poly), be.free(ev)
            assert all(int.from_bytes(raw[s * es:(s + 1) * es], 'little') == y for s, y in zip(steps, ys)), ('I on the domain', m, mm)
            for i in rng.sample(range(mm), min(mm, 8)):             # ... and by Horner on Python integers
                acc = 0
                for c in reversed(icoef[:mm]):
                    acc = (acc * xs[i] + c) % p
                assert acc == ys[i], ('I', m, mm, i)
            if mm <= 4096:
                out = C.create_string_buffer(mm * es)
                assert be.lib.gs_small_interpolate(b''.join(f.le(x) for x in xs), b''.join(f.le(y) for y in ys), mm, C.cast(out, C.c_void_p)) == 0
                assert out.raw == b''.join(f.le(c) for c in icoef[:mm]), ('gs_small_interpolate', m, mm)
    return ran


@pytest.mark.gpu
@pytest.mark.parametrize('modulus', [None, _abi.MODULUS_64, _abi.MODULUS_32, _abi.MODULUS_17, _abi.MODULUS_256, _abi.MODULUS_224],
                         ids=['p128', 'q64', 'q32', 'q17', 'p256', 'p224'])
def test_gs_boundary_polys_against_integers(modulus):
    be = Backend(device=0, modulus=modulus)
    try:
        ran = _check_entry_point(be, random.Random(0xB0DA))
        # every listed size, except in the 17-bit field: 96769 - 1 = 2^9 * 189 carries domains of at most 512 points (T <= 256)
        assert ran == ([5, 63, 64, 65] if modulus == _abi.MODULUS_17 else [5, 63, 64, 65, 1000, 4096, 4097, 20000, 65536]), ran
    finally:
        be.close()


@pytest.mark.gpu
def test_gs_boundary_polys_refuses_bad_steps(hip_backend):
    f = PrimeField(backend=hip_backend)
    omega = f.getRootOfUnity(512)
    for steps in ([1, 2, 3, 2, 9, 10], [1, 2, 3, 4, 5, 256]):
        with pytest.raises(_abi.GstarkError):
            _boundary_polys(hip_backend, f, omega, 512, 256, [(steps, [1] * len(steps))])


@pytest.mark.gpu
@pytest.mark.parametrize('log2_len', [2, 4, 8, 10])
def test_tree_switch_over_does_not_change_the_result(hip_backend, log2_len):
    """schoolbook and transform products give the same tree wherever the switch-over lies"""
    f = PrimeField(backend=hip_backend)
    before = hip_backend.lib.gs_boundary_schoolbook_log2(log2_len)
    try:
        _check_entry_point(hip_backend, random.Random(log2_len), sizes=(65, 1000, 4097))
    finally:
        hip_backend.lib.gs_boundary_schoolbook_log2(before)


def _mimc_case(be, steps, m, rng, opts):
    from genstark_amd.air import MimcAir, runMimc
    f = PrimeField(backend=be)
    air = MimcAir(steps, opts['extensionFactor'], f)
    control = runMimc(f, steps, air.roundConstants, 3)
    return air, [{'step': s, 'register': 0, 'value': control[s]} for s in rng.sample(range(steps), m)], [3]


def _quintic_case(be, steps, ms, rng, opts):
    f = PrimeField(backend=be)
    rows = quintic_trace(f.modulus, steps, [5, 9])
    a = []
    for reg, m in enumerate(ms):
        a += [{'step': s, 'register': reg, 'value': rows[s][reg]} for s in rng.sample(range(steps), m)]
    rng.shuffle(a)
    return quintic_air(f, steps), a, [5, 9]


def _quad_case(be, steps, ms, rng, opts):
    f = PrimeField(backend=be)
    rows = quad_trace(f.modulus, steps, [5, 9, 2, 3])
    a = []
    for reg, m in enumerate(ms):
        a += [{'step': s, 'register': reg, 'value': rows[s][reg]} for s in rng.sample(range(steps), m)]
    rng.shuffle(a)
    return quad_air(f, steps), a, [5, 9, 2, 3]


@pytest.mark.gpu
@pytest.mark.parametrize('alg', ['blake2s256', 'sha256'])
def test_proof_bytes_device_path_host_path_and_oracle(hip_backend, oracle_backend, alg):
    """the same statement through the driver bound to the HIP library (device path), the same with the host path forced, and bound to
    the oracle double (host path): identical bytes; the native verifier accepts them"""
    opts = dict(OPTS, hashAlgorithm=alg)
    steps = 1 << 13
    # (the oracle double's own gs_small_interpolate takes 15 s for 1 000 points and grows with the cube of the count: registers with
    #  4 096 assertions are compared between the two paths on the HIP binding only)
    cases = [('mimc', 5, True), ('mimc', 64, True), ('mimc', 1000, True), ('mimc', 4096, False),
             ('quintic', (5, 64), True), ('quintic', (1000, 64), True), ('quintic', (1000, 4096), False), ('quintic', (4096, 5), False), ('quintic', (64,), True)]
    cases += [('quad', (5, 64, 200), True), ('quad', (200, 5, 64, 200), True), ('quad', (1000, 200, 64, 300), False)]
    for kind, shape, with_oracle in cases:
        blobs = []
        for be in (hip_backend, oracle_backend) if with_oracle else (hip_backend,):
            rng = random.Random(str((kind, shape)))
            air, a, seed = _mimc_case(be, steps, shape, rng, opts) if kind == 'mimc' else (_quintic_case if kind == 'quintic' else _quad_case)(be, steps, shape, rng, opts)
            nat = NativeProver(_Statement(air, opts))
            blobs.append(nat.prove_bytes(a, [], seed))
            if be is hip_backend:
                nat.host_boundary(True)
                try:
                    blobs.append(nat.prove_bytes(a, [], seed))
                finally:
                    nat.host_boundary(False)
                assert nat.verify_bytes(a, blobs[0]) is True
        assert blobs[0] == blobs[1], (kind, shape, 'device path != forced host path')
        if with_oracle:
            assert blobs[0] == blobs[2], (kind, shape, 'HIP != oracle')


@pytest.mark.gpu
def test_beyond_the_old_cap(hip_backend):
    """more than 4 096 assertions on a register: proves on the device path, verifies, and wrong statements are refused"""
    f = PrimeField(backend=hip_backend)
    p = f.modulus
    # the golden statement of the CPU tier (5 000 + 3 assertions, 2^13 steps): the committed proof is what the driver gives today
    nat = NativeProver(_Statement(quintic_air(f, 1 << 13)))
    a = golden_statement(p)
    blob = nat.prove_bytes(a, [], [5, 9])
    assert nat.verify_bytes(a, blob) is True
    assert blob == open(GOLDEN, 'rb').read()
    # 2^16 steps: every step of register 0 (65 536 assertions) and 20 000 cells of register 1
    steps = 1 << 16
    rows = quintic_trace(p, steps, [5, 9])
    rng = random.Random(16)
    a = [{'step': s, 'register': 0, 'value': rows[s][0]} for s in range(steps)] + \
        [{'step': s, 'register': 1, 'value': rows[s][1]} for s in rng.sample(range(steps), 20000)]
    nat = NativeProver(_Statement(quintic_air(f, steps)))
    blob = nat.prove_bytes(a, [], [5, 9])
    assert nat.verify_bytes(a, blob) is True
    wrong = [dict(x) for x in a]
    wrong[70000]['value'] = (wrong[70000]['value'] + 1) % p
    with pytest.raises(StarkError, match=f"Assertion at step {wrong[70000]['step']}, register 1 conflicts with execution trace"):
        nat.prove_bytes(wrong, [], [5, 9])
    with pytest.raises(StarkError, match='Verification of linear combination correctness failed'):
        nat.verify_bytes(wrong, blob)
    with pytest.raises(StarkError, match='Verification of linear combination correctness failed'):
        nat.verify_bytes(a[:-1], blob)
    nat.host_boundary(True)
    try:
        with pytest.raises(StarkError, match='gs_small_interpolate failed'):       # the host path keeps its cap
            nat.prove_bytes(a, [], [5, 9])
    finally:
        nat.host_boundary(False)


def _prove_verify_and_refuse(nat, a, seeds, tamper_at):
    """proves, verifies; a wrong value is refused at prove time with the reference's message; an altered assertion list is refused by verify"""
    blob = nat.prove_bytes(a, [], seeds)
    assert nat.verify_bytes(a, blob) is True
    wrong = [dict(x) for x in a]
    wrong[tamper_at]['value'] = (wrong[tamper_at]['value'] + 1) % nat.field.modulus
    w = wrong[tamper_at]
    with pytest.raises(StarkError, match=f"Assertion at step {w['step']}, register {w['register']} conflicts with execution trace"):
        nat.prove_bytes(wrong, [], seeds)
    with pytest.raises(StarkError, match='Verification of linear combination correctness failed'):
        nat.verify_bytes(wrong, blob)
    with pytest.raises(StarkError, match='Verification of linear combination correctness failed'):
        nat.verify_bytes(a[:tamper_at] + a[tamper_at + 1:], blob)
    return blob


@pytest.mark.gpu
def test_rescue_every_chain_asserted(hip_backend):
    """C3-shaped: Rescue 4x128, 2^16 steps = 2 048 chains, every chain's first and last row asserted: 4 096 assertions on each of four
    registers (the old cap).  Device path == forced host path."""
    f = PrimeField(backend=hip_backend)
    air, a, seeds = rescue_statement(f, 2048)
    assert len(a) == 4 * 4096
    nat = NativeProver(_Statement(air, dict(OPTS, exeQueryCount=68, friQueryCount=24)))
    blob = _prove_verify_and_refuse(nat, a, seeds, 9001)
    nat.host_boundary(True)
    try:
        assert nat.prove_bytes(a, [], seeds) == blob
    finally:
        nat.host_boundary(False)


@pytest.mark.gpu
def test_poseidon_every_output_asserted(hip_backend):
    """C4-long-shaped: Poseidon 6x128, 2^20 steps = 16 384 chains, every chain's output asserted on one register (beyond the old cap)."""
    f = PrimeField(backend=hip_backend)
    air, a, seeds = poseidon_statement(f, 16384)
    assert len(a) == 16384
    nat = NativeProver(_Statement(air, dict(OPTS, exeQueryCount=48, friQueryCount=24)))
    _prove_verify_and_refuse(nat, a, seeds, 12345)


def _runtime_primes():
    """three of tests/test_runtime_modulus.py's primes: 31, 61 and 255 bits"""
    from test_runtime_modulus import PRIMES
    return [PRIMES[0], PRIMES[6], PRIMES[18]]


@pytest.mark.gpu
@pytest.mark.parametrize('which', [0, 1, 2], ids=['31bit', '61bit', '255bit'])
def test_runtime_modulus_flavour(which):
    """the runtime-modulus flavour (one modulus per process: a worker): the entry point against integers, a proof through both paths"""
    import subprocess
    import sys
    q = _runtime_primes()[which]
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'boundary_worker.py'), 'runtime', str(q)], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f'runtime boundary: modulus {q} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_sanitized_verifier_on_large_assertion_sets():
    """the sanitizer tier for the new host code (host_transform, poly_product, zero_poly_tree, boundary_values_tree, Plan::fill_xs,
    gs_prover_boundary_at_on): malformed sets, both forms, the golden proof with altered assertions and corrupted bytes under
    -fsanitize=address,undefined — refusals, no report"""
    import subprocess
    import sys
    import test_sanitizers as ts
    if not (ts.ASAN and ts.STDCPP):
        pytest.skip('libasan is not in this image')
    from conftest import _build_oracle
    _build_oracle()
    out = subprocess.check_output(['bash', os.path.join(ROOT, 'tools', 'build_sanitized.sh')], text=True).strip().splitlines()[-1]
    stdout = ts.run_clean([sys.executable, os.path.join(ROOT, 'tests', 'boundary_worker.py'), 'sanitized'], ts.san_env(out), 'sanitized boundary:')
    assert 'no report' in stdout


@pytest.mark.gpu
def test_interpolate_at_roots_public_surface(hip_backend):
    """PrimeField.interpolateAtRoots: a device vector with interpolate's coefficients, also beyond interpolate's 4 096 points"""
    f = PrimeField(backend=hip_backend)
    p, rng = f.modulus, random.Random(99)
    for order, m in ((256, 5), (4096, 1000), (1 << 14, 6000)):
        g = f.getRootOfUnity(order)
        pos, ys = rng.sample(range(order), m), [rng.randrange(p) for _ in range(m)]
        got = f.interpolateAtRoots(g, order, pos, ys)
        assert got.length == m
        coef = got.toValues()
        if m <= 4096:
            assert coef == f.interpolate([pow(g, s, p) for s in pos], ys).toValues()
        else:
            with pytest.raises(_abi.GstarkError):
                f.interpolate([pow(g, s, p) for s in pos], ys)
        for i in rng.sample(range(m), min(m, 16)):
            acc = 0
            for c in reversed(coef):
                acc = (acc * pow(g, pos[i], p) + c) % p
            assert acc == ys[i]


def _node_interpolate(mode, env_extra):
    import shutil
    import subprocess
    node = shutil.which('node')
    if not (node and os.path.exists('/usr/include/node/node_api.h')):
        pytest.skip('node or its headers are not in this image')
    subprocess.check_call(['bash', os.path.join(ROOT, 'napi', 'build.sh')], stdout=subprocess.DEVNULL)
    r = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_interpolate_at_roots.js'), mode], cwd=ROOT, env=dict(os.environ, **env_extra),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f'js interpolateAtRoots ({mode}) OK' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_js_interpolate_without_the_optional_entry_point():
    """galois.js on a library without gs_boundary_polys (the oracle double): has() says so, interpolateAtRoots throws, interpolate()
    behaves as before, its 4 096 cap and error included"""
    from conftest import _build_oracle
    _build_oracle()
    _node_interpolate('double', {'GSTARK_LIB_DIR': os.path.join(ROOT, 'oracle'), 'GSTARK_ALLOW_TEST_DOUBLE': '1'})


@pytest.mark.gpu
def test_js_interpolate_at_roots():
    """galois.interpolateAtRoots on the GPU: == interpolate() up to 4 096 points, the definition above; interpolate() of a power series routed"""
    _node_interpolate('hip', {})


@pytest.mark.gpu
def test_interpolate_routes_power_series_and_other_generators(hip_backend):
    """PrimeField.interpolate of a whole power series goes to the device (8 192 points: beyond the host cap) and gives interpolateRoots'
    polynomial; interpolateAtRoots takes any generator of the domain"""
    f = PrimeField(backend=hip_backend)
    p, rng = f.modulus, random.Random(5)
    n = 8192
    xs = f.getPowerSeries(f.getRootOfUnity(n), n)
    ys = f.newVectorFrom([rng.randrange(p) for _ in range(n)])
    assert f.interpolate(xs, ys).toValues() == f.interpolateRoots(xs, ys).toValues()
    order, m = 1024, 300
    g = pow(f.getRootOfUnity(order), 77, p)
    pos, yv = rng.sample(range(order), m), [rng.randrange(p) for _ in range(m)]
    assert f.interpolateAtRoots(g, order, pos, yv).toValues() == f.interpolate([pow(g, s, p) for s in pos], yv).toValues()
    with pytest.raises(_abi.GstarkError):
        f.interpolateAtRoots(5, order, pos, yv)             # not a generator of a 1 024-point domain
