#!/usr/bin/env python
"""bench.py — prove() wall-clock and NTT GF(p) elements/s for MiMC-128 on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W        (N > 1: one rank per GPU under torch.distributed.run — by the caller, or by
                                                          bench.py itself when WORLD_SIZE is not set)
    python bench.py ... --full                           everything below as well (roofline, CPU baseline, configurations, ...)
    python bench.py ... --dump-outputs DIR               the last timed step's proof as DIR/proof_bytes.npy (float32, one per byte)

A plain run sets up, warms up, times the K steps and prints the line: `value`, `ms_per_step`, `prove_ms`, `phases_ms` and the
config record come from the timed steps alone.  Everything else this file describes (the Python-mirror cross-check and verification
of the timed proof, `roofline`, `cpu_baseline`, `configs`, `phases_readme`, `pipelined`, and at N > 1 the `one_proof` leg) runs
only under --full.

One "step" = one complete prove() of the workload (default: BASELINE configs[4] = MiMC-128, 2^20 trace steps,
extensionFactor 16, exeQueryCount 48, friQueryCount 64, blake2s256): execution trace, iNTT, LDE, leaf hashing,
Merkle trees, composition polynomial, linear combination, FRI, spot checks — nothing skipped.  The only input of
prove() is the seed; every vector lives in HBM for the whole step.

Multi-GPU (N > 1): `value` is one independent proof per GPU — rank r proves its own trace (seed 3 + r): weak scaling, no data-path
collective (a single MiMC proof is bounded by the serial recurrence of its one trace register).  Beside it, `one_proof`: ONE proof
across all ranks through the native distributed driver (csrc/prover_dist.h) over RCCL on device buffers (csrc/comm_rccl.cc) — C4
(BASELINE configs[3]: Poseidon, 6 registers, 2^16 steps as 1 024 hash chains) with the single-GPU time of the same run (strong
scaling), and C5 (the headline statement); `collectives[]` lists every exchange with its bytes and device time, `rccl_ranks` the
communicator size.

`value` = NTT points transformed per second at whole-prove() level, aggregated over ranks:
          (points of the transforms the timed driver LAUNCHED, from its own counters: gs_prover_last_stats) * K * N
          / max-over-ranks wall time.  For MiMC-128 that is the trace iNTT (T points) and the low-degree extension (N points)
          plus two small transforms of the round-constant register: the composition polynomial is evaluated directly on the
          evaluation domain (gs_mimc_composition), no transform is credited that did not run.
`prove_ms` (= ms_per_step) is the other half of BASELINE.json's metric; `phases_ms` comes from the driver's own clock.
`roofline` describes the dominant kernel (one radix-256 NTT pass, k_ntt_wave<4, *>), timed live with events on the
stream the kernels run on; `roofline.second_roof` is the VALU-issue roof measured in the same run (tools/microbench5: the
kernel's own product routines on registers only); `roofline.traffic` is read from the PMC counters by a rocprofv3 child
process of this run (tools/pmc_traffic.py).  `cpu_baseline` is the same prove() on the CPU oracle's implementation of the
C ABI: single-threaded and on every host core (OpenMP build of the same source), on bounded samples.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s spec, ~6.3 TB/s achievable)


def expected_ntt_points(steps, ef):
    """What the native driver launches as NTT passes for MiMC-128 (counted by the driver itself; this closed form is only the
    cross-check): iNTT(T) of the trace + LDE NTT(N) + iNTT(64·cf) and NTT(64·E) of the 64-periodic round-constant register."""
    return steps + steps * ef + 64 * 4 + 64 * ef


def make_stark(ga, backend, steps, ef, fri, logger=None):
    opts = {'hashAlgorithm': 'blake2s256', 'extensionFactor': ef, 'exeQueryCount': 48, 'friQueryCount': fri}
    return ga.instantiateMimc(steps, opts, logger, backend=backend)


def assertions_for(stark, steps, seed):
    trace = stark.generateExecutionTrace([], [seed])['dTrace']
    return [{'step': 0, 'register': 0, 'value': trace.getValue(0, 0)},
            {'step': steps - 1, 'register': 0, 'value': trace.getValue(0, steps - 1)}]


def cpu_prove(ga, lib, log_steps, ef, exe, fri, threads, timeout=120):
    """one prove() through the native driver on the CPU oracle's implementation of the C ABI, in a child process pinned to
    `threads` OpenMP threads; returns (seconds, ntt_points, sha256 hex of the serialized proof, its length) — seed 3, assertions at
    the first and the last step, like the timed GPU proof of rank 0"""
    import subprocess
    code = (
        'import sys, time, json, hashlib; sys.path.insert(0, %r)\n'
        'import genstark_amd as ga\n'
        'from genstark_amd._abi import Backend\n'
        'from genstark_amd.native import NativeProver\n'
        'be = Backend(lib_path=%r, allow_test_double=True)\n'
        'steps = 1 << %d\n'
        'st = ga.instantiateMimc(steps, {"hashAlgorithm": "blake2s256", "extensionFactor": %d, "exeQueryCount": %d, "friQueryCount": %d}, backend=be)\n'
        'tr = st.generateExecutionTrace([], [3])["dTrace"]\n'
        'a = [{"step": 0, "register": 0, "value": tr.getValue(0, 0)}, {"step": steps - 1, "register": 0, "value": tr.getValue(0, steps - 1)}]\n'
        'p = NativeProver(st)\n'
        't0 = time.perf_counter(); d = p.prove_bytes(a, [], [3]); dt = time.perf_counter() - t0\n'
        'assert st.verify(a, st.parse(d))\n'
        'print(json.dumps({"s": dt, "points": p.last_stats()["ntt_points"], "sha256": hashlib.sha256(d).hexdigest(), "bytes": len(d)}))\n') % (ROOT, lib, log_steps, ef, exe, fri)
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), OMP_PROC_BIND='false', OMP_WAIT_POLICY='passive')
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode:
        raise RuntimeError(r.stderr[-400:])
    j = json.loads(r.stdout.strip().splitlines()[-1])
    return j['s'], j['points'], j['sha256'], j['bytes']


def cpu_baseline(ga, ef, fri, gpu_digest=None):
    """the CPU path timed on this box's host cores, single-threaded AND on all cores, core count stated, for C2
    (2^13 steps, E=16, exe 48, fri 24) and for the largest trace that stays within the time budget.  "port": the oracle's plain-C
    implementation of the same C ABI under the same native driver (oracle/liboracle_omp.so = oracle_abi.c built with -fopenmp)."""
    import subprocess
    lib = os.path.join(ROOT, 'oracle', 'liboracle_omp.so')
    if not os.path.exists(lib):
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'oracle'), '-s', 'liboracle_omp.so'])
    visible = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    rows = []
    budget = time.perf_counter() + 50.0
    compared = []

    def same(log_steps, ef_, exe, fri_, sha):
        # the proof the CPU run produced against the GPU's for the same statement (gpu_digest proves it on the HIP library): bytes, via sha256
        if gpu_digest is None:
            return None
        ok = gpu_digest(log_steps, ef_, exe, fri_) == sha
        compared.append((log_steps, ef_, fri_, ok))
        return ok
    # C2 first: one thread, then a sweep of thread counts up to every visible CPU — a container may see more CPUs than its quota
    # lets it run (the first all-256 attempt on the GPU box was 100x slower than one thread); `cores` = the count that won
    s_, pts, sha, _ = cpu_prove(ga, lib, 13, 16, 48, 24, 1)
    rows.append({'config': 'C2: 2^13 steps, E=16, exe 48, fri 24', 'threads': 1, 'prove_ms': round(s_ * 1e3, 1), 'elements_per_s': pts / s_,
                 'same_bytes_as_gpu': same(13, 16, 48, 24, sha)})
    cores, best_c2 = 1, s_
    for threads in [t for t in (4, 8, 16, 32, 64, 128) if t < visible] + [visible]:
        try:
            s_, pts, sha, _ = cpu_prove(ga, lib, 13, 16, 48, 24, threads)
        except Exception:   # noqa: BLE001  (timeout: oversubscribed)
            break
        rows.append({'config': 'C2: 2^13 steps, E=16, exe 48, fri 24', 'threads': threads, 'prove_ms': round(s_ * 1e3, 1), 'elements_per_s': pts / s_})
        if s_ < best_c2:
            cores, best_c2 = threads, s_
        elif s_ > 3 * best_c2:
            break
    # then the headline shape (E, fri of the workload) at growing trace lengths while the budget lasts: all cores, and one thread
    best = None
    one = None
    for log_steps in (14, 16, 18, 20):
        if best is not None and best['s'] * 4.5 > budget - time.perf_counter():
            break
        s_, pts, sha, nbytes = cpu_prove(ga, lib, log_steps, ef, 48, fri, cores)
        best = {'log': log_steps, 's': s_, 'points': pts, 'same': same(log_steps, ef, 48, fri, sha), 'bytes': nbytes}
        rows.append({'config': f'2^{log_steps} steps, E={ef}, exe 48, fri {fri}', 'threads': cores, 'prove_ms': round(s_ * 1e3, 1), 'elements_per_s': pts / s_,
                     'same_bytes_as_gpu': best['same'], 'proof_bytes': nbytes})
    for log_steps in (14, 16, 18):
        if one is not None and one['s'] * 4.5 > budget + 25.0 - time.perf_counter():
            break
        s_, pts, sha, _ = cpu_prove(ga, lib, log_steps, ef, 48, fri, 1)
        one = {'log': log_steps, 's': s_, 'points': pts}
        rows.append({'config': f'2^{log_steps} steps, E={ef}, exe 48, fri {fri}', 'threads': 1, 'prove_ms': round(s_ * 1e3, 1), 'elements_per_s': pts / s_})
    return {'value': best['points'] / best['s'], 'unit': 'elements/s', 'cores': cores, 'kind': 'port',
            'sample': f'one prove() of MiMC-128 2^{best["log"]} steps, E={ef}, friQueryCount={fri} through the native driver on the CPU oracle '
                      f'(oracle_abi.c, OpenMP, {cores} threads): {best["s"]:.2f} s; NTT points launched / wall time',
            'prove_ms': round(best['s'] * 1e3, 1),
            # every CPU proof of this leg is compared with the GPU's proof of the same statement (sha256 of the serialized bytes)
            'same_bytes_as_gpu': (all(ok for *_, ok in compared) if compared else None), 'proof_bytes': best['bytes'],
            'bytes_compared_for': [f'2^{l} steps, E={e}, fri {q}' for l, e, q, _ in compared],
            'single_thread': {'value': one['points'] / one['s'], 'unit': 'elements/s', 'cores': 1, 'prove_ms': round(one['s'] * 1e3, 1),
                              'sample': f'the same at 2^{one["log"]} steps on one thread'},
            'all_runs': rows, 'host_cpus_visible': visible,
            'cores_note': f'{visible} CPUs visible; {cores} threads was the fastest of the sweep on C2 and is what "all cores" uses'}


# issue cost of one wave-instruction per SIMD with 4 waves resident, by class (tools/microbench4.hip -> profiles/r02_a_instruction_costs.txt)
VALU_CLASS_NS = {'cheap': 1.1, 'vop3': 1.8, 'carry': 1.95, 'mad64': 2.0}


def ntt_plan(logn, table_log=20):
    """the pass structure csrc/ntt.hip builds for a 2^logn-point transform: [(log2 radix, twiddle source)], twiddle source 0 = first
    pass (none), 1 = [k][jq] table (<= 2^20 entries), 2 = running product"""
    np_ = (logn + 7) // 8
    base, extra = logn // np_, logn % np_
    out, acc = [], 0
    for i in range(np_):
        l = base + (1 if i < extra else 0)
        out.append((l, 0 if i == 0 else (1 if acc + l <= table_log else 2)))
        acc += l
    return out


def second_roof(n, transform_ms, npass, traffic_detail=None):
    """The roof the NTT kernel actually sits under: VALU issue.  Two derivations, both from this run and this build:
    (a) routines: tools/microbench5 runs the kernel's own product routines on registers only (no memory traffic); per 16 elements a
        pass does two radix-16 networks, 15 per-lane exchange products, 16 per-lane input products on twiddled passes (+ 15 per-lane
        chain products when the twiddles are a running product), 16 pack + unpack;
    (b) counters: the kernels' VALU instruction count — SQ_INSTS_VALU of the same launches (rocprofv3 child process), checked against
        the static instruction mix of the compiled kernels (csrc/ntt_isa_mix.json, straight-line code) — times the measured issue
        cost of each instruction class."""
    import subprocess
    logn = n.bit_length() - 1
    plan = ntt_plan(logn)
    out = {'bound': 'valu-issue', 'unit': 'ms per transform', 'achieved': round(transform_ms, 4), 'plan': plan}
    exe = os.path.join(ROOT, 'tools', 'microbench5')
    simds = 1024
    if os.path.exists(exe):
        try:
            r = subprocess.run([exe, '--json'], capture_output=True, text=True, timeout=120)
            m = json.loads(r.stdout.strip().splitlines()[-1])
            simds = m['cus'] * 4
            occ = 4                                  # every k_ntt_wave variant holds 4 waves per SIMD since round 3 (<= 128 VGPRs, no scratch)
            dif, mulv, pack = m['dif16_network_ns'][occ - 1], m['mul_v_ns'][occ - 1], m['pack_unpack_add_ns'][occ - 1]
            per_wave = [2 * dif + (15 + (16 if tw else 0) + (15 if tw == 2 else 0)) * mulv + 16 * pack for _, tw in plan]
            floor_ms = sum(per_wave) * (n / 16 / 64) / simds * 1e-6
            out.update({'peak': round(floor_ms, 4), 'frac': round(floor_ms / transform_ms, 4),
                        'measured_ns_per_wave_at_1_2_3_4_waves_per_simd': {'radix16_network_17_products_64_addsub_16_norm': m['dif16_network_ns'],
                                                                           'per_lane_product': m['mul_v_ns'], 'pack_unpack_add': m['pack_unpack_add_ns'],
                                                                           'canonical_limb_fe_mul_for_reference': m['fe_mul_ns']},
                        'kernel_waves_per_simd': occ,
                        'note': 'peak = time the passes\' own routines need with no memory stall at all (registers-only microbenchmark at the '
                                'kernel\'s occupancy, same run); frac = peak / achieved'})
        except Exception as e:   # noqa: BLE001
            out['error'] = repr(e)[:200]
    else:
        out['error'] = 'tools/microbench5 not built'
    # (b) from the counters of the kernels themselves
    try:
        mix = json.load(open(os.path.join(ROOT, 'genstark_amd', 'csrc', 'ntt_isa_mix.json')))
        waves = n / 16 / 64
        rows, total_ns = [], 0.0
        for l, tw in plan:
            key = next((k for k in mix if f'k_ntt_waveILi{l - 4}ELi{tw}E' in k), None)
            if key is None:
                raise KeyError(f'k_ntt_wave<{l - 4}, {tw}>')
            k = mix[key]
            ns_per_wave = sum(k[c] * VALU_CLASS_NS[c] for c in VALU_CLASS_NS)
            counted = util = None
            for name, d in ((traffic_detail or {}).get('kernels') or {}).items():
                if name.replace(' ', '').startswith(f'k_ntt_wave<{l - 4},{tw}>') and d.get('SQ_INSTS_VALU_avg'):
                    counted = d['SQ_INSTS_VALU_avg']
                    util = d.get('valu_issue_utilisation')
            insts = counted if counted else k['valu'] * waves
            rows.append({'kernel': f'k_ntt_wave<{l - 4}, {tw}>', 'static_valu_per_wave': k['valu'], 'mix': {c: k[c] for c in VALU_CLASS_NS},
                         'SQ_INSTS_VALU_per_launch': counted, 'static_valu_per_launch': k['valu'] * waves,
                         'issue_floor_us': round(insts * (ns_per_wave / k['valu']) / simds * 1e-3, 1),
                         'valu_issue_utilisation': util})
            total_ns += insts * (ns_per_wave / k['valu']) / simds
        out['from_counters'] = {'peak': round(total_ns * 1e-6, 4), 'frac': round(total_ns * 1e-6 / transform_ms, 4), 'passes': rows,
                                'class_cost_ns': VALU_CLASS_NS,
                                'note': 'VALU wave-instructions of each pass (SQ_INSTS_VALU when the PMC pass ran, else the static count of the '
                                        'straight-line kernel x waves) x issue cost of their classes / SIMDs: dependency stalls inside the '
                                        'routines are NOT in this floor, which is why it is lower than `peak`.  valu_issue_utilisation: '
                                        'SQ_ACTIVE_INST_VALU x 4 / 1024 SIMDs over GRBM_GUI_ACTIVE / 8 XCDs of the same launches — the share of '
                                        'its own cycles a SIMD spent issuing vector instructions, at whatever clock the part sustained'}
    except Exception as e:   # noqa: BLE001
        out['from_counters'] = {'error': repr(e)[:200]}
    return out


def dump_outputs(out_dir, data, rank, world, limit=64 << 20):
    """what the timed path returned in its last step, the serialized proof, as float32 (one value per byte, exact): rank 0 writes
    out_dir/proof_bytes.npy, rank r > 0 out_dir/proof_bytes_rank<r>.npy.  A proof larger than this rank's share of `limit` bytes of
    .npy data is written as a fixed, seeded sample of its byte positions (proof_bytes_index.npy beside it, float64)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    suffix = '' if rank == 0 else f'_rank{rank}'
    vals = np.frombuffer(data, dtype=np.uint8).astype(np.float32)
    share = limit // max(world, 1)
    if vals.size * 4 > share:
        cap = share // 12                                # float32 value + float64 index per sampled byte
        pos = np.sort(np.random.default_rng(0x5eed).choice(vals.size, size=cap, replace=False))
        vals = vals[pos]
        np.save(os.path.join(out_dir, f'proof_bytes_index{suffix}.npy'), pos.astype(np.float64))
    np.save(os.path.join(out_dir, f'proof_bytes{suffix}.npy'), vals)


def pmc_traffic(logn):
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'pmc_traffic.py'), str(logn)], capture_output=True, text=True, timeout=420)
        j = json.loads(r.stdout.strip().splitlines()[-1])
        return j.get('hbm_bytes_per_launch'), j
    except Exception as e:   # noqa: BLE001
        return None, {'error': repr(e)[:200]}


def comm_selftest(backend, comm, rank, world):
    """Both collectives of a gs_comm (include/gstark_comm.h) on rank-stamped patterns in device buffers of `backend`; returns None or
    what went wrong.  Piece h of rank r's send buffer is the byte (16 * r + h) & 255 repeated (+ the offset inside the piece)."""
    import ctypes as C
    piece = 4096
    ag = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    pat = lambda r, h: bytes(((16 * r + h + 7 * i) & 255) for i in range(piece))
    send, recv = backend.alloc(piece * world), backend.alloc(piece * world)
    try:
        backend.upload(send, b''.join(pat(rank, h) for h in range(world)))
        rc = ag(comm.all_gather)(comm.self, backend.ctx, send, recv, piece)          # contributes piece 0 of the send buffer
        backend.sync()
        if rc:
            return f'all_gather returned {rc}'
        if backend.download(recv, piece * world) != b''.join(pat(r, 0) for r in range(world)):
            return 'all_gather delivered wrong bytes'
        backend.upload(recv, bytes(piece * world))
        rc = ag(comm.all_to_all)(comm.self, backend.ctx, send, recv, piece)
        backend.sync()
        if rc:
            return f'all_to_all returned {rc}'
        if backend.download(recv, piece * world) != b''.join(pat(r, rank) for r in range(world)):
            return 'all_to_all delivered wrong bytes'
        if comm.fork and comm.join:
            # the overlapped form the driver uses for the evaluation tree's digests (gs_comm::fork / join): the collective goes to the
            # communicator's own stream behind an event, the context's stream waits for it at join
            fj = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
            backend.upload(recv, bytes(piece * world))
            rc = fj(comm.fork)(comm.self, backend.ctx) or ag(comm.all_to_all)(comm.self, backend.ctx, send, recv, piece) or fj(comm.join)(comm.self, backend.ctx)
            backend.sync()
            if rc:
                return f'forked all_to_all returned {rc}'
            if backend.download(recv, piece * world) != b''.join(pat(r, rank) for r in range(world)):
                return 'forked all_to_all delivered wrong bytes'
        if comm.take_timings:
            tt = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.POINTER(C.c_double), C.c_uint32)
            tt(comm.take_timings)(comm.self, (C.c_double * 8)(), 8)                   # drain the event pairs
        return None
    finally:
        backend.free(send)
        backend.free(recv)


def self_launch(n):
    """Re-execute this command line under torch.distributed.run with n ranks on this node (127.0.0.1, a free port); returns the
    launcher's exit code.  (The N > 1 form `python -m torch.distributed.run ... bench.py --gpus N` sets WORLD_SIZE and never gets here.)"""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(('127.0.0.1', 0))
        port = so.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # dmabuf IPC: what RCCL needs on this driver
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


# ---- the ONE line the driver parses.  Round 5's line had grown to 28.7 KB and the driver could not parse it (BENCH_r05.json.parsed == null);
# the line is now the contract keys plus one-level summaries, bounded by LINE_LIMIT; everything else is written to bench_detail.json
LINE_LIMIT = 6000
ROOFLINE_KEYS = ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'traffic_source', 'kernel', 'launch_ms', 'transform_ms',
                 'ntt_kernel_elements_per_sec')
CPU_KEYS = ('value', 'unit', 'cores', 'kind', 'sample', 'prove_ms', 'same_bytes_as_gpu', 'host_cpus_visible')
CONFIG_KEYS = ('name', 'prove_ms', 'proof_bytes', 'proof_sha256', 'device_busy_ms', 'verify_native_ms')
CONTRACT_KEYS = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
                 'data', 'config')


def _short(s, n):
    return s if not isinstance(s, str) or len(s) <= n else s[:n - 1] + '~'


def _r(x, nd=4):
    return round(x, nd) if isinstance(x, float) else x


def compact_line(out, detail_name='bench_detail.json'):
    """`out` (everything this run measured) reduced to the record the driver reads: the contract keys, `roofline` and `cpu_baseline` as
    flat objects, the reference's phase log, one row per BASELINE configuration, and (N > 1) one row per one-proof statement.  Returns
    the JSON text, at most LINE_LIMIT bytes: optional blocks are dropped from the end of the list below until it fits."""
    c = {k: out[k] for k in CONTRACT_KEYS if k in out}
    c['metric'] = _short(c.get('metric'), 100)
    c['dtype'] = _short(c.get('dtype'), 24)
    cfg = dict(c.get('config') or {})
    cfg.pop('ntt_points_source', None)
    for k in ('workload', 'parallelism'):
        if k in cfg:
            cfg[k] = _short(cfg[k], 200)
    c['config'] = cfg
    c['value'], c['ms_per_step'] = _r(c.get('value'), 1), _r(c.get('ms_per_step'))
    for k in ('prove_ms', 'driver_total_ms', 'test_double', 'rccl_ranks', 'strong', 'strong_unavailable', 'launcher_note'):
        if k in out:
            c[k] = _short(_r(out[k]), 240)
    rf = out.get('roofline')
    if rf:
        r = {k: _short(rf.get(k), 120) for k in ROOFLINE_KEYS}
        sr = rf.get('second_roof') or {}
        r['second_roof'] = {'bound': sr.get('bound'), 'frac': sr.get('frac')}
        pd = rf.get('proof_dominant_kernel')
        if pd:
            r['proof_dominant_kernel'] = {'kernel': _short(pd.get('kernel'), 40), 'ms_per_proof': pd.get('ms_per_proof'),
                                          'frac_of_compression_roof': pd.get('frac_of_compression_roof'), 'frac_of_hbm_peak': pd.get('frac_of_hbm_peak')}
        c['roofline'] = r
    cpu = out.get('cpu_baseline')
    if cpu:
        c['cpu_baseline'] = {k: _short(_r(cpu.get(k), 1), 200) for k in CPU_KEYS}
    optional = []                                        # dropped last-first when the line would not fit
    pr = out.get('phases_readme')
    if pr and pr.get('ms'):
        c['phases_readme'] = {'ms': [[_short(l, 44), m] for l, m in pr['ms']], 'total_ms': pr.get('total_ms')}
        optional.append('phases_readme')
    if out.get('pipelined'):
        c['pipelined'] = {k: _r(out['pipelined'].get(k), 3) for k in ('lanes', 'proofs', 'ms_per_proof')}
        optional.append('pipelined')
    if out.get('configs'):
        c['configs'] = [({k: _short(x.get(k), 80) for k in CONFIG_KEYS if k in x} if 'error' not in x else {'error': _short(x['error'], 120)})
                        for x in out['configs']]
        optional.append('configs')
    op = out.get('one_proof')
    if op:
        o = {k: _short(op[k], 160) for k in ('error', 'rccl_error', 'rccl_mode', 'gpu_sharing', 'rccl_create_ms', 'rccl_selftest_ms') if k in op}
        if 'comm' in op:
            o['comm'] = _short(op['comm'].get('name'), 80)
        for key in ('c4', 'c4_long', 'c5'):
            if key in op:
                x = op[key]
                o[key] = {'ms_per_proof': x.get('ms_per_proof'), 'single_gpu_ms_per_proof': x.get('single_gpu_ms_per_proof'),
                          'speedup_vs_one_gpu': x.get('speedup_vs_one_gpu'), 'mode': 'solo' if str(x.get('mode', '')).startswith('rank 0') else 'sharded',
                          'same_bytes': x.get('same_bytes_as_the_single_gpu_proof_on_every_rank'), 'verified': x.get('verified'),
                          'collectives': len(x.get('collectives') or []), 'collective_bytes_per_rank': x.get('collective_bytes_per_rank')}
                if x.get('sharded_anyway') and 'ms_per_proof' in x['sharded_anyway']:
                    o[key]['sharded_anyway_ms'] = x['sharded_anyway']['ms_per_proof']
        c['one_proof'] = o
        optional.insert(0, 'one_proof')                  # the scaling record goes last of all
    c['detail'] = detail_name
    line = json.dumps(c, separators=(',', ':'))
    while len(line.encode()) > LINE_LIMIT and optional:
        c.pop(optional.pop())
        c['dropped_to_fit'] = c.get('dropped_to_fit', 0) + 1
        line = json.dumps(c, separators=(',', ':'))
    assert len(line.encode()) <= LINE_LIMIT, len(line)
    return line


def emit(out, detail_path):
    """write everything to `detail_path` (best effort: a read-only tree must not cost the line), then print the compact record as the
    LAST line of stdout"""
    try:
        with open(detail_path, 'w') as fh:
            json.dump(out, fh, indent=1)
    except OSError as e:
        print(f'bench.py: could not write {detail_path}: {e}', file=sys.stderr, flush=True)
    try:
        # whatever native libraries left in C stdio's buffer (RCCL prints a version banner through printf when a communicator is
        # created: on a pipe it would otherwise come out at exit, AFTER the line) goes out first
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:   # noqa: BLE001
        pass
    print(compact_line(out, os.path.basename(detail_path)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--log-trace', type=int, default=20, help='log2 of the MiMC trace length (BASELINE: 20)')
    ap.add_argument('--extension-factor', type=int, default=16)
    ap.add_argument('--fri-queries', type=int, default=64)
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-pmc', action='store_true', help='skip the rocprofv3 child process that measures roofline.traffic')
    ap.add_argument('--no-configs', action='store_true', help='skip the per-configuration runs (tools/config_runs.py: every BASELINE.json config, N = 1 only)')
    ap.add_argument('--sharded-leg-timeout', type=float, default=150.0,
                    help='N > 1 only: seconds allowed for the one-proof-across-all-ranks measurements (0 = skip them: replicas only)')
    ap.add_argument('--c4-log-trace', type=int, default=16, help='N > 1 only: log2 steps of the Poseidon 6-register proof across the ranks (0 = skip)')
    ap.add_argument('--c4-long-log-trace', type=int, default=20, help='N > 1 only: log2 steps of the LONG Poseidon proof across the ranks (16 384 chains at 20; 0 = skip)')
    ap.add_argument('--lanes', type=int, default=8, help='prover lanes of the extra throughput-mode leg (0 = skip it)')
    ap.add_argument('--lane-proofs', type=int, default=48, help='proofs pushed through the lanes in that leg')
    # test-only: drive the distributed harness on CPU (gloo) against the oracle's implementation of the C ABI
    ap.add_argument('--detail', default=os.path.join(ROOT, 'bench_detail.json'), help='where the full record goes (the last stdout line is its summary)')
    ap.add_argument('--test-double-lib', default=None, help=argparse.SUPPRESS)
    # test-only: run the N > 1 flow (process group, one-proof leg over the RCCL communicator) with ONE rank — what a one-GPU box can execute of it
    ap.add_argument('--force-dist', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--full', action='store_true',
                    help='everything beyond the headline figure as well: Python-mirror cross-check and verification, roofline, CPU baseline, '
                         'per-configuration children, phase log, pipelined lanes, and (N > 1) the one-proof leg.  Without it a run sets up, '
                         'warms up, times the steps and prints the line')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step returned (the serialized proof, one float32 per byte) '
                         'as DIR/proof_bytes.npy (rank r > 0: DIR/proof_bytes_rank<r>.npy)')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    cpu_mode = args.test_double_lib is not None
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # `python bench.py --gpus N` without a launcher: become the launcher — one rank per GPU under torch.distributed.run on a free
        # local port; the ranks' stdout (rank 0's one JSON line) passes straight through, the exit code is the launcher's
        sys.exit(self_launch(args.gpus))

    import torch
    import genstark_amd as ga
    from genstark_amd._abi import Backend

    rank = int(os.environ.get('RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    # more ranks than GPUs on this box (a dry run of the N > 1 path on a one-GPU machine): ranks share devices round-robin; RCCL
    # cannot form a communicator over duplicate devices, so the control path is gloo and the one-proof collectives are staged
    # through the host (genstark_amd/comm.py: TorchComm) — reported as `gpu_sharing`, rccl_ranks 0
    ndev = 0 if cpu_mode else torch.cuda.device_count()
    shared_gpus = (not cpu_mode) and world > ndev >= 1
    device_index = local_rank % ndev if shared_gpus else local_rank
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if world == 1:        # --force-dist without a launcher: a one-rank group of this process alone
            import socket
            with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
                so.bind(('127.0.0.1', 0))
                os.environ.setdefault('MASTER_PORT', str(so.getsockname()[1]))
            os.environ.setdefault('RANK', '0')
            os.environ.setdefault('WORLD_SIZE', '1')
        if cpu_mode or shared_gpus:
            dist.init_process_group('gloo')
            if not cpu_mode:
                torch.cuda.set_device(device_index)
        else:
            torch.cuda.set_device(device_index)
            dist.init_process_group('nccl', device_id=torch.device('cuda', device_index))   # nccl == RCCL on ROCm
    else:
        dist = None
        if not cpu_mode:
            torch.cuda.set_device(device_index)
    host_collectives = cpu_mode or shared_gpus          # torch.distributed tensors live on the host (gloo)
    launcher_note = None
    if args.gpus != world:
        # a launcher started a different number of ranks than --gpus says: the ranks that exist are what is measured and reported
        launcher_note = f'--gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks: n_gpus reports the ranks that ran'
        if rank == 0:
            print('bench.py: ' + launcher_note, file=sys.stderr, flush=True)

    if cpu_mode:
        stream = None
        backend = Backend(lib_path=args.test_double_lib, allow_test_double=True)
    else:
        # a non-default torch stream: the library launches every kernel on it, so torch.cuda.Event timings see them
        stream = torch.cuda.Stream()
        torch.cuda.set_stream(stream)
        assert stream.cuda_stream != 0
        backend = Backend(device=device_index, stream=stream.cuda_stream)
    steps, ef, fri = 1 << args.log_trace, args.extension_factor, args.fri_queries
    n = steps * ef
    seed = 3 + rank

    def barrier():
        if not cpu_mode:
            torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        if not cpu_mode:
            torch.cuda.synchronize()

    stark = make_stark(ga, backend, steps, ef, fri)
    a = assertions_for(stark, steps, seed)
    # the product's prove(): the native driver (csrc/prover.cc — lib/Stark.ts:81-163 as C++ above the C ABI); the Python mirror
    # of the same sequence (stark.prove) is timed beside it outside the timed region and must give the same bytes
    from genstark_amd.native import NativeProver
    from genstark_amd.prover import Prover
    # the timed object: Prover = the AIR + options handed straight to the native driver (no mirror object involved)
    prover = Prover(stark.air, {'hashAlgorithm': 'blake2s256', 'extensionFactor': ef, 'exeQueryCount': 48, 'friQueryCount': fri})
    data = None
    for _ in range(args.warmup):
        data = prover.prove_bytes(a, [], [seed])
    # torch's import leaves ~10^6 long-lived Python objects; a generational full collection over them costs tens of ms and
    # would land inside a random timed step.  Move everything alive now to the permanent generation (standard practice for
    # latency-sensitive Python services); objects created by the timed steps are still collected normally.
    import gc
    gc.collect()
    gc.freeze()
    barrier()
    t0 = time.perf_counter()
    step_ms = []
    launched = []
    for _ in range(args.steps):
        ts = time.perf_counter()
        data = prover.prove_bytes(a, [], [seed])
        step_ms.append(round((time.perf_counter() - ts) * 1e3, 3))
        launched.append(prover.last_stats())
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], device='cpu' if host_collectives else 'cuda', dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = elapsed / args.steps * 1e3
    points = launched[-1]['ntt_points']                  # what the timed driver launched as NTT passes, from its own counters
    assert all(st['ntt_points'] == points for st in launched)
    if args.log_trace >= 8:
        assert points == expected_ntt_points(steps, ef), (points, expected_ntt_points(steps, ef))
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, data, rank, world)
    mirror_ms = None
    if args.full:
        proof = stark.parse(data)
        # the Python mirror on the same statement: same bytes, its own wall-clock (not part of `value`)
        mirror_ms = []
        for _ in range(3):
            ts = time.perf_counter()
            mirror_proof = stark.prove(a, [], [seed])
            mirror_ms.append(round((time.perf_counter() - ts) * 1e3, 3))
        assert stark.serialize(mirror_proof) == data, 'native driver and Python mirror disagree'

        # outside the timed region: the proof is valid and the wire format is consistent (reference acceptance criterion)
        assert len(data) == stark.sizeOf(proof)
        if rank == 0 or cpu_mode:
            assert stark.verify(a, stark.parse(data))
        if dist is not None:
            # every rank proved its OWN trace: the evaluation roots must all differ (no rank idled or duplicated work)
            roots = [None] * world
            dist.all_gather_object(roots, proof['evRoot'].hex())
            assert len(set(roots)) == world, 'ranks produced identical proofs'

    out = None
    if rank == 0 and cpu_mode:
        out = {'metric': 'NTT GF(p) elements/sec over whole prove() (MiMC-128)', 'value': points * world / (ms_per_step * 1e-3),
               'unit': 'elements/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': ms_per_step,
               'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'data': 'synthetic', 'test_double': True,
               'config': {'workload': f'MiMC-128 prove(), 2^{args.log_trace} steps', 'ntt_points_per_prove': points}}
    elif rank == 0:
        # ---- per-phase breakdown of the LAST TIMED step, from the native driver's own clock (host wall-clock at its phase
        # boundaries; it adds no device synchronisation, so a phase lasts until its last blocking call returned)
        phases = launched[-1]['phases_ms']
        driver_total_ms = launched[-1]['total_ms']
        out = {
            'metric': 'prove() ms + NTT GF(p) elements/sec, MiMC-128 2^20 steps', 'value': points * world / (ms_per_step * 1e-3),
            'unit': 'elements/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': ms_per_step,
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'u128',
            'metric_note': 'value = NTT points launched per second of whole prove() (two thirds of which is the serial host trace recurrence); prove_ms is the '
                           'other half of the metric; the kernel-level figures are roofline.ntt_kernel_elements_per_sec and pipelined.ms_per_proof',
            'data': 'synthetic',
            'config': {'workload': f'MiMC-128 prove(), 2^{args.log_trace} steps, extensionFactor {ef}, exeQueryCount 48, '
                                   f'friQueryCount {fri}, blake2s256; one independent proof per GPU',
                       'secret_registers': 0, 'field': 'GF(2^128-9*2^32+1): 4x u32 limbs in memory, 5x 26-bit limbs inside the NTT networks',
                       'evaluation_domain': n, 'ntt_points_per_prove': points, 'ntt_transforms_per_prove': launched[-1]['ntt_transforms'],
                       'ntt_points_source': 'gs_prover_last_stats: rows * n of every transform the timed driver launched', 'proof_bytes': len(data)},
            'prove_ms': ms_per_step, 'per_step_ms': step_ms, 'phases_ms': phases, 'phases_source': 'native driver clock, last timed step', 'driver_total_ms': driver_total_ms,
        }
        if args.full:
            # ---- roofline of the dominant kernel: one radix-256 NTT pass over n = T*E points
            import ctypes as C
            f = stark.air.field
            w = f.getRootOfUnity(n)
            src = f.getPowerSeries(0x123456789abcdef0123456789, n)
            dst = f.newVector(n)
            wb = w.to_bytes(16, 'little')
            call = lambda: backend.call('gs_eval_polys_at_roots', C.c_void_p(src.ptr), 1, n, wb, n, C.c_void_p(dst.ptr))
            call()
            torch.cuda.synchronize()
            reps = 20
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                call()
            e1.record(stream)
            e1.synchronize()
            logn = n.bit_length() - 1
            npass = (logn + 7) // 8
            transform_ms = e0.elapsed_time(e1) / reps
            launch_ms = transform_ms / npass
            # algorithmic bytes: 32 B per element per transform -> one pass launch does 1/npass of a transform
            alg_bytes_per_launch = 32.0 * n / npass
            achieved = alg_bytes_per_launch / (launch_ms * 1e-3) / 1e9
            # counter passes and the CPU baseline run on rank 0 at N = 1 only: at N > 1 the other ranks are waiting at the one-proof leg below
            traffic, traffic_detail = (None, {'skipped': True}) if (args.no_pmc or world > 1) else pmc_traffic(logn)
            roofline = {'bound': 'hbm', 'achieved': round(achieved, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                        'frac': round(achieved / HBM_PEAK_GBS, 4), 'traffic': traffic,
                        'traffic_source': 'rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE child processes of this run (tools/pmc_traffic.py)',
                        'traffic_detail': traffic_detail,
                        'kernel': f'k_ntt_wave<4, *> (radix-256 Stockham pass, one wave per tile, lazy five-limb butterflies), {npass} launches per 2^{logn}-point transform',
                        'launch_ms': round(launch_ms, 4), 'transform_ms': round(transform_ms, 4),
                        'ntt_kernel_elements_per_sec': round(n / (transform_ms * 1e-3), 1),
                        'second_roof': second_roof(n, transform_ms, npass, traffic_detail)}
            del src, dst

            def gpu_digest(log_steps, ef_, exe, fri_, _cache={}):
                key = (log_steps, ef_, exe, fri_)
                if key not in _cache:
                    import hashlib
                    if key == (args.log_trace, ef, 48, fri) and seed == 3:
                        blob = data                                    # the timed proof itself
                    else:
                        st_ = ga.instantiateMimc(1 << log_steps, {'hashAlgorithm': 'blake2s256', 'extensionFactor': ef_, 'exeQueryCount': exe, 'friQueryCount': fri_}, backend=backend)
                        blob = Prover(st_.air, {'hashAlgorithm': 'blake2s256', 'extensionFactor': ef_, 'exeQueryCount': exe, 'friQueryCount': fri_}).prove_bytes(
                            assertions_for(st_, 1 << log_steps, 3), [], [3])
                    _cache[key] = hashlib.sha256(blob).hexdigest()
                return _cache[key]

            cpu = None if (args.no_cpu_baseline or world > 1) else cpu_baseline(ga, ef, fri, gpu_digest)

            # ---- every BASELINE.json configuration through the product entry (compiled programs, packed seeds), driver-run: wall-clock per
            # proof, device-busy time and launches per proof (rocprofv3 --kernel-trace of a second child), the reference's own phase log
            # with device-synchronised times.  Child processes of this run (tools/config_runs.py); N = 1 only
            configs = None
            if not args.no_configs and world == 1:
                import subprocess
                try:
                    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'config_runs.py')], capture_output=True, text=True, timeout=600)
                    configs = json.loads([l for l in r.stdout.splitlines() if l.startswith('[')][-1])
                except Exception as e:   # noqa: BLE001
                    configs = [{'error': repr(e)[:300]}]
            # the kernel that dominates the PROOF (the NTT pass above dominates the transform metric, not the proof): from the C5 run
            c5 = next((c for c in (configs or []) if c.get('name') == 'C5' and c.get('dominant_kernel')), None)
            if c5 is not None:
                ms_k = c5['dominant_kernel_ms_per_proof']
                fused_leaves = 'k_merkle_fused<1, 1>' in c5['dominant_kernel']
                comp = n * 1.875 if fused_leaves else None        # 2^24 leaf hashes + the three node layers above them in the same launch
                roofline['proof_dominant_kernel'] = {
                    'kernel': c5['dominant_kernel'], 'ms_per_proof': ms_k, 'share_of_device_busy_time': c5['dominant_share'],
                    'device_busy_ms_per_proof': c5['device_busy_ms'],
                    'what': 'evaluation-tree commitment: mergeVectorRows + the first three node layers in one launch (lib/Stark.ts:113-118)' if fused_leaves else None,
                    'bound': 'blake2s compression issue rate (39.5 G compressions/s chip-wide, tools/microbench_hash.hip), not HBM',
                    'compressions_per_sec': None if comp is None else round(comp / (ms_k * 1e-3), 1),
                    'frac_of_compression_roof': None if comp is None else round(comp / (ms_k * 1e-3) / 39.5e9, 4),
                    'algorithmic_GBs': None if comp is None else round(n * (16 + 32 + 28) / (ms_k * 1e-3) / 1e9, 1),
                    'frac_of_hbm_peak': None if comp is None else round(n * (16 + 32 + 28) / (ms_k * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            # every kernel of the headline proof and of the long Poseidon proof against its roof (tools/config_runs.py: kernel_table): the
            # kernel trace of the configuration's own child run joined with the library's tally of what each launch had to move
            roofline['kernels'] = {c_['name']: c_.pop('kernels') for c_ in (configs or []) if c_.get('name') in ('C5', 'C4_long') and c_.get('kernels')}
            roofline['kernels_note'] = ('per proof: calls and ms from rocprofv3 --kernel-trace of the configuration\'s child run; algorithmic_MB = the bytes the launches HAD to '
                                        'read once and write once (gs_traffic_enable: tallied by the library per launch from its arguments — an NTT pass 16 B in + 16 B out '
                                        'per element, a Merkle layer 64 B in + 32 B out per node, ...); frac_hbm against 8 TB/s; frac_own_roof where the kernel\'s own roof '
                                        'is known (BLAKE2s compression issue 39.5 G/s; NTT passes: issue time of their static VALU mix)')
            for c_ in (configs or []):
                c_.pop('kernels', None)
            # the reference's phase vocabulary for the headline proof (README.md:62-73; lib/Stark.ts:92-152), device-synchronised
            prover.sync_phases(True)
            prover.prove_bytes(a, [], [seed])
            phases_readme = prover.last_stats().get('phases_readme')
            prover.sync_phases(False)

            # ---- extra leg (reported beside `value`, never as `value`): throughput of a proving service that keeps several
            # independent proofs in flight on this GPU (genstark_amd/pipeline.py); every proof runs the unmodified prove()
            pipelined = None
            if args.lanes > 0 and world == 1:
                from genstark_amd.pipeline import ProverPool
                job = (a, [], [seed])
                with ProverPool(lambda be: ga.mimcProver(steps, {'hashAlgorithm': 'blake2s256', 'extensionFactor': ef, 'exeQueryCount': 48, 'friQueryCount': fri}, backend=be), lanes=args.lanes,
                                backend_factory=lambda: Backend(device=device_index), native=True) as pool:
                    for _ in range(max(args.warmup, 1)):
                        pool.on_every_lane(lambda s: s.prove_bytes(*job))
                    tp = time.perf_counter()
                    proofs = pool.prove_many_bytes([job] * args.lane_proofs)
                    dt = time.perf_counter() - tp
                    assert all(pr == data for pr in proofs)                        # same statement -> same bytes as the timed steps
                pipelined = {'lanes': args.lanes, 'proofs': args.lane_proofs, 'ms_per_proof': round(dt / args.lane_proofs * 1e3, 3),
                             'value': points * args.lane_proofs / dt, 'unit': 'elements/s',
                             'note': 'independent proofs in flight on one GPU (one library context + HIP stream per lane): a lane\'s '
                                     'host-side trace recurrence overlaps the other lanes\' kernels; latency of one proof is prove_ms'}
            out.update({'python_mirror_prove_ms': mirror_ms, 'roofline': roofline, 'cpu_baseline': cpu, 'pipelined': pipelined,
                        'phases_readme': {'ms': phases_readme, 'total_ms': None if not phases_readme else round(sum(m for _, m in phases_readme), 4),
                                          'note': 'the reference\'s own log points (README.md:62-73, lib/Stark.ts:92-152) on ONE extra proof of the headline statement '
                                                  'with the device synchronised at each of them (gs_prover_sync_phases): each entry is that phase alone; the timed '
                                                  'proofs above run asynchronously and overlap them (phases_ms)'},
                        'configs': configs})
    # ---- N > 1.  `value` stays the BASELINE metric on the BASELINE workload with one independent MiMC-128 proof per GPU (weak
    # scaling, no data-path collective: a single MiMC proof is bounded by the serial trace recurrence of its one register, SURVEY 8e
    # "Fallback").  Beside it, the `one_proof` object: ONE proof across all ranks through the native distributed driver
    # (csrc/prover_dist.h, gs_prover_prove_dist) over RCCL (csrc/comm_rccl.cc) — C4 (BASELINE configs[3]: Poseidon, 6 registers,
    # 2^16 steps = 1 024 hash chains, trace generation sharded by segment) is the strong-scaling measurement, with the same proof on
    # ONE GPU timed in the same run; C5 (the headline statement as one proof) is reported with it.  Every collective is listed with
    # its bytes and device time.  The leg runs under a watchdog: whatever happens in it, every rank leaves within
    # --sharded-leg-timeout seconds and rank 0 still prints ONE valid line.
    if out is not None and launcher_note:
        out['launcher_note'] = launcher_note
    if dist is not None and args.full and args.sharded_leg_timeout > 0:
        import hashlib
        import threading
        result = {}

        def timed_dist(nat, a0, inputs, sd, comm_obj, reps):      # nat: a Prover
            comm = comm_obj.comm
            nat.prove_bytes(a0, inputs, sd, comm=comm)                            # warm-up: plans, block cache, RCCL channels
            nat.prove_bytes(a0, inputs, sd, comm=comm)                            # ... and the proof whose collectives are reported with their device times
            colls = nat.last_collectives()
            if hasattr(comm_obj, 'timings'):
                comm_obj.timings(False)                                           # the timed proofs carry no event records on the stream
            barrier()
            ts = time.perf_counter()
            for _ in range(reps):
                blob = nat.prove_bytes(a0, inputs, sd, comm=comm)
            barrier()
            ms = (time.perf_counter() - ts) / reps * 1e3
            if hasattr(comm_obj, 'timings'):
                comm_obj.timings(True)
            t = torch.tensor([ms], device='cpu' if host_collectives else 'cuda', dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            digests = [None] * world
            dist.all_gather_object(digests, hashlib.sha256(blob).hexdigest())          # verification only, not on the data path
            for c in colls:
                # xGMI is point to point: in an all-gather every peer's piece (`bytes`) arrives over its own link, in an all-to-all every
                # pair exchanges `bytes` over its own link — so bytes / device time is the rate PER LINK (peak ~64 GB/s per direction)
                c['GBs_per_link'] = None if not c.get('ms') else round(c['bytes'] / (c['ms'] * 1e-3) / 1e9, 2)
            return float(t[0]), blob, len(set(digests)) == 1, colls, nat.last_stats()

        def mode_of(colls):
            # what the distributed driver did with the statement (gs_comm::solo_below, include/gstark_comm.h)
            return 'rank 0 alone, bytes delivered to every rank (fewer than 2^20 evaluation-domain points per rank: not worth a collective)' \
                if colls and colls[0]['label'].startswith('solo') else 'sharded over the ranks'

        def leg():
            try:
                if not cpu_mode:
                    torch.cuda.set_device(device_index)      # the HIP current device is per-thread state
                    torch.cuda.set_stream(stream)
                from genstark_amd.comm import RcclComm, TorchComm
                comm = None
                if not host_collectives:
                    # the product communicator: RCCL on the library's device buffers.  It is checked with known patterns first (both
                    # collectives, every rank); if any rank cannot create it or sees wrong bytes, ALL ranks fall back to collectives
                    # staged through the host over a gloo group, so that the strong-scaling figures still exist — and say so
                    # Three forms of the RCCL communicator are tried in turn, each on a fresh communicator, every rank taking the same decision
                    # (the errors are all-gathered): as built (ncclAllToAll; collectives may be forked onto the communicator's own stream),
                    # without the overlap, and with the grouped ncclSend / ncclRecv exchange as well.  `rccl_mode` says which one ran.
                    attempts = [('alltoall + overlap', {}), ('alltoall, in stream order', {'GSTARK_RCCL_NO_OVERLAP': '1'}),
                                ('grouped send/recv, in stream order', {'GSTARK_RCCL_NO_OVERLAP': '1', 'GSTARK_RCCL_GROUPED_ALLTOALL': '1'})]
                    tried = []
                    for mode, env_extra in attempts:
                        rccl_error = None
                        for k in ('GSTARK_RCCL_NO_OVERLAP', 'GSTARK_RCCL_GROUPED_ALLTOALL'):
                            os.environ.pop(k, None)
                        os.environ.update(env_extra)                   # (read by gs_rccl_comm_create, csrc/comm_rccl.cc)
                        try:
                            uid = [RcclComm.unique_id() if rank == 0 else None]
                            dist.broadcast_object_list(uid, src=0)                          # control path: 128 bytes
                            t_rccl = time.perf_counter()
                            comm = RcclComm(backend, rank, world, uid[0])
                            result['rccl_create_ms'] = round((time.perf_counter() - t_rccl) * 1e3, 1)
                            t_rccl = time.perf_counter()
                            rccl_error = comm_selftest(backend, comm.comm, rank, world)
                            result['rccl_selftest_ms'] = round((time.perf_counter() - t_rccl) * 1e3, 1)
                        except Exception as e:   # noqa: BLE001
                            rccl_error = repr(e)[:200]
                        errs = [None] * world
                        dist.all_gather_object(errs, rccl_error)
                        if not any(errs):
                            result['rccl_mode'] = mode
                            break
                        tried.append(f'{mode}: {next(e for e in errs if e)}')
                        if comm is not None:
                            try:
                                comm.close()
                            except Exception:   # noqa: BLE001
                                pass
                        comm = None
                    if tried:
                        result['rccl_error'] = '; '.join(tried)[:400]
                if comm is None:
                    group = dist.new_group(backend='gloo') if not host_collectives else None
                    comm = TorchComm(backend, group=group)
                    err = comm_selftest(backend, comm.comm, rank, world)
                    if err:
                        raise RuntimeError('host-staged collectives failed their self-test: ' + err)
                is_rccl = isinstance(comm, RcclComm)
                result['comm'] = {'name': 'rccl' if is_rccl else ('torch.distributed (test double run)' if cpu_mode else
                                                                   'torch.distributed gloo, device buffers staged through the host'), 'ranks': world,
                                  'selftest': 'all_gather + all_to_all of rank-stamped patterns: ok'}
                if shared_gpus:
                    result['gpu_sharing'] = f'{world} ranks on {ndev} GPU(s): a dry run of the N > 1 path, not a scaling measurement'
                result['rccl_ranks'] = world if is_rccl else 0
                result['HSA_ENABLE_IPC_MODE_LEGACY'] = os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')

                def sharded_anyway(nat, a0, inputs, sd, reps, single_blob):
                    # the same statement with the bar off (solo_below = 1): what sharding a proof this small costs — reported beside the
                    # driver's own choice, never instead of it
                    comm.comm.solo_below = 1
                    try:
                        ms_f, blob_f, same_f, colls_f, st_f = timed_dist(nat, a0, inputs, sd, comm, reps)
                    except Exception as e:   # noqa: BLE001  (an extra: it must not take the statement's own record down)
                        return {'error': repr(e)[:200]}
                    finally:
                        comm.comm.solo_below = 0
                    return {'ms_per_proof': round(ms_f, 3), 'same_bytes_as_the_single_gpu_proof_on_every_rank': bool(same_f and blob_f == single_blob),
                            'phases_ms': st_f['phases_ms'], 'collectives': colls_f,
                            'collective_bytes_per_rank': sum(c['bytes'] * (world if c['kind'] == 'all_to_all' else 1) for c in colls_f)}
                # C4 (BASELINE configs[3]): Poseidon 6x128, 2^16 steps as 1 024 independent 64-step hash chains, E = 16 — and the same AIR
                # at 2^20 steps (16 384 chains): the 2^16-step statement is latency-bound on ONE GPU already (2.1 ms inside the driver), the
                # long one is where the shards have work to do.  First rows are packed before the timed region (inputs resident).
                from genstark_amd.poseidon import poseidon6x128_air
                from genstark_amd.prover import Prover
                if hasattr(backend, 'jit') and not cpu_mode:
                    backend.jit()      # a proving service compiles an AIR's programs once (hiprtc, ~1 s each); the warm-up proofs below pay for it
                for key, log_t4 in (('c4', args.c4_log_trace), ('c4_long', args.c4_long_log_trace)):
                    if log_t4 <= 0:
                        continue
                    t4 = 1 << log_t4
                    opts4 = {'hashAlgorithm': 'blake2s256', 'extensionFactor': 16, 'exeQueryCount': 48, 'friQueryCount': 24}
                    p4 = Prover(poseidon6x128_air(t4, 16, stark.air.field, segmented=True), opts4)
                    seed4 = p4.pack_seed([[1 + s_, 2, 3 + s_, 4] for s_ in range(t4 // 64)])
                    a4 = [{'step': 0, 'register': 0, 'value': 1}, {'step': 64 * (t4 // 64 - 1), 'register': 2, 'value': 3 + t4 // 64 - 1}]   # first rows of the first / last chain
                    single = p4.prove_bytes(a4, [], seed4)                                  # the same statement on ONE GPU (every rank, concurrently)
                    reps4 = max(3, args.steps)
                    barrier()
                    ts = time.perf_counter()
                    for _ in range(reps4):
                        single = p4.prove_bytes(a4, [], seed4)
                    single_ms = (time.perf_counter() - ts) / reps4 * 1e3
                    ms4, blob4, same4, colls4, st4 = timed_dist(p4, a4, [], seed4, comm, reps4)
                    verified4 = None if t4 > (1 << 16) else (rank != 0 or bool(p4.verify(a4, blob4)))   # the long statement is not verified here (host verifier: seconds)
                    ok4 = same4 and blob4 == single and verified4 is not False
                    forced4 = sharded_anyway(p4, a4, [], seed4, reps4, single) if colls4 and colls4[0]['label'].startswith('solo') else None
                    result[key] = {'workload': f'Poseidon 6x128, 2^{log_t4} steps = {t4 // 64} hash chains, E=16, exe 48, fri 24, blake2s256',
                                   'mode': mode_of(colls4), 'sharded_anyway': forced4,
                                   'ms_per_proof': round(ms4, 3), 'single_gpu_ms_per_proof': round(single_ms, 3),
                                   'speedup_vs_one_gpu': round(single_ms / ms4, 3), 'ranks': world, 'proofs_timed': reps4, 'proof_bytes': len(blob4),
                                   'scaling': 'strong', 'air_programs': 'compiled (gs_air_jit)' if not cpu_mode else 'interpreted', 'phases_ms': st4['phases_ms'], 'collectives': colls4,
                                   'collective_bytes_per_rank': sum(c['bytes'] * (world if c['kind'] == 'all_to_all' else 1) for c in colls4),
                                   'same_bytes_as_the_single_gpu_proof_on_every_rank': bool(same4 and blob4 == single), 'verified': verified4,
                                   'same_bytes_as_the_single_gpu_proof_on_every_rank_and_verified': bool(ok4) if verified4 is not None else None}
                # C5: the headline statement as ONE proof (every rank the same seed)
                a0 = assertions_for(stark, steps, 3)
                want = prover.prove_bytes(a0, [], [3])
                ms, blob, same, colls, st5 = timed_dist(prover, a0, [], [3], comm, args.steps)
                ok = same and blob == want and (rank != 0 or stark.verify(a0, stark.parse(blob)))
                forced5 = sharded_anyway(prover, a0, [], [3], args.steps, want) if colls and colls[0]['label'].startswith('solo') else None
                result['c5'] = {'workload': f'MiMC-128 2^{args.log_trace} steps, E={ef}: ONE proof across {world} ranks', 'ms_per_proof': round(ms, 3),
                                'mode': mode_of(colls), 'sharded_anyway': forced5,
                                'ranks': world, 'proofs_timed': args.steps, 'proof_bytes': len(blob), 'scaling': 'strong',
                                'phases_ms': st5['phases_ms'], 'collectives': colls,
                                'note': 'bounded from below by the serial x^3 + k recurrence of the one trace register (replicated on every rank)',
                                'same_bytes_as_the_single_gpu_proof_on_every_rank': bool(same and blob == want), 'verified': True if ok else False,
                                'same_bytes_as_the_single_gpu_proof_on_every_rank_and_verified': bool(ok)}
            except BaseException as e:                                          # never take the main line down
                result['error'] = repr(e)[:300]

        barrier()                  # every rank starts its watchdog at the same moment (rank 0 has just measured the roofline)
        th = threading.Thread(target=leg, daemon=True)
        th.start()
        th.join(args.sharded_leg_timeout)
        snap = dict(result)                    # the leg may still be running: report what it had at the deadline, ignore later writes
        if th.is_alive():
            snap['error'] = f'timed out after {args.sharded_leg_timeout} s'
        if out is not None:
            out['config']['parallelism'] = (f'value: {world} independent proofs, one per GPU (no data-path collective). one_proof: the evaluation domain '
                                            f'strided over {world} ranks — coset NTTs, constraint evaluation, pointwise work and FRI folds local; trace '
                                            'segments generated by their owners; per Merkle tree one all-to-all of leaf digests + one all-gather of '
                                            'sub-roots; all query answers in one all-gather; native driver (csrc/prover_dist.h) over RCCL on device buffers')
            out['one_proof'] = snap
            out['rccl_ranks'] = snap.get('rccl_ranks')
            # strong scaling in one object: the longest statement that ran as ONE proof across the ranks, beside the same proof on one GPU
            sk = next((k for k in ('c4_long', 'c4') if k in snap), None)
            # ... and ONLY when the collectives were RCCL over as many ranks as GPUs: with the host-staged fallback (or ranks sharing a GPU)
            # one_proof.*.ms_per_proof stay as a record of what ran, but they are not a scaling measurement and must not read as one
            strong_ok = sk is not None and snap.get('rccl_ranks') == world and not shared_gpus
            out['strong_unavailable'] = None if strong_ok else (
                'no one-proof statement ran' if sk is None else
                f'rccl_ranks = {snap.get("rccl_ranks")} of {world} ranks' + (f' ({snap["rccl_error"]})' if snap.get('rccl_error') else '') +
                (f'; {snap["gpu_sharing"]}' if snap.get('gpu_sharing') else '') +
                ': the collectives were staged through the host, so the one-proof times are a dry run, not strong scaling')
            out['strong'] = None if not strong_ok else {
                'workload': snap[sk]['workload'], 'key': sk, 'ms_1gpu': snap[sk]['single_gpu_ms_per_proof'], 'ms_Ngpu': snap[sk]['ms_per_proof'],
                'speedup': snap[sk]['speedup_vs_one_gpu'], 'ranks': world, 'same_bytes': snap[sk]['same_bytes_as_the_single_gpu_proof_on_every_rank'],
                'note': 'ONE proof across all ranks (csrc/prover_dist.h over RCCL) against the same proof on one GPU, both timed in this run; '
                        '`value` above is the replica figure (one independent proof per GPU)'}
            out['collectives'] = (snap.get('c4_long') or snap.get('c4') or snap.get('c5') or {}).get('collectives', [])
            emit(out, args.detail)
        sys.stdout.flush()
        os._exit(0)      # the line is out; a rank may be stuck in (or may have bailed out of) a collective of the extra leg, so no
                         # rank waits for the others in a final barrier
    elif out is not None:
        emit(out, args.detail)
        out = None
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
