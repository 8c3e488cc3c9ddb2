"""Statements and driver helpers shared by tests/test_boundary_many_assertions.py, its workers and the tools that regenerate its golden
proof / measure the verifier (tools/make_many_assertions_golden.py, tools/boundary_host_bench.py).  Not a test module."""
import os
import random

from genstark_amd import _abi
from genstark_amd.native import NativeProver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPTS = {'hashAlgorithm': 'blake2s256', 'extensionFactor': 16, 'exeQueryCount': 24, 'friQueryCount': 12}
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'many_assertions_quintic_2p13.proof')


def quintic_air(field, steps):
    """the two-register degree-5 AIR of tests/runtime_modulus_worker.py"""
    from genstark_amd.air_generic import GenericAir
    ks = [[(7 * i + 3) % field.modulus for i in range(8)]]
    return GenericAir(steps, 2, [5, 5], ks, lambda r, k: [(r[0] + k[0]) ** 5 + r[1], r[0] + 2 * r[1]],
                      lambda r, n, k: [n[0] - ((r[0] + k[0]) ** 5 + r[1]), n[1] - (r[0] + 2 * r[1])], lambda seed: [seed[0], seed[1]], None, field)


def quintic_trace(p, steps, seed):
    """the same recurrence on Python integers: rows of [r0, r1]"""
    rows, r = [], list(seed)
    for i in range(steps):
        rows.append(r)
        k = (7 * (i % 8) + 3) % p
        r = [(pow(r[0] + k, 5, p) + r[1]) % p, (r[0] + 2 * r[1]) % p]
    return rows


def golden_statement(p, steps=1 << 13):
    """5 000 assertions on register 0, three on register 1 (the statement of GOLDEN; tools/make_many_assertions_golden.py proves it)"""
    rows = quintic_trace(p, steps, [5, 9])
    rng = random.Random(5000)
    at = sorted(rng.sample(range(steps), 5000))
    return [{'step': s, 'register': 0, 'value': rows[s][0]} for s in at] + [{'step': s, 'register': 1, 'value': rows[s][1]} for s in (0, 77, steps - 1)]


class Statement:
    def __init__(self, air, opts=OPTS):
        self.air, self.exeQueryCount, self.friQueryCount = air, opts['exeQueryCount'], opts['friQueryCount']
        self.hashAlg = _abi.HASH_ALGS[opts['hashAlgorithm']]


class HostFieldShim:
    """what NativeProver.boundary_at reads of a field"""

    def __init__(self, modulus, element_size):
        self.modulus, self.elementSize = modulus, element_size

    def le(self, v):
        return int(v).to_bytes(self.elementSize, 'little')


def host_driver(modulus):
    """The native driver bound to the HOST-side entry points of the product library of a field flavour (gs_small_interpolate needs no
    device and no context; the library loads without a GPU): what gs_prover_boundary_at_on needs."""
    from genstark_amd.native import _driver

    class _Lib:
        pass
    be = _Lib()
    be.lib = _abi.load_library(_abi.HIP_LIB_PATHS[modulus])
    be.modulus, be.element_size = modulus, be.lib.gs_element_size()
    nat = NativeProver.__new__(NativeProver)
    nat.lib, nat.binding = _driver(be)
    nat.field = HostFieldShim(modulus, be.element_size)
    return nat


def root_of_unity(p, order):
    """an element of exactly that (power-of-two) order"""
    e = (p - 1) // order
    for g in range(2, 1000):
        w = pow(g, e, p)
        if pow(w, order // 2, p) == p - 1:
            return w
    raise AssertionError('no root found')


def rescue_statement(f, chains=2048):
    """C3-shaped: Rescue 4x128, 32 steps per chain; every chain's first and last row asserted on all four registers (2 * chains assertions
    on each of four registers).  -> (air, assertions, seeds)"""
    from genstark_amd.hostfield import HostField
    from genstark_amd.rescue import rescue4x128_air
    seeds = [[42 + s, 43 + 2 * s] for s in range(chains)]
    hf = HostField(f.modulus)
    one = rescue4x128_air(32, 16, hf, segmented=True)         # a chain's values do not depend on how many chains there are
    a = []
    for s, seed in enumerate(seeds):
        tr = one.hostTrace([seed])
        for step in (0, 31):
            a += [{'step': 32 * s + step, 'register': r, 'value': tr[step][r]} for r in range(4)]
    return rescue4x128_air(32 * chains, 16, f, segmented=True), a, seeds


def poseidon_statement(f, chains=16384):
    """C4-long-shaped: Poseidon 6x128, 64 steps per chain; every chain's output (register 0 of its last row) asserted: `chains` assertions
    on one register.  -> (air, assertions, seeds)"""
    from genstark_amd.hostfield import HostField
    from genstark_amd.poseidon import poseidon6x128_air
    seeds = [[1 + s, 2, 3 + s, 4] for s in range(chains)]
    hf = HostField(f.modulus)
    one = poseidon6x128_air(64, 16, hf, segmented=True)
    a = [{'step': 64 * s + 63, 'register': 0, 'value': one.hostTrace([seed])[63][0]} for s, seed in enumerate(seeds)]
    return poseidon6x128_air(64 * chains, 16, f, segmented=True), a, seeds


def quad_air(field, steps):
    """a four-register AIR for statements that assert three or four registers: the quintic pair twice, side by side"""
    from genstark_amd.air_generic import GenericAir
    ks = [[(7 * i + 3) % field.modulus for i in range(8)]]
    return GenericAir(steps, 4, [5, 5, 5, 5], ks,
                      lambda r, k: [(r[0] + k[0]) ** 5 + r[1], r[0] + 2 * r[1], (r[2] + k[0]) ** 5 + r[3], r[2] + 2 * r[3]],
                      lambda r, n, k: [n[0] - ((r[0] + k[0]) ** 5 + r[1]), n[1] - (r[0] + 2 * r[1]), n[2] - ((r[2] + k[0]) ** 5 + r[3]), n[3] - (r[2] + 2 * r[3])],
                      lambda seed: list(seed), None, field)


def quad_trace(p, steps, seed):
    return [x + y for x, y in zip(quintic_trace(p, steps, seed[:2]), quintic_trace(p, steps, seed[2:]))]
