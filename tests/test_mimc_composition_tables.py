"""gs_mimc_composition from per-point tables (include/gstark_mimc.h, csrc/air_mimc.hip): gs_mimc_composition_prepare builds X, U and IU
before the trace, gs_mimc_composition_tables reads them.  The reference is gs_mimc_composition on the same device and the same inputs
(itself checked against Python integers and the oracle in test_gpu_parity.py); this is exact field arithmetic, so every output byte
must be equal.  Which kernels ran is read from the library's own tally (gs_traffic_enable), so no case passes through the fallback
unnoticed."""
import ctypes as C
import itertools
import os
import random

import pytest

from conftest import P, ROOT, rand_elements, to_bytes
from genstark_amd import _abi

pytestmark = pytest.mark.gpu

OLD, NEW = 'k_mimc_composition', 'k_mimc_composition_tables'
TABLE_KERNELS = ('k_mimc_table_x', 'k_mimc_table_u', 'k_mimc_table_iu')
# csrc/ntt.hip (plan_get): the power table of a domain is split into omega^i, i < 2^12, and omega^(i << 12); gs_mimc_composition takes
# its tw_hi branch above that, so 2^13 is the smallest domain at which the reference computes its points that way
LOG_LO = 12


def launches(tally):
    return {k: v['launches'] for k, v in tally.items() if k == OLD or k == NEW or k in TABLE_KERNELS}


def asserted_steps(steps, nroots):
    """step 0; step steps - 1, where (i - root) mod n wraps; two adjacent steps"""
    return {1: [steps - 1], 2: [0, steps - 1], 3: [0, 1, steps - 1], 4: [0, steps - 1, 5, 6]}[nroots]


def composition_args(f, rng, vp, vk, klen, n, steps, roots, with_lc, incs):
    q_inc, b_inc = (steps, 2 * steps) if incs else (0, 0)
    args = (C.c_void_p(vp.ptr), n, steps, f.le(f.getRootOfUnity(n)), C.c_void_p(vk.ptr), klen, to_bytes(rng.randrange(P) for _ in range(4)), q_inc, b_inc,
            to_bytes(rng.randrange(P) for _ in roots), (C.c_uint64 * len(roots))(*roots), len(roots))
    return args, (to_bytes(rng.randrange(P) for _ in range(2)) if with_lc else None)


def both_paths(be, f, args, lc, n):
    """(gs_mimc_composition, prepare + gs_mimc_composition_tables) on the same arguments -> the two output buffers"""
    _, _, steps, w, _, _, _, _, _, ipoly, roots, nroots = args
    old, new = f.newVector(n), f.newVector(n)
    be.call('gs_mimc_composition', *args, lc, C.c_void_p(old.ptr))
    be.call('gs_mimc_composition_prepare', n, steps, w, roots, nroots, ipoly)
    be.call('gs_mimc_composition_tables', *args, lc, C.c_void_p(new.ptr))
    return old.toBuffer(), new.toBuffer()


def test_entry_points_are_optional(hip_backend):
    """declared in their own header, not among the mandatory symbols of include/gstark.h; the HIP library has them"""
    assert set(_abi.MIMC_SYMBOLS).isdisjoint(_abi.EXPORTED_SYMBOLS) and set(_abi.MIMC_SYMBOLS).isdisjoint(_abi.OPTIONAL_SYMBOLS)
    header = open(os.path.join(ROOT, 'include', 'gstark_mimc.h')).read()
    for name in _abi.MIMC_SYMBOLS:
        assert name + '(' in header
        assert hasattr(hip_backend.lib, name)


@pytest.mark.parametrize('period', [2, 16, 32])
@pytest.mark.parametrize('logn', [10, 12, LOG_LO + 1])
def test_table_path_equals_table_free_pass(hip_backend, logn, period):
    """1..4 assertions x with / without the folded linear combination x zero / non-zero degree increments, per size and n / steps"""
    from genstark_amd.field import PrimeField
    be, f = hip_backend, PrimeField(backend=hip_backend)
    rng = random.Random(1000 * logn + period)
    n = 1 << logn
    steps = n // period
    klen = 64
    vp, vk = f.newVectorFrom(rand_elements(rng, n)), f.newVectorFrom(rand_elements(rng, klen))
    for nroots, with_lc, incs in itertools.product((1, 2, 3, 4), (False, True), (False, True)):
        at = asserted_steps(steps, nroots)
        roots = [s * period for s in at]
        args, lc = composition_args(f, rng, vp, vk, klen, n, steps, roots, with_lc, incs)
        be.traffic(True)
        old, new = both_paths(be, f, args, lc, n)
        ran = launches(be.traffic())
        be.traffic(False)
        assert ran[OLD] == 1 and ran[NEW] == 1 and ran['k_mimc_table_iu'] == 1, ran
        # the asserted points: U = 0 and IU = 0 there (the u table's 0^-1 = 0), so the boundary term vanishes as it does in the reference
        for r in roots:
            assert new[16 * r:16 * r + 16] == old[16 * r:16 * r + 16], (nroots, with_lc, incs, r)
        assert new == old, (nroots, with_lc, incs)


def test_single_assertion_at_step_zero_and_a_cyclic_register_of_odd_length(hip_backend):
    """one root at index 0 (no wrap at all), and a k table whose length is no power of two (the pass then indexes it by division)"""
    from genstark_amd.field import PrimeField
    be, f = hip_backend, PrimeField(backend=hip_backend)
    rng = random.Random(77)
    n, steps, klen = 1 << 12, 1 << 8, 48
    vp, vk = f.newVectorFrom(rand_elements(rng, n)), f.newVectorFrom(rand_elements(rng, klen))
    for roots in ([0], [0, 16 * 255]):
        args, lc = composition_args(f, rng, vp, vk, klen, n, steps, roots, True, True)
        old, new = both_paths(be, f, args, lc, n)
        assert new == old


def test_grid_stride_at_2p20(hip_backend):
    """more points than one sweep of the grid (2048 workgroups of 256): the loops of the three table kernels and of the pass"""
    from genstark_amd.field import PrimeField
    be, f = hip_backend, PrimeField(backend=hip_backend)
    rng = random.Random(2020)
    n, steps = 1 << 20, 1 << 16
    vp, vk = f.getPowerSeries(0xfedcba9876543210fedcba987654321, n), f.newVectorFrom(rand_elements(rng, 64))
    args, lc = composition_args(f, rng, vp, vk, 64, n, steps, [0, 16 * (steps - 1), 16 * 7], True, True)
    old, new = both_paths(be, f, args, lc, n)
    assert new == old


def test_tables_are_kept_per_shape_and_rebuilt_when_it_changes(hip_backend):
    """X for (omega, n, steps), U for the root indices on top, IU for every call; other arguments than the prepared ones: the table-free pass"""
    from genstark_amd._abi import Backend
    from genstark_amd.field import PrimeField
    be = Backend(device=0)                      # a context of its own: no tables yet
    try:
        f = PrimeField(backend=be)
        rng = random.Random(31)
        n, steps = 1 << 12, 1 << 8
        vp, vk = f.newVectorFrom(rand_elements(rng, n)), f.newVectorFrom(rand_elements(rng, 64))
        be.traffic(True)
        for roots in ([0, 16 * 255], [0, 16 * 255], [0, 16 * 7]):        # new asserted values each time; the third: another position
            args, lc = composition_args(f, rng, vp, vk, 64, n, steps, roots, True, True)
            old, new = both_paths(be, f, args, lc, n)
            assert new == old
        assert launches(be.traffic()) == {OLD: 3, NEW: 3, 'k_mimc_table_x': 1, 'k_mimc_table_u': 2, 'k_mimc_table_iu': 3}
        # prepared for one interpolant, asked with another: not these tables
        other, lc = composition_args(f, rng, vp, vk, 64, n, steps, [0, 16 * 7], True, True)
        be.traffic(True)
        old, new = both_paths(be, f, args, lc, n)
        out = f.newVector(n)
        be.call('gs_mimc_composition_tables', *other, lc, C.c_void_p(out.ptr))
        ref = f.newVector(n)
        be.call('gs_mimc_composition', *other, lc, C.c_void_p(ref.ptr))
        assert new == old and out.toBuffer() == ref.toBuffer()
        assert launches(be.traffic()) == {OLD: 3, NEW: 1, 'k_mimc_table_iu': 1}
        be.traffic(False)
    finally:
        be.close()


def _prove(be, steps, at, seed):
    import genstark_amd as ga
    from genstark_amd.prover import Prover
    opts = {'hashAlgorithm': 'blake2s256', 'extensionFactor': 16, 'exeQueryCount': 20, 'friQueryCount': 12}
    stark = ga.instantiateMimc(steps, opts, backend=be)
    controls = ga.runMimc(stark.air.field, steps, stark.air.roundConstants, seed)
    assertions = [{'step': s, 'register': 0, 'value': controls[s]} for s in at]
    return Prover(stark.air, opts).prove_bytes(assertions, [], [seed])


def test_proofs_reuse_the_tables_and_fall_back_above_the_size_cap():
    """Three proofs in one context: the same shape with other asserted values (X and U serve both, IU is rebuilt), then other assertion
    positions (U is rebuilt).  The same three with the tables capped below the domain size: the table-free pass, the same proof bytes."""
    from genstark_amd._abi import Backend
    steps = 1 << 8
    jobs = [([0, steps - 1], 3), ([0, steps - 1], 5), ([0, 9, 10, steps - 1], 5)]
    be = Backend(device=0)
    try:
        be.traffic(True)
        with_tables = [_prove(be, steps, at, seed) for at, seed in jobs]
        assert launches(be.traffic()) == {NEW: 3, 'k_mimc_table_x': 1, 'k_mimc_table_u': 2, 'k_mimc_table_iu': 3}
        assert with_tables[0] != with_tables[1]
        previous = be.lib.gs_mimc_composition_tables_max_n(steps * 16 // 2)
        try:
            be.traffic(True)
            without = [_prove(be, steps, at, seed) for at, seed in jobs]
            assert launches(be.traffic()) == {OLD: 3}
        finally:
            be.lib.gs_mimc_composition_tables_max_n(previous)
        be.traffic(False)
        assert without == with_tables
    finally:
        be.close()
