"""Records of any length hashed with Poseidon and Rescue: include/gstark_absorb.h, csrc/hades.hip, csrc/rescue.hip, csrc/sponge_common.h,
genstark_amd/field_tree.py (absorb / absorbMany of HadesHash and RescueHash), lib128.compute_poseidon_absorb_air, js/hades.js, js/rescue.js.

Every comparison is equality of field elements.  The reference of the host members is `restated`, the definition written out below;
the reference of the device is the host member.  CPU tier: the host members, the refusals, the whole Python layer on the tests' double
(which lacks the entries: host integers), the AIR under the mirror Stark, the header, node.  GPU tier: both kernels at the seams of their
workgroups, of the rate and of the layouts, raw calls with padded strides and every refusal of the library, trees over absorbed records,
the runtime-modulus flavour (`python tests/test_absorb.py runtime <q>`), the AIR's proof bytes, node."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pytest

from genstark_amd import _abi, lib128, lib224
from genstark_amd._abi import Backend, GstarkError
from genstark_amd.errors import StarkError
from genstark_amd.field import Matrix, PrimeField
from genstark_amd.hades import HadesHash, HadesMerkleTree
from genstark_amd.rescue_hash import RescueHash, rescue4x128
from genstark_amd._mirror.stark import Stark
from sponge_common import FLAVOURS, ROOT, check_header_is_plain_c, check_symbol_table, flavour_fixture, heap_nodes, input_rows, needs_node, run_js

OPTS = {'hashAlgorithm': 'blake2s256', 'extensionFactor': 32, 'exeQueryCount': 44, 'friQueryCount': 20}       # those of tests/test_lib128.py


def restated(permute, width, p, record, rate, digest):
    """the definition, written out: the length in the first capacity element, `rate` inputs added per permutation"""
    state = [0] * width
    state[rate] = len(record)
    for b in range((len(record) + rate - 1) // rate):
        for j in range(rate):
            if b * rate + j < len(record):
                state[j] = (state[j] + record[b * rate + j]) % p
        state = permute(state)
    return state[:digest]


def default_rate(width):
    return width - 1 if width <= 3 else width - 2


def seam_lengths(rate):
    return sorted({n for n in (1, rate - 1, rate, rate + 1, 2 * rate, 2 * rate + 1, 4 * rate + 3) if n >= 1})


def random_rescue(f, rng, width, rounds=2):
    """random constants and a full-size inverse exponent, as tests/test_rescue_hash.py builds them"""
    p = f.modulus
    return RescueHash(f, 3, rng.randrange(1 << (p.bit_length() - 1), p - 1), width, rounds, [[rng.randrange(p) for _ in range(width)] for _ in range(width)],
                      [rng.randrange(p) for _ in range(width * (width + 2))])


def random_hades(f, rng, alpha, rf, rp, width):
    """random round constants and matrix: values are compared, no property of the matrix is used (and every field has them)"""
    p = f.modulus
    return HadesHash(f, alpha, rf, rp, width, [[rng.randrange(p) for _ in range(width)] for _ in range(rf + rp)],
                     [[rng.randrange(p) for _ in range(width)] for _ in range(width)])


def rescue_permutation(h, modified):
    return lambda state: (h.modifiedSponge if modified else h.sponge)(state)[1][-1]


# ---- CPU tier: header and binding table -------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    check_header_is_plain_c('absorb')


def test_symbol_table_matches_the_header():
    assert _abi.ABSORB_SYMBOLS == ('gs_hades_absorb', 'gs_rescue_absorb')
    check_symbol_table('absorb', _abi.ABSORB_SYMBOLS, (_abi.EXPORTED_SYMBOLS, _abi.OPTIONAL_SYMBOLS, _abi.HADES_SYMBOLS, _abi.RESCUE_SYMBOLS))
    table = open(os.path.join(ROOT, 'napi', 'gstark_napi.cc')).read()
    for name in _abi.ABSORB_SYMBOLS:
        assert f'{{"{name}", "' in table, name


def test_the_double_lacks_the_entries(oracle_backend):
    assert not any(hasattr(oracle_backend.lib, name) for name in _abi.ABSORB_SYMBOLS)


# ---- CPU tier: the host members -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', [2, 3, 6, 8])
def test_hades_absorb_is_the_definition(oracle_backend, width):
    f = PrimeField(backend=oracle_backend)
    p, rng = f.modulus, random.Random(0xAB50 + width)
    for rp in (0, 1):
        h = HadesHash(f, 5, 2, rp, width)
        for rate in sorted({1, default_rate(width), width - 1}):
            for length in seam_lengths(rate):
                record = input_rows(rng, p, 7, length)[6]
                for digest in (1, 2):
                    if digest > rate:
                        continue
                    assert h.absorb(record, digest, rate) == restated(h.permute, width, p, record, rate, digest), (width, rp, rate, length, digest)
                if rate == default_rate(width) and rate >= 2:                 # the defaults: two elements at that rate
                    assert h.absorb(record) == h.absorb(record, 2, rate)
    h = HadesHash(f, 5, 2, 1, 6)
    assert h.absorb([p - 1, p + 3, 2 * p]) == h.absorb([p - 1, 3, 0])          # inputs are taken mod p, the length is not part of them


@pytest.mark.parametrize('width', [2, 4])
def test_rescue_absorb_is_the_definition(oracle_backend, width):
    f = PrimeField(backend=oracle_backend)
    p, rng = f.modulus, random.Random(0xAB60 + width)
    h = random_rescue(f, rng, width)
    for modified in (True, False):
        for rate in sorted({1, default_rate(width), width - 1}):
            for length in seam_lengths(rate):
                record = input_rows(rng, p, 7, length)[6]
                for digest in (1, 2):
                    if digest > rate:
                        continue
                    want = restated(rescue_permutation(h, modified), width, p, record, rate, digest)
                    assert h.absorb(record, digest, rate, modified) == want, (width, modified, rate, length, digest)
    record = [5, 6, 7]
    assert h.absorb(record) == h.absorb(record, 1, default_rate(width), True)


def test_refusals(oracle_backend):
    f = PrimeField(backend=oracle_backend)
    rng = random.Random(3)
    for h in (HadesHash(f, 5, 2, 1, 6), random_rescue(f, rng, 4)):
        for kwargs, text in (({'rate': 0}, 'a rate of 0'), ({'rate': h.width}, f'a rate of {h.width}'), ({'rate': 1, 'digest': 2}, 'a digest of'),
                             ({'digest': 3}, 'a digest of'), ({'digest': 0}, 'a digest of')):
            with pytest.raises(GstarkError, match='absorb: ' + text):
                h.absorb([1, 2, 3], **kwargs)
            with pytest.raises(GstarkError, match='absorb: ' + text):
                h.absorbMany([[1, 2, 3]], **kwargs)
        with pytest.raises(GstarkError, match='absorb: a record of 0 elements'):
            h.absorb([])
        with pytest.raises(GstarkError, match='absorb: a record of 0 elements'):
            h.absorbMany([[], []])
        with pytest.raises(GstarkError, match='absorb: a record of 65537 elements'):
            h.absorb([1] * ((1 << 16) + 1))
        with pytest.raises(GstarkError, match='absorb: a record of 65537 elements'):
            h.absorbMany([[1] * ((1 << 16) + 1)])
        with pytest.raises(GstarkError, match='absorb: every row has the same number'):
            h.absorbMany([[1, 2, 3], [1, 2]])
        with pytest.raises(GstarkError, match='absorb: every column has the same number'):
            h.absorbMany([f.newVectorFrom([1, 2, 3]), f.newVectorFrom([1, 2])], columns=True)


def test_the_length_separates_what_padding_does_not(oracle_backend):
    f = PrimeField(backend=oracle_backend)
    rng = random.Random(4)
    h, r = HadesHash(f, 5, 8, 55, 6), random_rescue(f, rng, 4)
    for a in (0, 1, 77, f.modulus - 1):
        assert h.hash([a]) == h.hash([a, 0])                                  # the one-permutation hash pads with zeros ...
        assert h.absorb([a]) != h.absorb([a, 0])                              # ... the length in the capacity keeps them apart
        assert r.absorb([a]) != r.absorb([a, 0])
        assert r.absorb([a], modified=False) != r.absorb([a, 0], modified=False)
    for x in ([1], [1, 2], [1, 2, 3, 4]):
        assert h.absorb(x) != h.hash(x)
        assert r.absorb(x, 2) != r.modifiedSponge(x)[1][-1][:2]
    assert h.absorb([1, 2, 3, 4]) != h.absorb([1, 2, 3, 4, 0])


def test_absorb_many_on_the_double(oracle_backend):
    f = PrimeField(backend=oracle_backend)
    p, rng = f.modulus, random.Random(5)
    r4 = random_rescue(f, rng, 4)
    for h, kwargs in ((HadesHash(f, 5, 2, 1, 6), {}), (HadesHash(f, 3, 2, 0, 3), {'rate': 1, 'digest': 1}), (r4, {}), (r4, {'modified': False, 'digest': 2})):
        assert not h.onDevice
        for length in (1, 4, 5, 11):
            rows = input_rows(rng, p, 9, length)
            want = [h.absorb(r, **kwargs) for r in rows]
            columns = [list(c) for c in zip(*rows)]
            assert h.absorbMany(rows, **kwargs).toValues() == want
            assert h.absorbMany(f.newMatrixFrom(rows), **kwargs).toValues() == want
            assert h.absorbMany(columns, columns=True, **kwargs).toValues() == want
            assert h.absorbMany(f.newMatrixFrom(columns), columns=True, **kwargs).toValues() == want
            assert h.absorbMany([f.newVectorFrom(c) for c in columns], columns=True, **kwargs).toValues() == want
        for empty in (h.absorbMany([], **kwargs), h.absorbMany(Matrix(oracle_backend, 0, 5), **kwargs), h.absorbMany(Matrix(oracle_backend, 5, 0), columns=True, **kwargs)):
            assert isinstance(empty, Matrix) and (empty.rowCount, empty.colCount) == (0, kwargs.get('digest', 2 if isinstance(h, HadesHash) else 1))


def test_library_hashes_are_the_trees_hashes(oracle_backend):
    f = PrimeField(backend=oracle_backend)
    h = lib128.poseidon(f)
    assert (h.width, h.fullRounds, h.partialRounds, h.alpha) == (6, 8, 55, 5)
    assert h.hash([1, 2, 3, 4]) == lib128.poseidon_hash(f, [1, 2, 3, 4]) == lib128.poseidon_tree(f, [(0, 0), (0, 0)]).hash.hash([1, 2, 3, 4])
    assert lib128.poseidon_sparse_tree(f, 3).hash.hash([5, 6]) == h.hash([5, 6])
    from test_wide_fields import oracle_for
    be = oracle_for('p224')
    try:
        f = PrimeField(backend=be)
        h = lib224.poseidon(f)
        assert h.width == 3 and h.hash([42, 43]) == lib224.poseidon_hash(f, [42, 43]) == lib224.poseidon_tree(f, [0, 0]).hash.hash([42, 43])
        assert lib224.poseidon_sparse_tree(f, 3).hash.hash([5]) == h.hash([5])
    finally:
        be.close()


# ---- CPU tier: the AIR --------------------------------------------------------------------------------------------------------------
def absorb_statement(backend, length):
    f = PrimeField(backend=backend)
    record = input_rows(random.Random(0xA1B + length), f.modulus, 7, length)[6]
    inputs, first, assertions = lib128.poseidon_absorb_inputs(f, record)
    blocks = (length + 3) // 4
    air = lib128.compute_poseidon_absorb_air(f, blocks)
    return f, record, air, inputs, first, assertions


def check_absorb_air(backend, length, native=False):
    f, record, air, inputs, first, assertions = absorb_statement(backend, length)
    digest = lib128.poseidon(f).absorb(record)
    assert first == (record + [0, 0, 0])[:4] + [length, 0]
    assert [(a['step'], a['register'], a['value']) for a in assertions] == [(0, 4, length), (0, 5, 0), (air.steps - 1, 0, digest[0]), (air.steps - 1, 1, digest[1])]
    trace = air.hostTrace(first, inputs=inputs)
    assert len(trace) == 64 * ((length + 3) // 4) and trace[-1][:2] == digest
    stark = Stark(air, OPTS)
    proof = stark.prove(assertions, inputs, first)
    data = stark.serialize(proof)
    assert len(data) == stark.sizeOf(proof) and stark.verify(assertions, stark.parse(data))
    if native:
        from conftest import native_same_bytes
        native_same_bytes(stark, assertions, inputs, first, data)
    return stark, assertions, data


@pytest.mark.parametrize('length', [1, 4, 5, 8, 13])
def test_absorb_air_oracle(oracle_backend, length):
    stark, assertions, data = check_absorb_air(oracle_backend, length)
    other = length - 1 if length % 4 != 1 else length + 1                    # another length of the same number of blocks
    with pytest.raises(StarkError):
        stark.verify([dict(assertions[0], value=other)] + assertions[1:], stark.parse(data))
    with pytest.raises(StarkError):
        stark.verify(assertions[:2] + [dict(assertions[2], value=assertions[2]['value'] ^ 1)] + assertions[3:], stark.parse(data))


def test_absorb_air_refuses_three_blocks(oracle_backend):
    f = PrimeField(backend=oracle_backend)
    with pytest.raises(ValueError, match=r'a record of 9 elements is 3 blocks: the number of blocks, ceil\(L / 4\), is a power of two'):
        lib128.poseidon_absorb_inputs(f, list(range(9)))
    with pytest.raises(ValueError, match=r'3 blocks: the number of blocks, ceil\(L / 4\), is a power of two'):
        lib128.compute_poseidon_absorb_air(f, 3)


# ---- GPU tier: the kernels ----------------------------------------------------------------------------------------------------------
HADES_COUNTS = (1, 63, 64, 65, 255, 256, 257)         # the seams of a wave (64 lanes) and of a workgroup (256 threads)
RESCUE_COUNTS = (1, 7, 8, 9, 15, 16, 17, 65)          # the seams of 64 / G rows per workgroup (G = 8, 4: 8 and 16 rows), several workgroups

flavour = flavour_fixture()


def check_layouts(h, rows, want, counts, digests, **kwargs):
    """absorbMany over the first `count` of `rows` for every count, by rows (a view of one upload) and by columns, against want[k][:digest]"""
    f, length = h.field, len(rows[0])
    whole = f.newMatrixFrom(rows)
    for count in counts:
        by_rows = Matrix(f.backend, count, length, owner=whole._owner, offset=whole._offset)
        by_columns = f.newMatrixFrom([list(c) for c in zip(*rows[:count])])
        for digest in digests:
            expect = [w[:digest] for w in want[:count]]
            assert h.absorbMany(by_rows, digest=digest, **kwargs).toValues() == expect, (h.width, length, count, digest, kwargs, 'rows')
            assert h.absorbMany(by_columns, digest=digest, columns=True, **kwargs).toValues() == expect, (h.width, length, count, digest, kwargs, 'columns')


def check_hades(be, rng, widths=(2, 3, 6, 8), counts=HADES_COUNTS, real=(65, 257)):
    f = PrimeField(backend=be)
    p = f.modulus
    for width in widths:
        h = random_hades(f, rng, 3, 2, width % 2, width)                    # cheap rounds keep the host reference short
        assert h.onDevice
        for rate in sorted({1, default_rate(width), width - 1}):
            digests = (1, 2) if rate >= 2 else (1,)
            for length in seam_lengths(rate):
                # every count at the default rate; the other rates at the count that crosses a wave
                use = counts if rate == default_rate(width) else tuple(c for c in counts if c == 65) or counts[-1:]
                rows = input_rows(rng, p, max(use), length)
                want = [h.absorb(r, 2 if rate >= 2 else 1, rate) for r in rows]      # once, shared by every count, digest and layout
                check_layouts(h, rows, want, use, digests, rate=rate)
    if real:
        h = random_hades(f, rng, 5, 8, 55, 6)                                      # lib128's shape: 8 + 55 rounds, x^5, rate 4
        rows = input_rows(rng, p, max(real), 9)                              # three blocks, the last one short
        want = [h.absorb(r) for r in rows]
        check_layouts(h, rows, want, real, (1, 2))


def check_rescue(be, rng, widths=(2, 4, 8), counts=RESCUE_COUNTS):
    f = PrimeField(backend=be)
    p = f.modulus
    for width in widths:
        h = random_rescue(f, rng, width)
        assert h.onDevice
        for modified in (True, False):
            for rate in sorted({1, default_rate(width), width - 1}):
                digests = (1, 2) if rate >= 2 else (1,)
                for length in seam_lengths(rate):
                    use = counts if rate == default_rate(width) else (17,)
                    rows = input_rows(rng, p, max(use), length)
                    want = [h.absorb(r, 2 if rate >= 2 else 1, rate, modified) for r in rows]
                    check_layouts(h, rows, want, use, digests, rate=rate, modified=modified)


@pytest.mark.gpu
@pytest.mark.parametrize('width', [2, 3, 6, 8])
def test_hades_records_at_the_seams(flavour, width):
    check_hades(flavour, random.Random(0xAB50 + width), widths=(width,), real=(65, 257) if width == 6 else ())


@pytest.mark.gpu
@pytest.mark.parametrize('width', [2, 4, 8])
def test_rescue_records_at_the_seams(flavour, width):
    check_rescue(flavour, random.Random(0xAB60 + width), widths=(width,))


@pytest.mark.gpu
def test_example_parameter_sets(hip_backend):
    """the sets tools/absorb_bench.py measures: lib128's Poseidon and rescue4x128 at their default rates, against the host members"""
    f = PrimeField(backend=hip_backend)
    rng = random.Random(0xAB7)
    rows = input_rows(rng, f.modulus, 33, 13)
    h = lib128.poseidon(f)
    check_layouts(h, rows, [h.absorb(r) for r in rows], (33,), (1, 2))
    r = rescue4x128(f)
    rows = rows[:9]
    check_layouts(r, rows, [r.absorb(x, 2) for x in rows], (9,), (1, 2))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['p128', 'p224'])
def test_raw_calls_read_sub_matrices(name):
    """row_stride = L + 3 and elem_stride = count + 5: the leading part of a wider matrix, in both families"""
    be = Backend(device=0, modulus=FLAVOURS[name])
    try:
        f = PrimeField(backend=be)
        p, rng = f.modulus, random.Random(0xAB8)
        count, length = 70, 11
        hades, rescue = HadesHash(f, 3, 2, 1, 6), random_rescue(f, rng, 4)
        wide = input_rows(rng, p, count, length + 3)                         # rows layout: three more columns than are read
        tall = [[rng.randrange(p) for _ in range(count + 5)] for _ in range(length)]      # columns layout: five more records than are read
        for src, strides, records in ((f.newMatrixFrom(wide), (length + 3, 1), [r[:length] for r in wide]),
                                      (f.newMatrixFrom(tall), (1, count + 5), [[tall[i][k] for i in range(length)] for k in range(count)])):
            for h, entry, options in ((hades, 'gs_hades_absorb', ()), (rescue, 'gs_rescue_absorb', (1,)), (rescue, 'gs_rescue_absorb', (0,))):
                out = Matrix(be, count, 2)
                be.call(entry, h.handle(), C.c_void_p(src.ptr), count, length, *strides, default_rate(h.width), 2, *options, C.c_void_p(out.ptr))
                want = [h.absorb(r, 2) if h is hades else h.absorb(r, 2, None, bool(options[0])) for r in records]
                assert out.toValues() == want, (entry, strides, options)
    finally:
        be.close()


@pytest.mark.gpu
def test_refusals_of_the_library(hip_backend):
    """every refusal has its code (GS_ERR_ARG = -1) and an `absorb`-prefixed message of its own, and leaves `out` as it was"""
    f = PrimeField(backend=hip_backend)
    other = Backend(device=0)
    try:
        rng = random.Random(0xAB9)
        hades, rescue = HadesHash(f, 3, 2, 1, 6), random_rescue(f, rng, 4)
        foreign_hades, foreign_rescue = HadesHash(PrimeField(backend=other), 3, 2, 1, 6), random_rescue(PrimeField(backend=other), rng, 4)
        count, length = 8, 5
        src = f.newMatrixFrom(input_rows(rng, f.modulus, count, length))
        filled = [[rng.randrange(f.modulus), rng.randrange(f.modulus)] for _ in range(count)]
        out = f.newMatrixFrom(filled)
        good = dict(h=None, src=src.ptr, count=count, length=length, row_stride=length, elem_stride=1, rate=None, digest=2, out=out.ptr)
        cases = [(dict(h='foreign'), 'absorb: the handle belongs to another context'),
                 (dict(rate=0), 'absorb: a rate of 0 does not leave a capacity'),
                 (dict(rate='width'), 'absorb: a rate of . does not leave a capacity'),
                 (dict(digest=0), 'absorb: a digest of 1 or 2 elements and at most the rate'),
                 (dict(digest=3), 'absorb: a digest of 1 or 2 elements and at most the rate'),
                 (dict(rate=1, digest=2), 'absorb: a digest of 1 or 2 elements and at most the rate'),
                 (dict(length=0), 'absorb: a row of 0 elements'),
                 (dict(length=(1 << 16) + 1, row_stride=(1 << 16) + 1), 'absorb: a row of 65537 elements'),
                 (dict(row_stride=length - 1), 'absorb: strides .* are neither rows'),
                 (dict(row_stride=1, elem_stride=count - 1), 'absorb: strides .* are neither rows'),
                 (dict(row_stride=length, elem_stride=2), 'absorb: strides .* are neither rows'),
                 (dict(row_stride=2, elem_stride=count), 'absorb: strides .* are neither rows'),
                 (dict(count=(1 << 36) // 2 + 1), 'absorb: at most 2\\^36 permutations per call'),
                 (dict(src=None), 'absorb: in and out are required'),
                 (dict(out=None), 'absorb: in and out are required'),
                 (dict(out=src.ptr + 16), 'absorb: out overlaps in')]
        for h, foreign, entry, options in ((hades, foreign_hades, 'gs_hades_absorb', ()), (rescue, foreign_rescue, 'gs_rescue_absorb', (1,))):
            for change, text in cases:
                a = dict(good, **change)
                handle = (foreign if a['h'] == 'foreign' else h).handle()
                rate = h.width if a['rate'] == 'width' else default_rate(h.width) if a['rate'] is None else a['rate']
                args = (handle, C.c_void_p(a['src']), a['count'], a['length'], a['row_stride'], a['elem_stride'], rate, a['digest'], *options, C.c_void_p(a['out']))
                assert getattr(hip_backend.lib, entry)(hip_backend.ctx, *args) == -1, (entry, change)
                with pytest.raises(GstarkError, match=entry[3:] + text[6:]):
                    hip_backend.call(entry, *args)
                assert out.toValues() == filled, (entry, change)
            hip_backend.call(entry, h.handle(), None, 0, length, length, 1, default_rate(h.width), 2, *options, None)      # count 0: GS_OK, nothing touched
        with pytest.raises(GstarkError, match='rescue_absorb: modified is 0'):
            hip_backend.call('gs_rescue_absorb', rescue.handle(), C.c_void_p(src.ptr), count, length, length, 1, 2, 2, 2, C.c_void_p(out.ptr))
        assert out.toValues() == filled
        assert hades.absorbMany([]).rowCount == 0
    finally:
        other.close()


@pytest.mark.gpu
def test_trees_over_absorbed_records(hip_backend):
    f = PrimeField(backend=hip_backend)
    rng = random.Random(0xABA)
    h = HadesHash(f, 3, 2, 1, 6)
    records = input_rows(rng, f.modulus, 64, 7)
    leaves = [h.absorb(r) for r in records]
    node = lambda left, right: h.hash(left + right)[:2]
    tree = HadesMerkleTree(h, h.absorbMany(records, 2), 2)
    assert tree.deviceNodes.toValues() == heap_nodes(leaves, node, [0, 0])
    indexes, fresh = [5, 63, 0, 5], input_rows(rng, f.modulus, 4, 7)
    updates = tree.updateMany(indexes, h.absorbMany(fresh, 2))
    for i, r in zip(indexes, fresh):
        leaves[i] = h.absorb(r)
    want = heap_nodes(leaves, node, [0, 0])
    assert tree.deviceNodes.toValues() == want and updates[-1].root == tuple(want[1])
    assert HadesMerkleTree(h, h.absorbMany(f.newMatrixFrom([list(c) for c in zip(*records)]), 2, columns=True), 2).root != tree.root


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['q32', 'q17', 'p256'])
def test_other_built_fields(name):
    """the flavours flavour_fixture has no name for: one case per family"""
    be = Backend(device=0, modulus={'q32': _abi.MODULUS_32, 'q17': _abi.MODULUS_17, 'p256': _abi.MODULUS_256}[name])
    try:
        rng = random.Random(0xABB)
        check_hades(be, rng, widths=(6,), counts=(65,), real=())
        check_rescue(be, rng, widths=(4,), counts=(17,))
        f = PrimeField(backend=be)
        h = random_hades(f, rng, 3, 2, 1, 3)
        record = [f.modulus - 1] * 1000                                      # a long record: 500 blocks
        assert h.absorbMany([record] * 3).toValues() == [h.absorb(record)] * 3
    finally:
        be.close()


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    from test_runtime_modulus import PRIMES
    q = PRIMES[12]                                    # 127 bits
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(q)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'runtime absorb: modulus {q} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
def test_absorb_air_hip_equals_oracle(hip_backend, oracle_backend):
    assert check_absorb_air(hip_backend, 13, native=True)[2] == check_absorb_air(oracle_backend, 13)[2]      # 256 steps
    assert check_absorb_air(hip_backend, 4)[2] == check_absorb_air(oracle_backend, 4)[2]


# ---- node ---------------------------------------------------------------------------------------------------------------------------
def js_expectations(path):
    """what tests/js_absorb.js must find, from host integers: per field a width-6 Poseidon (x^5, 8 + 55 rounds) and a width-4 Rescue of random
    constants (3 rounds) over records of 1, 4, 5 and 11 elements"""
    from genstark_amd.hostfield import HostField
    rng = random.Random(0x35)
    s = lambda v: [s(x) for x in v] if isinstance(v, list) else str(v)
    out = []
    for modulus in (_abi.MODULUS_128, _abi.MODULUS_64):
        f = HostField(modulus)
        h, r = HadesHash(f, 5, 8, 55, 6), random_rescue(f, rng, 4, 3)
        cases = []
        for length in (1, 4, 5, 11):
            rows = [[0, 1, modulus - 1, 5, 6, 7, 8, 9, 10, 11, 12][:length]] + [[rng.randrange(modulus) for _ in range(length)] for _ in range(9)]
            cases.append({'rows': s(rows), 'hades': s([h.absorb(x) for x in rows]), 'hadesRate1': s([h.absorb(x, 1, 1) for x in rows]),
                          'rescue': s([r.absorb(x) for x in rows]), 'rescueSponge': s([r.absorb(x, 2, 3, False) for x in rows])})
        out.append({'modulus': str(modulus), 'invAlpha': str(r.invAlpha), 'mds': s(r.mds),
                    'constants': s(r.iConstants + [v for row in r.cMatrix for v in row] + r.cConstants), 'cases': cases})
    with open(path, 'w') as fh:
        json.dump(out, fh)


@needs_node
def test_js_on_a_library_without_the_entries(tmp_path):
    """the host members equal the Python host; the device members throw an Error that names the entry"""
    run_js('absorb', 'double', tmp_path, js_expectations)


@needs_node
@pytest.mark.gpu
def test_js_on_hip(tmp_path):
    run_js('absorb', 'hip', tmp_path, js_expectations)


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    rng = random.Random(q % 65521)
    check_hades(be, rng, widths=(3, 6), counts=(65, 257), real=())
    check_rescue(be, rng, widths=(2, 4), counts=(9, 17))
    print(f'runtime absorb: modulus {q} ok')
