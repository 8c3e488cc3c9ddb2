"""Batched updates of the device Merkle trees with every update's witness: include/gstark_tree_update.h, csrc/tree_update_plan.h,
csrc/field_tree.hip, FieldMerkleTree.update / updateMany (genstark_amd/field_tree.py), DeviceTree.update / updateMany (js/field_tree.js).

Every comparison is equality with host integers.  CPU tier: the header and the binding table, the host plan on its own under the
sanitizers (tests/host_harness/tree_update_plan_host.cpp), and updateMany on libraries without the entries (the host path) against the
naive model: the control tree rebuilt after every update.  GPU tier: the two kernels and the shared driver under both families at the
seams of a wave and of a workgroup, in three field flavours and the runtime-modulus one, the update statements of lib128 / lib224 proved
from the records, the library's refusals and the node binding.  `python tests/test_tree_update.py runtime <q>` is the check of the
runtime-modulus flavour (one modulus per process)."""
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
from genstark_amd.field import PrimeField
from genstark_amd.field_tree import TreeUpdate
from genstark_amd.hades import HadesHash, HadesMerkleTree
from genstark_amd.hostfield import HostField
from genstark_amd.rescue_hash import RescueHash, RescueMerkleTree, rescue2x64, rescue4x128
from sponge_common import FLAVOURS, ROOT, check_header_is_plain_c, check_symbol_table, flavour_fixture, heap_nodes, needs_node, run_js


# ---- CPU tier: header and binding table -------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    check_header_is_plain_c('tree_update')


def test_symbol_table_matches_the_header():
    assert _abi.TREE_UPDATE_SYMBOLS == ('gs_hades_merkle_update', 'gs_rescue_merkle_update')
    check_symbol_table('tree_update', _abi.TREE_UPDATE_SYMBOLS, (_abi.EXPORTED_SYMBOLS, _abi.OPTIONAL_SYMBOLS, _abi.HADES_SYMBOLS, _abi.RESCUE_SYMBOLS))
    assert '2^20' in open(os.path.join(ROOT, 'include', 'gstark_tree_update.h')).read()       # the cap on a batch is part of the contract


def test_the_double_lacks_the_entries(oracle_backend):
    assert not any(hasattr(oracle_backend.lib, name) for name in _abi.TREE_UPDATE_SYMBOLS)


# ---- CPU tier: the host plan on its own ---------------------------------------------------------------------------------------------
def test_plan_against_brute_force_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'tree_update_plan_host')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-omit-frame-pointer', os.path.join(ROOT, 'tests', 'host_harness', 'tree_update_plan_host.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'batches ok' in r.stdout and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


# ---- the models -----------------------------------------------------------------------------------------------------------------------
def naive_model(build, leaves, indexes, new):
    """the control tree rebuilt after every update: (before per update, root per update, final nodes) in the control's shapes"""
    leaves = list(leaves)
    tree = build(leaves)
    before, roots = [], []
    for i, v in zip(indexes, new):
        before.append(tree.prove(i))
        leaves[i] = v
        tree = build(leaves)
        roots.append(tree.root)
    return before, roots, tree.nodes


def stepwise_model(node, leaves, indexes, new, snapshots=()):
    """one update at a time on rows of host integers, only the path recomputed: (before, roots, {count: the 2n node rows after `count`
    updates}); before[j] and roots[j] do not depend on what follows, so one run serves every prefix of the batch"""
    n, zero = len(leaves), [0] * len(leaves[0])
    nodes = heap_nodes([list(v) for v in leaves], node, zero)
    depth = n.bit_length() - 1
    before, roots, snaps = [], [], {}
    for j, (i, v) in enumerate(zip(indexes, new)):
        at = n + i
        before.append([nodes[at]] + [nodes[(at >> l) ^ 1] for l in range(depth)])
        nodes[at] = list(v)
        while at > 1:
            at >>= 1
            nodes[at] = node(nodes[2 * at], nodes[2 * at + 1])
        roots.append(nodes[1])
        if j + 1 in snapshots:
            snaps[j + 1] = list(nodes)
    return before, roots, snaps


def index_patterns(n, k, rng):
    """the patterns of the plan harness, k updates each: all indexes equal, two sibling leaves alternating, every leaf in turn, the two
    halves of the tree interleaved, and random ones (the whole tree, and a window of 4 leaves: heavy collisions)"""
    pair = (rng.randrange(n) & ~1)
    return {'equal': [n - 1] * k, 'siblings': [pair + (j & 1) for j in range(k)], 'every leaf': [j % n for j in range(k)],
            'halves': [(j // 2 + (n // 2) * (j & 1)) % n for j in range(k)], 'random': [rng.randrange(n) for _ in range(k)],
            'window': [(n - min(n, 4)) + rng.randrange(min(n, 4)) for _ in range(k)]}


def shaped(tree, rows):
    return [tree._shape(r) for r in rows]


# ---- CPU tier: updateMany on libraries without the entries ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def p224_double():
    from test_wide_fields import oracle_for
    be = oracle_for('p224')
    yield be
    be.close()


def small_batch(n, rng, p, leaves, random_leaf):
    """a repeated index, a sibling pair back to back, an update that changes nothing, and a random one"""
    i = rng.randrange(n)
    indexes = [i, i ^ 1, i, rng.randrange(n), i ^ 1]
    new = [random_leaf() for _ in indexes]
    new[4] = new[1]                                   # leaf i ^ 1 already holds it
    return indexes, new


def check_against_the_naive_model(tree, build, verify, leaves, indexes, new):
    want_before, want_roots, want_nodes = naive_model(build, leaves, indexes, new)
    root = tree.root
    records = tree.updateMany(indexes, new)
    assert [r.before for r in records] == want_before
    assert [r.root for r in records] == want_roots
    assert tree.nodes == want_nodes and tree.root == want_roots[-1]
    for i, record in zip(indexes, records):
        assert isinstance(record, TreeUpdate) and verify(root, i, record.before)
        root = record.root
    assert tree.proveMany(indexes) == [tree.prove(i) for i in indexes]
    path, root = tree.prove(indexes[0]), tree.root
    assert tree.update(indexes[0], path[0]) == TreeUpdate(path, root) and tree.nodes == want_nodes      # the leaf it holds: nothing changes


@pytest.mark.parametrize('n', [2, 4, 64])
def test_host_updates_equal_the_naive_model(oracle_backend, p224_double, n):
    rng = random.Random(0x0DD + n)
    f = PrimeField(backend=oracle_backend)
    p = f.modulus
    pair = lambda: (rng.randrange(p), rng.randrange(p))
    leaves = [pair() for _ in range(n)]
    tree = lib128.poseidon_tree(f, leaves)
    assert tree.deviceNodes is None
    check_against_the_naive_model(tree, lambda v: lib128.PoseidonMerkleTree(f, v), lambda root, i, path: HadesMerkleTree.verify(root, i, path, tree.hash), leaves,
                                  *small_batch(n, rng, p, leaves, pair))
    # the double with a hash of its own, nodes of one element, and a field without a backend: the same model
    for field in (f, HostField(p)):
        h = HadesHash(field, 3, 2, 1, 3)
        leaves = [rng.randrange(p) for _ in range(n)]

        class Control:
            def __init__(self, values):
                rows = heap_nodes([[v] for v in values], lambda a, b: h.hash(a + b)[:1], None)
                self.nodes = [None] + [r[0] for r in rows[1:]]
                self.root = self.nodes[1]

            def prove(self, i):
                return [self.nodes[n + i]] + [self.nodes[((n + i) >> l) ^ 1] for l in range(n.bit_length() - 1)]
        check_against_the_naive_model(HadesMerkleTree(h, leaves, 1), Control, lambda root, i, path: HadesMerkleTree.verify(root, i, path, h), leaves,
                                      *small_batch(n, rng, p, leaves, lambda: rng.randrange(p)))
    f224 = PrimeField(backend=p224_double)
    q = f224.modulus
    leaves = [rng.randrange(q) for _ in range(n)]
    tree224 = lib224.poseidon_tree(f224, leaves)
    check_against_the_naive_model(tree224, lambda v: lib224.PoseidonMerkleTree(f224, v), lambda root, i, path: HadesMerkleTree.verify(root, i, path, tree224.hash),
                                  leaves, *small_batch(n, rng, q, leaves, lambda: rng.randrange(q)))


@pytest.mark.parametrize('n', [2, 4, 64])
def test_host_updates_of_the_rescue_tree_equal_the_naive_model(oracle_backend, n):
    rng = random.Random(0x0EE + n)
    f = PrimeField(backend=oracle_backend)
    p = f.modulus
    h = rescue4x128(f)

    class Control:
        def __init__(self, values):
            self.nodes = heap_nodes(list(values), h.hash2, None)
            self.root = self.nodes[1]

        def prove(self, i):
            return [self.nodes[n + i]] + [self.nodes[((n + i) >> l) ^ 1] for l in range(n.bit_length() - 1)]
    leaves = [rng.randrange(p) for _ in range(n)]
    tree = RescueMerkleTree(h, leaves)
    assert tree.deviceNodes is None
    check_against_the_naive_model(tree, Control, lambda root, i, path: RescueMerkleTree.verify(root, i, path, h.hash2), leaves,
                                  *small_batch(n, rng, p, leaves, lambda: rng.randrange(p)))


def test_the_stepwise_model_equals_the_naive_one():
    """the model of the GPU tier against the control rebuilt after every update, once, on host integers"""
    f = HostField(_abi.MODULUS_64)
    rng = random.Random(5)
    h = HadesHash(f, 3, 2, 1, 3)
    node = lambda a, b: h.hash(a + b)[:1]
    leaves = [[rng.randrange(f.modulus)] for _ in range(8)]
    indexes = index_patterns(8, 12, rng)['window'] + index_patterns(8, 12, rng)['random']
    new = [[rng.randrange(f.modulus)] for _ in indexes]

    class Control:
        def __init__(self, values):
            self.nodes = heap_nodes(values, node, None)
            self.root = self.nodes[1]

        def prove(self, i):
            return [self.nodes[8 + i]] + [self.nodes[((8 + i) >> l) ^ 1] for l in range(3)]
    before, roots, nodes = naive_model(Control, leaves, indexes, new)
    got = stepwise_model(node, leaves, indexes, new, snapshots=(len(indexes),))
    assert got[0] == before and got[1] == roots and got[2][len(indexes)][1:] == nodes[1:]


def test_refusals(oracle_backend):
    f = PrimeField(backend=oracle_backend)
    h3, h6 = HadesHash(f, 3, 2, 1, 3), HadesHash(f, 3, 2, 1, 6)
    single, pairs = HadesMerkleTree(h3, [1, 2, 3, 4], 1), HadesMerkleTree(h6, [(1, 2)] * 4, 2)
    rescue = RescueMerkleTree(RescueHash(f, 3, -3, 3, 2, [[1, 2, 3], [4, 5, 7], [9, 8, 11]], list(range(1, 16))), [1, 2, 3, 4])
    for tree, leaf in ((single, 7), (pairs, (7, 8)), (rescue, 7)):
        nodes = tree.nodes
        for bad in (4, -1, 1 << 40):
            with pytest.raises(GstarkError, match=f'^{tree._who}: an index is outside of the 4 leaves'):
                tree.updateMany([0, bad], [leaf, leaf])
            with pytest.raises(GstarkError, match='outside'):
                tree.update(bad, leaf)
        for indexes, leaves in (([0, 1], [leaf]), ([0], [leaf, leaf]), ([], [leaf]), ([0], [])):
            with pytest.raises(GstarkError, match=f'^{tree._who}: {len(indexes)} indexes and {len(leaves)} leaves'):
                tree.updateMany(indexes, leaves)
        assert tree.updateMany([], []) == []
        assert tree.nodes == nodes                    # a refused batch and an empty one change nothing
    for tree, bad in ((single, (7, 8)), (pairs, 7), (pairs, (7,)), (pairs, (7, 8, 9)), (rescue, (7, 8))):
        with pytest.raises(GstarkError, match=f'^{tree._who}: every leaf has {tree.digest} elements'):
            tree.updateMany([0], [bad])
    with pytest.raises(GstarkError, match='Vector holds leaves of one element'):
        pairs.updateMany([0], f.newVectorFrom([7]))
    with pytest.raises(GstarkError, match='the leaf matrix has 1 columns'):
        pairs.updateMany([0], f.newMatrixFrom([[7]]))
    assert single.updateMany([2], f.newVectorFrom([7]))[0].before[0] == 3 and single.prove(2)[0] == 7      # leaves on a "device" are read


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 257, 1000)                   # the seams of a wave (64 lanes) and of a workgroup (256 threads)
SIZES = (2, 4, 1 << 11)

flavour = flavour_fixture()


def check_family(f, make_tree, node, digest, rng, sizes=SIZES, counts=COUNTS):
    """make_tree(leaves) builds the device tree from rows of `digest` integers; node(left, right) is its node on host rows.  Per size
    and pattern ONE model run of max(counts) updates; every count is a prefix of it on a fresh tree."""
    p = f.modulus
    row = lambda: [rng.randrange(p) for _ in range(digest)]
    for n in sizes:
        leaves = [row() for _ in range(n)]
        fresh = make_tree(leaves).deviceNodes.toBuffer()
        for name, indexes in index_patterns(n, max(counts), rng).items():
            new = [row() for _ in indexes]
            for j in range(5, len(new), 11):          # some updates change nothing: the leaf as it was at the call
                new[j] = leaves[indexes[j]]
            before, roots, snaps = stepwise_model(node, leaves, indexes, new, snapshots=counts)
            for k in counts:
                tree = make_tree(leaves)
                records = tree.updateMany(indexes[:k], new[:k] if digest > 1 else [v[0] for v in new[:k]])
                where = (digest, n, name, k)
                assert [r.before for r in records] == [shaped(tree, b) for b in before[:k]], where
                assert [r.root for r in records] == shaped(tree, roots[:k]), where
                assert _rows(tree.deviceNodes)[1:] == snaps[k][1:], where
                assert tree.root == tree._shape(roots[k - 1]) and tree.nodes[1:] == shaped(tree, snaps[k][1:]), where
            # two calls back to back equal one run of the concatenation; proveMany sees the last tree
            k = counts[-2] if len(counts) > 1 else counts[0]
            cut = k // 3
            tree = make_tree(leaves)
            flat = new if digest > 1 else [v[0] for v in new]
            records = (tree.updateMany(indexes[:cut], flat[:cut]) if cut else []) + tree.updateMany(indexes[cut:k], flat[cut:k])
            assert [r.before for r in records] == [shaped(tree, b) for b in before[:k]] and [r.root for r in records] == shaped(tree, roots[:k]), (digest, n, name)
            assert _rows(tree.deviceNodes)[1:] == snaps[k][1:], (digest, n, name)
            probe = [0, n - 1] + indexes[:20]
            assert tree.proveMany(probe) == [shaped(tree, [snaps[k][n + i]] + [snaps[k][((n + i) >> l) ^ 1] for l in range(n.bit_length() - 1)]) for i in probe]
        # a batch that sets every leaf: the node array of a fresh tree over the new leaves, bit for bit
        order = list(range(n))
        rng.shuffle(order)
        new = [row() for _ in range(n)]
        tree = make_tree(leaves)
        assert tree.deviceNodes.toBuffer() == fresh
        tree.updateMany(order, [new[i] if digest > 1 else new[i][0] for i in order])
        assert tree.deviceNodes.toBuffer() == make_tree(new).deviceNodes.toBuffer(), (digest, n)


def _rows(array):
    from genstark_amd.field import Matrix
    return array.toValues() if isinstance(array, Matrix) else [[v] for v in array.toValues()]


def check_hades(be, rng, sizes=SIZES, counts=COUNTS):
    f = PrimeField(backend=be)
    for digest, width in ((1, 3), (2, 6)):
        h = HadesHash(f, 3, 2, 1, width)              # few rounds: the host model of a thousand updates of 2^11 leaves stays short
        assert hasattr(be.lib, 'gs_hades_merkle_update')
        check_family(f, lambda leaves: HadesMerkleTree(h, f.newMatrixFrom(leaves), digest), lambda a, b: h.hash(a + b)[:digest], digest, rng, sizes, counts)


def random_rescue(f, rng, width, rounds):
    p = f.modulus
    return RescueHash(f, 3, -3, width, rounds, [[rng.randrange(p) for _ in range(width)] for _ in range(width)], [rng.randrange(p) for _ in range(width * (width + 2))])


@pytest.mark.gpu
def test_hades_updates_at_the_seams(flavour):
    check_hades(flavour, random.Random(0x0DA7E))


@pytest.mark.gpu
def test_hades_updates_of_the_reference_shape(hip_backend):
    f = PrimeField(backend=hip_backend)
    h = HadesHash(f, 5, 8, 55, 6)
    check_family(f, lambda leaves: HadesMerkleTree(h, f.newMatrixFrom(leaves), 2), lambda a, b: h.hash(a + b)[:2], 2, random.Random(0x5855), sizes=(64,), counts=(65,))


@pytest.mark.gpu
def test_rescue_updates(hip_backend):
    f = PrimeField(backend=hip_backend)
    rng = random.Random(0x4E5C)
    h, n = rescue4x128(f), 64
    p = f.modulus
    leaves = [[rng.randrange(p)] for _ in range(n)]
    # the example's 32 rounds cost the host milliseconds per node, so the model remembers the nodes it has computed, and most of the
    # batch moves four neighbouring leaves between two values each: few distinct nodes for the host, 300 x 6 permutations for the device
    seen = {}

    def node(a, b):
        key = (a[0], b[0])
        if key not in seen:
            seen[key] = [h.hash2(*key)]
        return seen[key]
    base = 4 * rng.randrange(n // 4)
    pool = [[rng.randrange(p), rng.randrange(p)] for _ in range(4)]
    indexes = [rng.randrange(n) for _ in range(20)] + [base + rng.randrange(4) for _ in range(280)]
    new = [[rng.randrange(p)] for _ in range(20)] + [[rng.choice(pool[i - base])] for i in indexes[20:]]
    counts = (1, 65, 300)
    before, roots, snaps = stepwise_model(node, leaves, indexes, new, snapshots=counts)       # one run: every count is a prefix
    for k in counts:
        tree = RescueMerkleTree(h, f.newVectorFrom([v[0] for v in leaves]))
        records = tree.updateMany(indexes[:k], [v[0] for v in new[:k]])
        assert [r.before for r in records] == [[v[0] for v in b] for b in before[:k]], k
        assert [r.root for r in records] == [v[0] for v in roots[:k]], k
        assert tree.deviceNodes.toValues()[1:] == [v[0] for v in snaps[k][1:]], k
        assert RescueMerkleTree.verify(tree.root, indexes[0], tree.prove(indexes[0]), h.hash2)


@pytest.mark.gpu
def test_rescue_updates_in_another_flavour_and_the_width_that_holds_no_tree():
    be = Backend(device=0, modulus=_abi.MODULUS_64)
    try:
        f = PrimeField(backend=be)
        rng = random.Random(0x264)
        h = random_rescue(f, rng, 3, 2)
        check_family(f, lambda leaves: RescueMerkleTree(h, f.newVectorFrom([v[0] for v in leaves])), lambda a, b: [h.hash2(a[0], b[0])], 1, rng, sizes=(2, 64), counts=(1, 65, 300))
        h2 = rescue2x64(f)
        with pytest.raises(GstarkError, match='RescueMerkleTree: two nodes do not fit'):
            RescueMerkleTree(h2, [1, 2, 3, 4])
        buf = f.newVector(64)
        ptr = C.c_void_p(buf.ptr)
        with pytest.raises(GstarkError, match='rescue_merkle_update: two nodes do not fit'):
            be.call('gs_rescue_merkle_update', h2.handle(), ptr, 4, (C.c_uint64 * 1)(0), ptr, 1, ptr, ptr)
    finally:
        be.close()


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    from test_runtime_modulus import PRIMES
    q = PRIMES[12]                                    # 127 bits
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(q)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'runtime tree update: modulus {q} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


def update_statement(lib, f, record, new_leaf, index, depth, old_root):
    """ComputeMerkleUpdate of `lib` for one record of updateMany: (stark, assertions "old root, new root", inputs, first row)"""
    from genstark_amd._mirror.stark import Stark
    from test_lib128 import OPTS
    bits = [(index >> j) & 1 for j in range(depth)]                      # least significant bit first ...
    bits = [0] + bits[:-1]                                               # ... shifted as tests/test_lib128.py shifts them
    air = lib.compute_merkle_update_air(f, depth)
    inputs, first = lib.merkle_update_inputs(f, record.before[0], new_leaf, record.before[1:], bits)
    last = 64 * depth - 1
    at = lambda register, value: {'step': last, 'register': register, 'value': value}
    if lib is lib128:
        assertions = [at(0, old_root[0]), at(1, old_root[1]), at(12, record.root[0]), at(13, record.root[1])]
    else:
        assertions = [at(0, old_root), at(6, record.root)]
    return Stark(air, OPTS), assertions, inputs, first


def check_end_to_end(be, lib):
    from genstark_amd.errors import StarkError
    from genstark_amd.native import NativeProver
    f = PrimeField(backend=be)
    rng = random.Random(0x16)
    leaf = (lambda: rng.randrange(f.modulus)) if lib is lib224 else (lambda: (rng.randrange(f.modulus), rng.randrange(f.modulus)))
    leaves = [leaf() for _ in range(16)]
    tree, control = lib.poseidon_tree(f, leaves), lib.PoseidonMerkleTree(f, leaves)
    assert tree.deviceNodes is not None and tree.root == control.root
    indexes, new = [5, 4], [leaf(), leaf()]           # the second update changes the first one's sibling
    old_root = tree.root
    records = tree.updateMany(indexes, new)
    assert records[1].before[1] == new[0]
    for index, value, record in zip(indexes, new, records):
        leaves[index] = value
        assert record.root == lib.PoseidonMerkleTree(f, leaves).root
        stark, assertions, inputs, first = update_statement(lib, f, record, value, index, 4, old_root)
        nat = NativeProver(stark)
        proof = nat.prove_bytes(assertions, inputs, first)
        assert nat.verify_bytes(assertions, proof) is True
        with pytest.raises(StarkError):               # a wrong new root
            nat.verify_bytes(assertions[:-1] + [dict(assertions[-1], value=assertions[-1]['value'] ^ 1)], proof)
        old_root = record.root                        # the next statement's old root is this one's new root
    assert tree.root == old_root


@pytest.mark.gpu
def test_records_feed_the_merkle_update_stark_lib128(hip_backend):
    check_end_to_end(hip_backend, lib128)


@pytest.mark.gpu
def test_records_feed_the_merkle_update_stark_lib224():
    be = Backend(device=0, modulus=_abi.MODULUS_224)
    try:
        check_end_to_end(be, lib224)
    finally:
        be.close()


@pytest.mark.gpu
def test_bad_arguments_are_refused_by_the_library(hip_backend):
    f = PrimeField(backend=hip_backend)
    call = hip_backend.call
    rng = random.Random(2)
    h3, r3 = HadesHash(f, 3, 2, 1, 3), random_rescue(f, rng, 3, 2)
    tree = HadesMerkleTree(h3, [1, 2, 3, 4], 1)
    raw = tree.deviceNodes.toBuffer()
    nodes, buf = C.c_void_p(tree.deviceNodes.ptr), f.newMatrix(64, 2)
    ptr, one = C.c_void_p(buf.ptr), (C.c_uint64 * 2)(3, 4)
    other = Backend(device=0)
    try:
        fo = PrimeField(backend=other)
        for entry, foreign, digest in (('hades_merkle_update', HadesHash(fo, 3, 2, 1, 3), (1,)), ('rescue_merkle_update', random_rescue(fo, rng, 3, 2), ())):
            with pytest.raises(GstarkError, match=f'{entry}: the handle belongs to another context'):
                call('gs_' + entry, foreign.handle(), nodes, 4, *digest, one, ptr, 1, ptr, ptr)
    finally:
        other.close()
    for entry, h, digest in (('hades_merkle_update', h3, (1,)), ('rescue_merkle_update', r3, ())):
        for n in (3, 1, 0):
            with pytest.raises(GstarkError, match=f'{entry}: the number of leaves'):
                call('gs_' + entry, h.handle(), nodes, n, *digest, one, ptr, 1, ptr, ptr)
        with pytest.raises(GstarkError, match=f'{entry}: index 4 is outside of the 4 leaves'):
            call('gs_' + entry, h.handle(), nodes, 4, *digest, one, ptr, 2, ptr, ptr)
        with pytest.raises(GstarkError, match=f'{entry}: at most 2\\^20 updates'):
            call('gs_' + entry, h.handle(), nodes, 4, *digest, one, ptr, (1 << 20) + 1, ptr, ptr)
        call('gs_' + entry, h.handle(), nodes, 4, *digest, None, None, 0, None, None)         # an empty batch is no error
    for digest in (0, 2, 3):
        with pytest.raises(GstarkError, match='hades_merkle_update: nodes of'):
            call('gs_hades_merkle_update', h3.handle(), nodes, 4, digest, one, ptr, 1, ptr, ptr)
    assert tree.deviceNodes.toBuffer() == raw         # no refusal and no empty batch has touched the tree


# ---- the pin recorded before the family-neutral tree code got a unit of its own (csrc/field_tree.hip) ---------------------------------
FIELD_TREE_PIN = os.path.join(ROOT, 'tests', 'golden', 'field_tree_traffic.json')
FIELD_TREE_FLAVOURS = {'p128': None, 'q64': _abi.MODULUS_64}


def field_tree_sequence(be):
    """What tests/golden/make_field_tree_traffic.py records and the test below replays, per family (Poseidon with nodes of one and of two
    elements, Rescue): a tree of 8 leaves, five updates (leaf 5 and leaf 4 twice each — siblings, so `same` and `pred >= 0` occur — and
    leaf 2, whose sibling no update touches: `pred < 0`), proveMany of three indexes, pathRoots with and without replacing leaves, and a
    sparse tree of depth 3 with the same updates and the paths of a set and an unset index.  -> {family: {'traffic': Backend.traffic()
    over all of it, 'values': everything read back}}, tuples as lists (what JSON gives back)"""
    from genstark_amd.sparse_tree import HadesSparseMerkleTree, RescueSparseMerkleTree
    f = PrimeField(backend=be)
    p, rng = f.modulus, random.Random(0xF1E1D)
    plain = lambda v: [plain(x) for x in v] if isinstance(v, (list, tuple)) else v
    out = {}
    for name, h, digest in (('poseidon1', HadesHash(f, 3, 2, 1, 3), 1), ('poseidon2', HadesHash(f, 3, 2, 1, 6), 2), ('rescue', random_rescue(f, rng, 3, 2), 1)):
        rescue = isinstance(h, RescueHash)
        leaf = lambda: rng.randrange(p) if digest == 1 else (rng.randrange(p), rng.randrange(p))
        leaves, indexes, probe = [leaf() for _ in range(8)], [5, 4, 5, 2, 4], [4, 5, 0]
        new, replacing = [leaf() for _ in indexes], [leaf() for _ in probe]
        be.traffic(True)
        dense = RescueMerkleTree(h, f.newVectorFrom(leaves)) if rescue else HadesMerkleTree(h, leaves, digest)
        values = {'nodes': dense.nodes[1:]}
        values['records'] = [[r.before, r.root] for r in dense.updateMany(indexes, new)]
        values['nodes after'] = dense.nodes[1:]
        paths = dense.proveMany(probe)
        values['paths'] = paths
        values['path roots'] = type(dense).pathRoots(h, probe, paths)
        values['path roots of other leaves'] = type(dense).pathRoots(h, probe, paths, leaves=replacing)
        sparse = RescueSparseMerkleTree(h, 3) if rescue else HadesSparseMerkleTree(h, 3, digest)
        values['sparse empties'] = sparse.empties
        values['sparse records'] = [[r.before, r.root] for r in sparse.updateMany(indexes, new)]
        values['sparse root'], values['sparse stored'] = sparse.root, sparse.stored
        values['sparse paths'] = sparse.proveMany([5, 7])
        out[name] = {'traffic': be.traffic(), 'values': {key: plain(v) for key, v in values.items()}}
        be.traffic(False)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(FIELD_TREE_FLAVOURS))
def test_field_tree_matches_the_recorded_parent(name):
    """every launch (label, count, bytes, units) and every value of field_tree_sequence as the library computed them while the
    family-neutral kernels and drivers still stood in hades.hip and the two header templates"""
    with open(FIELD_TREE_PIN) as fh:
        want = json.load(fh)[name]
    be = Backend(device=0, modulus=FIELD_TREE_FLAVOURS[name]) if FIELD_TREE_FLAVOURS[name] else Backend(device=0)
    try:
        got = field_tree_sequence(be)
    finally:
        be.close()
    assert sorted(got) == sorted(want)
    for family in want:
        assert got[family]['traffic'] == want[family]['traffic'], family
        assert got[family]['values'] == want[family]['values'], family


# ---- node ---------------------------------------------------------------------------------------------------------------------------
def js_expectations(path):
    """what tests/js_tree_update.js must find, from host integers: per field a tree of pairs (width 6), a tree of single elements
    (width 3) and a Rescue tree (width 4, 3 rounds), 16 leaves each, with one batch of updates: repeats, a sibling pair, a no-op"""
    from test_rescue_hash import random_hash
    rng = random.Random(0x75)
    s = lambda v: [s(x) for x in v] if isinstance(v, (list, tuple)) else str(v)
    out = []
    for modulus in (_abi.MODULUS_128, _abi.MODULUS_64):
        f = HostField(modulus)
        h6, h3, hr = HadesHash(f, 5, 8, 55, 6), HadesHash(f, 3, 8, 5, 3), random_hash(f, rng, 4, 3)
        indexes = [5, 4, 5, 11, 4, 0, 15, 11]
        rec = {'modulus': str(modulus), 'indexes': indexes, 'rescue': {'alpha': '3', 'invAlpha': str(hr.invAlpha), 'rounds': 3, 'mds': s(hr.mds),
                                                                      'constants': s(hr.iConstants + [v for row in hr.cMatrix for v in row] + hr.cConstants)}}
        for key, digest, node in (('pairs', 2, lambda a, b: h6.hash(a + b)[:2]), ('singles', 1, lambda a, b: h3.hash(a + b)[:1]), ('rescued', 1, lambda a, b: [hr.hash2(a[0], b[0])])):
            leaves = [[rng.randrange(modulus) for _ in range(digest)] for _ in range(16)]
            new = [[rng.randrange(modulus) for _ in range(digest)] for _ in indexes]
            new[4] = new[1]                           # leaf 4 already holds it
            before, roots, snaps = stepwise_model(node, leaves, indexes, new, snapshots=(len(indexes),))
            flat = (lambda rows: rows) if digest == 2 else (lambda rows: [r[0] for r in rows])
            rec[key] = {'leaves': s(flat(leaves)), 'new': s(flat(new)), 'before': s([flat(b) for b in before]), 'roots': s(flat(roots)),
                        'nodes': s(flat(snaps[len(indexes)][1:]))}
        out.append(rec)
    with open(path, 'w') as fh:
        json.dump(out, fh)


@needs_node
def test_js_on_a_library_without_the_entries(tmp_path):
    """update and updateMany throw an Error that names what is missing"""
    run_js('tree_update', 'double', tmp_path, js_expectations)


@needs_node
@pytest.mark.gpu
def test_js_on_hip(tmp_path):
    run_js('tree_update', 'hip', tmp_path, js_expectations)


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    rng = random.Random(q % 65521)
    check_hades(be, rng, sizes=(64,), counts=(1, 65, 257))
    f = PrimeField(backend=be)
    h = random_rescue(f, rng, 3, 2)
    check_family(f, lambda leaves: RescueMerkleTree(h, f.newVectorFrom([v[0] for v in leaves])), lambda a, b: [h.hash2(a[0], b[0])], 1, rng, sizes=(64,), counts=(65,))
    print(f'runtime tree update: modulus {q} ok')
