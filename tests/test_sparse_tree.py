"""Sparse Merkle trees of fixed depth on the device: include/gstark_sparse_tree.h, csrc/sparse_tree_plan.h, csrc/field_tree.hip,
genstark_amd/sparse_tree.py, the sparse classes of js/field_tree.js.

The definition is the oracle: a sparse tree of depth d is the dense tree of 2^d leaves that all hold `empty` until set, so for small
depths the dense trees (which have tests of their own) must agree on every root, path and record, bit for bit.  Every comparison is
equality.  CPU tier: the header and the binding table, the host plan on its own under the sanitizers
(tests/host_harness/sparse_tree_plan_host.cpp), the host fallback on the tests' double against the dense host tree and, at depth 36,
against a dict model, and the refusals.  GPU tier: the three kernels and the shared driver under both families at the seams of a wave
and of a workgroup in three field flavours and the runtime-modulus one, depth 36, the update statements of lib128 / lib224 at depth 32
proved from the records, the library's refusals and the node binding.  `python tests/test_sparse_tree.py runtime <q>` is the check of
the runtime-modulus flavour (one modulus per process)."""
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
from genstark_amd.field import Matrix, PrimeField
from genstark_amd.field_tree import TreeUpdate, verify_path
from genstark_amd.hades import HadesHash, HadesMerkleTree
from genstark_amd.hostfield import HostField
from genstark_amd.rescue_hash import RescueHash, RescueMerkleTree, rescue2x64, rescue4x128
from genstark_amd.sparse_tree import HadesSparseMerkleTree, RescueSparseMerkleTree, SparseFieldMerkleTree
from sponge_common import ROOT, check_header_is_plain_c, check_symbol_table, flavour_fixture, needs_node, run_js

DEEP = [0, 1, 2**32 - 1, 2**32, 2**35, 2**36 - 2, 2**36 - 1]      # the indexes of the depth-36 tests: both ends, and bits 32 .. 35


# ---- CPU tier: header and binding table -------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    check_header_is_plain_c('sparse_tree')


def test_symbol_table_matches_the_header():
    assert _abi.SPARSE_TREE_SYMBOLS == ('gs_hades_sparse_create', 'gs_rescue_sparse_create', 'gs_sparse_update', 'gs_sparse_paths', 'gs_sparse_root', 'gs_sparse_empties',
                                        'gs_sparse_stored', 'gs_sparse_destroy')
    check_symbol_table('sparse_tree', _abi.SPARSE_TREE_SYMBOLS, (_abi.EXPORTED_SYMBOLS, _abi.OPTIONAL_SYMBOLS, _abi.HADES_SYMBOLS, _abi.RESCUE_SYMBOLS,
                                                                 _abi.TREE_UPDATE_SYMBOLS, _abi.TREE_VERIFY_SYMBOLS))
    header = open(os.path.join(ROOT, 'include', 'gstark_sparse_tree.h')).read()
    for limit in ('2^20', '2^31', '1 .. 36', 'up to d stored'):       # the caps and the cost of a leaf are part of the contract
        assert limit in header, limit
    addon = open(os.path.join(ROOT, 'napi', 'gstark_napi.cc')).read()
    for name in _abi.SPARSE_TREE_SYMBOLS:             # (gs_sparse_stored returns a count, which the addon's call() does not deliver)
        assert (f'{{"{name}", "' in addon) == (name != 'gs_sparse_stored'), name


def test_every_flavour_of_the_library_exports_the_entries():
    for path in list(_abi.HIP_LIB_PATHS.values()) + [_abi.HIP_LIB_PATH_RUNTIME]:
        lib = _abi.load_library(path)
        assert all(hasattr(lib, name) for name in _abi.SPARSE_TREE_SYMBOLS), path


def test_the_double_lacks_the_entries(oracle_backend):
    assert not any(hasattr(oracle_backend.lib, name) for name in _abi.SPARSE_TREE_SYMBOLS)


def test_a_device_hash_on_a_library_without_the_entries_is_an_error(oracle_backend):
    class OnDevice(HadesHash):
        onDevice = True
    with pytest.raises(GstarkError, match=r'HadesSparseMerkleTree: the library has no gs_hades_sparse_create \(include/gstark_sparse_tree.h\)'):
        HadesSparseMerkleTree(OnDevice(PrimeField(backend=oracle_backend), 3, 2, 1, 3), 3, 1)


# ---- CPU tier: the host plan on its own ---------------------------------------------------------------------------------------------
def test_plan_against_the_map_model_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'sparse_tree_plan_host')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-omit-frame-pointer', os.path.join(ROOT, 'tests', 'host_harness', 'sparse_tree_plan_host.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'calls ok' in r.stdout and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


# ---- the families and the models ----------------------------------------------------------------------------------------------------
def random_rescue(f, rng, width, rounds):
    p = f.modulus
    return RescueHash(f, 3, -3, width, rounds, [[rng.randrange(p) for _ in range(width)] for _ in range(width)], [rng.randrange(p) for _ in range(width * (width + 2))])


class Family:
    """sparse(depth, empty, slots_hint) and dense(leaves) over one hash, leaves in the shape the classes take, node(left, right) on rows"""

    def __init__(self, name, hash, digest):
        self.name, self.hash, self.digest, self.field = name, hash, digest, hash.field
        self.rescue = isinstance(hash, RescueHash)
        self.cls = RescueMerkleTree if self.rescue else HadesMerkleTree

    def sparse(self, depth, empty=None, slots_hint=1):
        return RescueSparseMerkleTree(self.hash, depth, empty, slots_hint) if self.rescue else HadesSparseMerkleTree(self.hash, depth, self.digest, empty, slots_hint)

    def dense(self, leaves):
        f = self.field
        if self.hash.onDevice:                        # leaves on the device: nothing goes through the host
            leaves = f.newVectorFrom(list(leaves)) if self.rescue else f.newMatrixFrom([[v] if self.digest == 1 else list(v) for v in leaves])
        return RescueMerkleTree(self.hash, leaves) if self.rescue else HadesMerkleTree(self.hash, leaves, self.digest)

    def leaf(self, rng):
        p = self.field.modulus
        return rng.randrange(p) if self.digest == 1 else (rng.randrange(p), rng.randrange(p))

    def rows(self, shaped):
        return [shaped] if self.digest == 1 else list(shaped)

    def node(self, left, right):
        return [self.hash.hash2(left[0], right[0])] if self.rescue else self.hash.hash(left + right)[:self.digest]

    def verify(self, root, index, path):
        shape = (lambda r: r[0]) if self.digest == 1 else tuple
        return verify_path(root, index, path, lambda a, b: shape(self.node(self.rows(a), self.rows(b))))


def hades_families(f):
    return [Family('hades1', HadesHash(f, 3, 2, 1, 3), 1), Family('hades2', HadesHash(f, 3, 2, 1, 6), 2)]      # few rounds: the host follows


class DictModel:
    """the dense tree of 2^depth leaves on host rows, one dict keyed by heap number: what is not in it is empties[level]"""

    def __init__(self, family, depth, empty):
        self.family, self.depth, self.held = family, depth, {}
        self.empties = [family.rows(empty)]
        for _ in range(depth):
            self.empties.append(family.node(self.empties[-1], self.empties[-1]))
        self.shape = (lambda r: r[0]) if family.digest == 1 else tuple

    def at(self, heap):
        return self.held.get(heap, self.empties[self.depth + 1 - heap.bit_length()])

    @property
    def root(self):
        return self.shape(self.at(1))

    def prove(self, index):
        heap = (1 << self.depth) + index
        return [self.shape(self.at(heap))] + [self.shape(self.at((heap >> l) ^ 1)) for l in range(self.depth)]

    def update(self, index, leaf):
        before = self.prove(index)
        heap = (1 << self.depth) + index
        self.held[heap] = self.family.rows(leaf)
        while heap > 1:
            heap >>= 1
            self.held[heap] = self.family.node(self.at(2 * heap), self.at(2 * heap + 1))
        return TreeUpdate(before, self.root)


def batches(n, k, rng):
    """name -> (indexes set by a call of their own before the batch, the batch of k indexes): the patterns of the dense update tests
    and three that only a sparse tree tells apart"""
    from test_tree_update import index_patterns
    out = {name: ([], indexes) for name, indexes in index_patterns(n, k, rng).items()}
    order = list(range(n))
    rng.shuffle(order)
    out['all new'] = ([], [order[j % n] for j in range(k)])                   # (new as long as the tree has leaves left)
    held = order[:min(n, 5)]
    out['all repeated'] = (held, [rng.choice(held) for _ in range(k)])
    evens = [2 * (i // 2) for i in order[:max(1, min(n, k) // 2)]]
    later = [a | 1 for a in evens] + evens                                    # the right leaf first: its sibling is created later in the batch
    out['siblings created later'] = ([], [later[j % len(later)] for j in range(k)])
    return out


def new_leaves(family, rng, tree_leaf, indexes, empty):
    """one leaf per index: random ones, some the leaf the tree holds at the call, some `empty` again"""
    new = [family.leaf(rng) for _ in indexes]
    for j in range(5, len(new), 11):
        new[j] = tree_leaf(indexes[j])
    for j in range(7, len(new), 13):
        new[j] = empty
    return new


def check_against_dense(family, depths, counts, rng, patterns=None):
    """the same calls on the sparse tree (slots_hint=1: the store doubles inside the run) and on the dense tree of [empty] * 2^depth"""
    f, n_checked = family.field, 0
    for depth in depths:
        n = 1 << depth
        for nonzero in (False, True):
            empty = family.leaf(rng) if nonzero else (0 if family.digest == 1 else (0, 0))
            fresh = family.dense([empty] * n)
            nodes = fresh.nodes
            probe = family.sparse(depth, empty if nonzero else None)
            assert probe.root == fresh.root and probe.depth == depth and probe.digest == family.digest and probe.stored == [0] * (depth + 1)
            assert probe.empties == [nodes[n >> l] for l in range(depth + 1)], (family.name, depth)      # the dense tree's leftmost node of each level
            assert probe.proveMany(range(n)) == fresh.proveMany(range(n)) and probe.updateMany([], []) == []
            for name, (held, indexes) in batches(n, max(counts), rng).items():
                if patterns and name not in patterns:
                    continue
                first = [family.leaf(rng) for _ in held]
                new = new_leaves(family, rng, lambda i: first[held.index(i)] if i in held else empty, indexes, empty)
                # before[j] and root[j] do not depend on what follows: ONE dense run of max(counts) updates serves every count as a prefix
                top = max(counts)
                dense = family.dense([empty] * n)
                first_records = dense.updateMany(held, first)
                want = dense.updateMany(indexes[:top], new[:top])
                for k in counts:
                    where = (family.name, depth, nonzero, name, k)
                    sparse = family.sparse(depth, empty if nonzero else None)
                    assert sparse.updateMany(held, first) == first_records, where
                    records = sparse.updateMany(indexes[:k], new[:k])
                    assert records == want[:k], where
                    assert all(isinstance(r, TreeUpdate) for r in records) and sparse.root == records[-1].root, where
                    touched = set(held) | set(indexes[:k])
                    assert sparse.stored[0] == len(touched) and sparse.stored[depth] == 1, where
                    if k == top:
                        assert sparse.root == dense.root and sparse.proveMany(range(n)) == dense.proveMany(range(n)), where
                        assert sparse.getMany(indexes[:3]) == [dense.prove(i)[0] for i in indexes[:3]], where
                    n_checked += 1
                # two calls back to back equal one call of the concatenation, and the tree between two counts
                k = counts[-2] if len(counts) > 1 else counts[0]
                cut = k // 3
                sparse, dense = family.sparse(depth, empty if nonzero else None), family.dense([empty] * n)
                sparse.updateMany(held, first), dense.updateMany(held, first)
                records = (sparse.updateMany(indexes[:cut], new[:cut]) if cut else []) + sparse.updateMany(indexes[cut:k], new[cut:k])
                assert records == dense.updateMany(indexes[:k], new[:k]) and sparse.root == dense.root, (family.name, depth, nonzero, name, 'two calls')
                assert sparse.proveMany(range(n)) == dense.proveMany(range(n)), (family.name, depth, nonzero, name, 'two calls')
                if getattr(f, 'backend', None) is not None:
                    paths = sparse.proveMany(range(n), device=True)
                    assert isinstance(paths, Matrix) and (paths.rowCount, paths.colCount) == (n, (depth + 1) * family.digest)
                    assert family.cls.verifyMany(sparse.root, list(range(n)), paths, family.hash) == [True] * n
    return n_checked


# ---- CPU tier: the host fallback ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', [1, 2, 6])
def test_host_fallback_equals_the_dense_host_tree(oracle_backend, depth):
    rng = random.Random(0x5A + depth)
    f = PrimeField(backend=oracle_backend)
    for family in hades_families(f) + [Family('rescue', random_rescue(f, rng, 3, 2), 1), Family('hostfield', HadesHash(HostField(f.modulus), 3, 2, 1, 3), 1)]:
        assert not family.hash.onDevice
        assert check_against_dense(family, [depth], (1, 5, 40), rng) == 2 * 9 * 3


def test_host_fallback_of_the_library_trees(oracle_backend):
    rng = random.Random(0x128)
    f = PrimeField(backend=oracle_backend)
    sparse, dense = lib128.poseidon_sparse_tree(f, 2), lib128.poseidon_tree(f, [(0, 0)] * 4)
    assert isinstance(sparse, HadesSparseMerkleTree) and sparse.digest == 2 and sparse.root == dense.root
    new = [(rng.randrange(f.modulus), rng.randrange(f.modulus)) for _ in range(3)]
    assert sparse.updateMany([3, 2, 3], new) == dense.updateMany([3, 2, 3], new) and sparse.proveMany(range(4)) == dense.proveMany(range(4))
    from test_wide_fields import oracle_for
    be = oracle_for('p224')
    try:
        f224 = PrimeField(backend=be)
        sparse, dense = lib224.poseidon_sparse_tree(f224, 2, empty=9), lib224.poseidon_tree(f224, [9] * 4)
        assert sparse.digest == 1 and sparse.update(1, 5) == dense.update(1, 5) and sparse.root == dense.root and sparse.get(0) == 9
    finally:
        be.close()


def check_depth_36(family, rng, on_device):
    """set and absent indexes at depth 36 against the dict model; every path verifies on the host, and on the device where the tree is"""
    depth = 36
    for empty in (None, family.leaf(rng)):
        zero = 0 if family.digest == 1 else (0, 0)
        tree, model = family.sparse(depth, empty, slots_hint=1), DictModel(family, depth, zero if empty is None else empty)
        assert tree.empties == [model.shape(r) for r in model.empties] and tree.root == tree.empties[depth]
        new = [family.leaf(rng) for _ in range(2)]
        first = tree.updateMany([5, 4], new)          # from an empty tree: the second one's sibling is the first one's leaf
        assert tree.getMany([5, 4]) == new
        assert first[0].before[1] == tree.empties[0] and first[1].before[1] == new[0] and first[0].before[0] == tree.empties[0]
        assert first == [model.update(5, new[0]), model.update(4, new[1])]
        indexes = DEEP + [rng.randrange(1 << depth) for _ in range(5)] + [DEEP[3], 5]
        leaves = [family.leaf(rng) for _ in indexes]
        root = tree.root
        records = tree.updateMany(indexes, leaves)
        assert records == [model.update(i, v) for i, v in zip(indexes, leaves)] and tree.root == model.root
        absent = [3, 2**32 + 1, 2**35 + 2**33, 2**36 - 3] + [rng.randrange(1 << depth) for _ in range(3)]
        probe = indexes + absent
        paths = tree.proveMany(probe)
        assert paths == [model.prove(i) for i in probe]
        assert all(family.verify(tree.root, i, path) for i, path in zip(probe, paths))
        assert all(path[0] == tree.empties[0] for path in paths[len(indexes):])      # the non-membership paths start with `empty`
        assert tree.getMany(indexes[-2:] + absent[:1]) == [leaves[-2], leaves[-1], tree.empties[0]]
        on_the_device = tree.proveMany(probe, device=True)
        assert family.cls.pathRoots(family.hash, probe, on_the_device, digest=family.digest) == [tree.root] * len(probe)
        assert family.cls.verifyMany(tree.root, probe, on_the_device, family.hash) == [True] * len(probe)
        assert family.cls.verifyUpdates(root, indexes, leaves, records, family.hash) == [True] * len(records)
        p = family.field.modulus
        altered = list(records[3].before)
        altered[20] = (altered[20] + 1) % p if family.digest == 1 else (altered[20][0], (altered[20][1] + 1) % p)
        forged = records[:3] + [TreeUpdate(altered, records[3].root)] + records[4:]
        assert family.cls.verifyUpdates(root, indexes, leaves, forged, family.hash) == [True] * 3 + [False] + [True] * (len(records) - 4)
        stored = tree.stored
        assert stored[0] == len(set(indexes) | {4, 5}) and stored[depth] == 1 and all(1 <= s <= stored[0] for s in stored)
        assert (tree._tree is not None) == on_device
        # every stored leaf back to `empty`: the root of the tree with nothing stored, and nothing pruned
        everything = sorted(set(indexes) | {4, 5})
        tree.updateMany(everything, [tree.empties[0]] * len(everything))
        assert tree.root == tree.empties[depth] and tree.stored == stored


def test_host_fallback_at_depth_36(oracle_backend):
    rng = random.Random(0x36)
    f = PrimeField(backend=oracle_backend)
    for family in hades_families(f) + [Family('rescue', random_rescue(f, rng, 3, 2), 1)]:
        check_depth_36(family, rng, on_device=False)


def test_refusals(oracle_backend):
    f = PrimeField(backend=oracle_backend)
    h3, h6 = HadesHash(f, 3, 2, 1, 3), HadesHash(f, 3, 2, 1, 6)
    r3 = RescueHash(f, 3, -3, 3, 2, [[1, 2, 3], [4, 5, 7], [9, 8, 11]], list(range(1, 16)))
    for depth in (0, 37, -1):
        with pytest.raises(GstarkError, match=f'^HadesSparseMerkleTree: a depth of 1 .. 36, not {depth}'):
            HadesSparseMerkleTree(h3, depth, 1)
        with pytest.raises(GstarkError, match=f'^RescueSparseMerkleTree: a depth of 1 .. 36, not {depth}'):
            RescueSparseMerkleTree(r3, depth)
    for h, digest in ((h3, 2), (h6, 3), (h3, 0)):
        with pytest.raises(GstarkError, match=f'^HadesSparseMerkleTree: nodes of {digest} elements'):       # a digest that does not fit the width
            HadesSparseMerkleTree(h, 4, digest)
    with pytest.raises(GstarkError, match='^RescueSparseMerkleTree: two nodes do not fit a state of 2'):       # the Rescue width that holds no tree
        RescueSparseMerkleTree(RescueHash(f, 3, -3, 2, 2, [[1, 2], [3, 5]], list(range(1, 9))), 4)
    with pytest.raises(GstarkError, match='slots_hint is 1 .. 2\\^31'):
        HadesSparseMerkleTree(h3, 4, 1, slots_hint=0)
    with pytest.raises(GstarkError, match='HadesSparseMerkleTree: every leaf has 2 elements'):
        HadesSparseMerkleTree(h6, 4, 2, empty=7)
    single, pairs, rescue = HadesSparseMerkleTree(h3, 3, 1), HadesSparseMerkleTree(h6, 36, 2, empty=(3, 4)), RescueSparseMerkleTree(r3, 3)
    for tree, leaf in ((single, 7), (pairs, (7, 8)), (rescue, 7)):
        tree.updateMany([1, 0], [leaf, leaf])
        root, stored, n = tree.root, tree.stored, 1 << tree.depth
        for bad in (n, -1):
            with pytest.raises(GstarkError, match=f'^{tree._who}: index {bad} is outside of the 2\\^{tree.depth} leaves'):
                tree.updateMany([0, bad], [leaf, leaf])
            with pytest.raises(GstarkError, match='outside'):
                tree.update(bad, leaf)
            with pytest.raises(GstarkError, match=f'^{tree._who}: index {bad} is outside'):
                tree.proveMany([0, bad])
            with pytest.raises(GstarkError, match='outside'):
                tree.get(bad)
        many = [0] * ((1 << 20) + 1)
        with pytest.raises(GstarkError, match=f'^{tree._who}: at most 2\\^20 updates per call'):
            tree.updateMany(many, [leaf] * len(many))
        with pytest.raises(GstarkError, match=f'^{tree._who}: at most 2\\^20 paths per call'):
            tree.proveMany(many)
        for indexes, leaves in (([0, 1], [leaf]), ([0], [leaf, leaf]), ([], [leaf]), ([0], [])):
            with pytest.raises(GstarkError, match=f'^{tree._who}: {len(indexes)} indexes and {len(leaves)} leaves'):
                tree.updateMany(indexes, leaves)
        assert tree.updateMany([], []) == [] and tree.proveMany([]) == []
        with pytest.raises(GstarkError, match='no node array'):
            tree.nodes
        assert tree.root == root and tree.stored == stored       # a refused call and an empty one leave the tree as it was
    for tree, bad in ((single, (7, 8)), (pairs, 7), (pairs, (7,)), (pairs, (7, 8, 9)), (rescue, (7, 8))):
        root = tree.root
        with pytest.raises(GstarkError, match=f'^{tree._who}: every leaf has {tree.digest} elements'):
            tree.updateMany([0], [bad])
        assert tree.root == root
    assert issubclass(HadesSparseMerkleTree, SparseFieldMerkleTree) and issubclass(HadesSparseMerkleTree, HadesMerkleTree)


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 257, 1000)                   # the seams of a wave (64 lanes) and of a workgroup (256 threads)
DEPTHS = (1, 2, 3, 9)

flavour = flavour_fixture()


@pytest.mark.gpu
@pytest.mark.parametrize('digest', [1, 2])
def test_seams_against_the_dense_device_tree(flavour, digest):
    f = PrimeField(backend=flavour)
    family = hades_families(f)[digest - 1]
    assert family.hash.onDevice and family.sparse(3)._tree is not None
    assert check_against_dense(family, DEPTHS, COUNTS, random.Random(0x5EA + digest)) == len(DEPTHS) * 2 * 9 * len(COUNTS)


@pytest.mark.gpu
def test_depth_36_on_the_device(flavour):
    rng = random.Random(0x3636)
    for family in hades_families(PrimeField(backend=flavour)):
        check_depth_36(family, rng, on_device=True)


@pytest.mark.gpu
def test_rescue_of_the_reference_shape(hip_backend):
    """rescue4x128 at depth 9: its 32 rounds cost the host milliseconds per node, so the model remembers the nodes it has computed and most
    of the batch moves four neighbouring leaves between two values each"""
    f = PrimeField(backend=hip_backend)
    rng = random.Random(0x4E5C)
    family = Family('rescue4x128', rescue4x128(f), 1)
    seen, plain = {}, family.node

    def node(a, b):
        key = (a[0], b[0])
        if key not in seen:
            seen[key] = plain(a, b)
        return seen[key]
    family.node = node
    depth, p = 9, f.modulus
    tree, model = family.sparse(depth, slots_hint=1), DictModel(family, depth, 0)
    assert tree.empties == [r[0] for r in model.empties]
    base = 4 * rng.randrange((1 << depth) // 4)
    pool = [[rng.randrange(p), rng.randrange(p)] for _ in range(4)]
    indexes = [rng.randrange(1 << depth) for _ in range(12)] + [base + rng.randrange(4) for _ in range(288)]
    new = [rng.randrange(p) for _ in range(12)] + [rng.choice(pool[i - base]) for i in indexes[12:]]
    want = [model.update(i, v) for i, v in zip(indexes, new)]
    assert tree.updateMany(indexes[:65], new[:65]) + tree.updateMany(indexes[65:], new[65:]) == want and tree.root == model.root
    probe = indexes[:4] + [base, base + 3, 0, (1 << depth) - 1]
    assert tree.proveMany(probe) == [model.prove(i) for i in probe]
    assert RescueMerkleTree.verifyMany(tree.root, probe, tree.proveMany(probe, device=True), family.hash) == [True] * len(probe)


@pytest.mark.gpu
def test_rescue_in_another_flavour_against_the_dense_device_tree():
    be = Backend(device=0, modulus=_abi.MODULUS_64)
    try:
        f = PrimeField(backend=be)
        rng = random.Random(0x264)
        family = Family('rescue', random_rescue(f, rng, 3, 2), 1)
        assert check_against_dense(family, (1, 2, 9), (1, 65, 300), rng) == 3 * 2 * 9 * 3
        check_depth_36(family, rng, on_device=True)
        h2 = rescue2x64(f)                            # (held: a handle lives as long as its hash object)
        with pytest.raises(GstarkError, match='RescueSparseMerkleTree: two nodes do not fit'):
            RescueSparseMerkleTree(h2, 9)
        tree = C.c_void_p()
        with pytest.raises(GstarkError, match='rescue_sparse_create: two nodes do not fit'):
            be.call('gs_rescue_sparse_create', h2.handle(), 9, None, 1, C.byref(tree))
        assert not tree.value
    finally:
        be.close()


@pytest.mark.gpu
def test_families_interleaved_on_one_context():
    """a tree reaches its family's hash through a pointer it carries: calls on a Poseidon sparse tree, a Rescue sparse tree and a dense
    tree of each family, alternating call by call on one context, give what the same calls give on fresh trees one tree at a time"""
    be = Backend(device=0, modulus=_abi.MODULUS_64)
    try:
        f = PrimeField(backend=be)
        rng = random.Random(0x1A7E)
        poseidon, rescue = hades_families(f)[0], Family('rescue', random_rescue(f, rng, 3, 2), 1)
        depth, indexes = 3, [5, 4, 5, 2]               # a repeat, a sibling pair, a leaf of its own
        makers = [lambda: poseidon.sparse(depth), lambda: rescue.sparse(depth), lambda: poseidon.dense([0] * 8), lambda: rescue.dense([0] * 8)]
        new = [[family.leaf(rng) for _ in indexes] for family in (poseidon, rescue)] * 2        # the same leaves for a family's two trees

        def calls(tree, leaves, j):
            return [tree.update(indexes[j], leaves[j]), tree.root, tree.proveMany(range(8))]
        alone = []
        for make, leaves in zip(makers, new):
            tree = make()
            alone.append([calls(tree, leaves, j) for j in range(len(indexes))])
        trees = [make() for make in makers]
        mixed = [[] for _ in trees]
        for j in range(len(indexes)):
            for k, (tree, leaves) in enumerate(zip(trees, new)):
                mixed[k].append(calls(tree, leaves, j))
        assert mixed == alone
        assert mixed[0] == mixed[2] and mixed[1] == mixed[3] and mixed[0] != mixed[1]      # sparse = dense within a family; the families differ
    finally:
        be.close()


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    from test_runtime_modulus import PRIMES
    q = PRIMES[12]                                    # 127 bits
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(q)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'runtime sparse tree: modulus {q} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


def update_statement(lib, f, record, new_leaf, index, depth, old_root):
    """ComputeMerkleUpdate of `lib` for one record of updateMany: (stark, assertions "old root, new root", inputs, first row).  Each path
    runs hash(h, node) in the first half of its registers and hash(node, h) in the second; the next level picks one by the index bit, and
    the root is in the half the TOP bit of the index names — the second one for the keys of the upper half of the key space"""
    from genstark_amd._mirror.stark import Stark
    from test_lib128 import OPTS
    bits = [(index >> j) & 1 for j in range(depth)]                      # least significant bit first ...
    top, bits = bits[-1], [0] + bits[:-1]                                # ... shifted as tests/test_lib128.py shifts them
    air = lib.compute_merkle_update_air(f, depth)
    inputs, first = lib.merkle_update_inputs(f, record.before[0], new_leaf, record.before[1:], bits)
    last = 64 * depth - 1
    at = lambda register, value: {'step': last, 'register': register, 'value': value}
    if lib is lib128:
        assertions = [at(6 * top, old_root[0]), at(6 * top + 1, old_root[1]), at(12 + 6 * top, record.root[0]), at(12 + 6 * top + 1, record.root[1])]
    else:
        assertions = [at(3 * top, old_root), at(6 + 3 * top, record.root)]
    return Stark(air, OPTS), assertions, inputs, first


def check_end_to_end(be, lib):
    """a tree no dense class can hold: two updates at depth 32, each record proved as ComputeMerkleUpdate"""
    from genstark_amd.errors import StarkError
    from genstark_amd.native import NativeProver
    f = PrimeField(backend=be)
    rng = random.Random(0x32)
    depth, p = 32, f.modulus
    leaf = (lambda: rng.randrange(p)) if lib is lib224 else (lambda: (rng.randrange(p), rng.randrange(p)))
    tree = lib.poseidon_sparse_tree(f, depth)
    assert tree._tree is not None and tree.depth == depth and tree.root == tree.empties[depth]
    indexes, new = [2**31 + 5, 2**31 + 4], [leaf(), leaf()]          # the second update changes the first one's sibling
    old_root = tree.root
    records = tree.updateMany(indexes, new)
    assert records[0].before[:2] == [tree.empties[0]] * 2 and records[1].before[1] == new[0]
    for index, value, record in zip(indexes, new, records):
        stark, assertions, inputs, first = update_statement(lib, f, record, value, index, depth, old_root)
        nat = NativeProver(stark)
        proof = nat.prove_bytes(assertions, inputs, first)
        assert nat.verify_bytes(assertions, proof) is True
        with pytest.raises(StarkError):               # a wrong new root
            nat.verify_bytes(assertions[:-1] + [dict(assertions[-1], value=assertions[-1]['value'] ^ 1)], proof)
        old_root = record.root                        # the next statement's old root is this one's new root
    assert tree.root == old_root and tree.stored == [2] + [1] * depth


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
    """every call here is refused on the host before anything is launched, or is an empty batch.  A tree whose hash has been destroyed
    is refused by the library's registry of live hash handles: the freed handle is looked up, never dereferenced"""
    f = PrimeField(backend=hip_backend)
    call, lib = hip_backend.call, hip_backend.lib
    rng = random.Random(2)
    h3, r3 = HadesHash(f, 3, 2, 1, 3), random_rescue(f, rng, 3, 2)
    tree = HadesSparseMerkleTree(h3, 3, 1, slots_hint=1)
    tree.updateMany([1, 6], [7, 8])
    root, stored = tree.root, tree.stored
    buf = f.newMatrix(64, 2)
    ptr, two, out = C.c_void_p(buf.ptr), (C.c_uint64 * 2)(3, 8), C.c_void_p()
    for create, h, digest in (('gs_hades_sparse_create', h3, (1,)), ('gs_rescue_sparse_create', r3, ())):
        who = create[3:]
        assert getattr(lib, create)(hip_backend.ctx, None, 3, *digest, None, 1, C.byref(out)) != 0 and not out.value        # a null hash handle
        assert getattr(lib, create)(hip_backend.ctx, h.handle(), 3, *digest, None, 1, None) != 0
        for depth in (0, 37):
            with pytest.raises(GstarkError, match=f'{who}: a depth of 1 .. 36, not {depth}'):
                call(create, h.handle(), depth, *digest, None, 1, C.byref(out))
        with pytest.raises(GstarkError, match=f'{who}: slots_hint is 1 .. 2\\^31'):
            call(create, h.handle(), 3, *digest, None, 0, C.byref(out))
        assert not out.value
    for digest in (0, 2, 3):
        with pytest.raises(GstarkError, match='hades_sparse_create: nodes of'):
            call('gs_hades_sparse_create', h3.handle(), 3, digest, None, 1, C.byref(out))
    other = Backend(device=0)
    try:
        ho = HadesHash(PrimeField(backend=other), 3, 2, 1, 3)                # (held: a handle lives as long as its hash object)
        with pytest.raises(GstarkError, match='hades_sparse_create: the handle belongs to another context'):
            call('gs_hades_sparse_create', ho.handle(), 3, 1, None, 1, C.byref(out))
        foreign = HadesSparseMerkleTree(ho, 3, 1)
        with pytest.raises(GstarkError, match='sparse_update: the tree belongs to another context'):
            call('gs_sparse_update', foreign._tree, two, ptr, 1, ptr, ptr)
        with pytest.raises(GstarkError, match='sparse_paths: the tree belongs to another context'):
            call('gs_sparse_paths', foreign._tree, two, 1, ptr)
        del foreign, ho
    finally:
        other.close()
    t = tree._tree
    for entry, args in (('gs_sparse_update', (two, ptr, 1, ptr, ptr)), ('gs_sparse_paths', (two, 1, ptr)), ('gs_sparse_root', (ptr,)), ('gs_sparse_empties', (ptr,))):
        assert getattr(lib, entry)(hip_backend.ctx, None, *args) != 0                 # a null tree
    assert lib.gs_sparse_stored(None, 0) == 0 and lib.gs_sparse_stored(t, 4) == 0 and lib.gs_sparse_stored(t, 0) == 2
    assert lib.gs_sparse_destroy(hip_backend.ctx, None) == 0
    with pytest.raises(GstarkError, match='sparse_update: index 8 is outside of the 2\\^3 leaves'):
        call('gs_sparse_update', t, two, ptr, 2, ptr, ptr)
    with pytest.raises(GstarkError, match='sparse_paths: index 8 is outside of the 2\\^3 leaves'):
        call('gs_sparse_paths', t, two, 2, ptr)
    with pytest.raises(GstarkError, match='sparse_update: at most 2\\^20 updates'):
        call('gs_sparse_update', t, two, ptr, (1 << 20) + 1, ptr, ptr)
    with pytest.raises(GstarkError, match='sparse_paths: at most 2\\^20 paths'):
        call('gs_sparse_paths', t, two, (1 << 20) + 1, ptr)
    for args in ((None, ptr, 1, ptr, ptr), (two, None, 1, ptr, ptr), (two, ptr, 1, None, ptr), (two, ptr, 1, ptr, None)):
        assert lib.gs_sparse_update(hip_backend.ctx, t, *args) != 0
    assert lib.gs_sparse_paths(hip_backend.ctx, t, two, 1, None) != 0 and lib.gs_sparse_root(hip_backend.ctx, t, None) != 0
    call('gs_sparse_update', t, None, None, 0, None, None)                   # an empty batch is no error
    call('gs_sparse_paths', t, None, 0, None)
    assert tree.root == root and tree.stored == stored                       # no refusal and no empty batch has touched the tree
    # a destroyed tree's hash, through the raw entries: the tree is refused by every entry that would use it, a create over the dead handle too
    for create, destroy, h, digest in (('gs_hades_sparse_create', 'gs_hades_destroy', HadesHash(f, 3, 2, 1, 3), (1,)), ('gs_rescue_sparse_create', 'gs_rescue_destroy', random_rescue(f, rng, 3, 2), ())):
        orphan, dead = C.c_void_p(), h.handle()
        call(create, dead, 3, *digest, None, 1, C.byref(orphan))
        es = f.elementSize                            # (alive: served — leaf, witness and root in three parts of the buffer)
        call('gs_sparse_update', orphan, (C.c_uint64 * 1)(2), C.c_void_p(buf.ptr + 64 * es), 1, ptr, C.c_void_p(buf.ptr + 96 * es))
        call(destroy, dead)
        h._handle = None                              # (the object does not destroy it a second time)
        for entry, args in (('gs_sparse_update', (two, ptr, 1, ptr, ptr)), ('gs_sparse_paths', (two, 1, ptr)), ('gs_sparse_root', (ptr,)), ('gs_sparse_empties', (ptr,))):
            with pytest.raises(GstarkError, match=f"{entry[3:]}: the tree's hash has been destroyed"):
                call(entry, orphan, *args)
        with pytest.raises(GstarkError, match=f'{create[3:]}: the hash has been destroyed'):
            call(create, dead, 3, *digest, None, 1, C.byref(out))
        assert not out.value and lib.gs_sparse_stored(orphan, 0) == 1
        call('gs_sparse_destroy', orphan)             # the tree itself can still be destroyed


# ---- node ---------------------------------------------------------------------------------------------------------------------------
def js_expectations(path):
    """what tests/js_sparse_tree.js must find, from the host fallback (which the CPU tier holds against the dense tree and the dict
    model): per field, at depth 3 and 36, a tree of pairs, a tree of single elements and a Rescue tree with one batch each — repeats, a
    sibling pair created right leaf first, an index above 2^32, a leaf set back to `empty` — and paths of set and absent indexes"""
    from test_rescue_hash import random_hash
    rng = random.Random(0x75)
    s = lambda v: [s(x) for x in v] if isinstance(v, (list, tuple)) else str(v)
    out = []
    for modulus in (_abi.MODULUS_128, _abi.MODULUS_64):
        f = HostField(modulus)
        h6, h3, hr = HadesHash(f, 5, 8, 55, 6), HadesHash(f, 3, 8, 5, 3), random_hash(f, rng, 4, 3)
        rec = {'modulus': str(modulus), 'rescue': {'alpha': '3', 'invAlpha': str(hr.invAlpha), 'rounds': 3, 'mds': s(hr.mds),
                                                   'constants': s(hr.iConstants + [v for row in hr.cMatrix for v in row] + hr.cConstants)}, 'trees': []}
        for depth in (3, 36):
            top = (1 << depth) - 1
            indexes = [5, 4, 5, top, 4, 0, top - 1, 5] if depth == 3 else [5, 4, 5, 2**32 + 7, 4, 2**35 + 1, top, 2**32 + 6]
            probe = indexes[:4] + ([2, 3] if depth == 3 else [2**33, 2**36 - 5, 3])
            for key, family, empty in (('pairs', Family('p', h6, 2), (rng.randrange(modulus), 3)), ('singles', Family('s', h3, 1), None), ('rescued', Family('r', hr, 1), 11)):
                tree = family.sparse(depth, empty)
                new = [family.leaf(rng) for _ in indexes]
                new[4] = new[1]                       # leaf 4 already holds it
                new[7] = tree.empties[0]              # back to `empty`
                records = tree.updateMany(indexes, new)
                rec['trees'].append({'kind': key, 'depth': depth, 'empty': None if empty is None else s(empty), 'indexes': s(indexes), 'new': s(new),
                                     'before': s([r.before for r in records]), 'roots': s([r.root for r in records]), 'empties': s(tree.empties),
                                     'probe': s(probe), 'paths': s(tree.proveMany(probe)), 'stored': tree.stored})
        out.append(rec)
    with open(path, 'w') as fh:
        json.dump(out, fh)


@needs_node
def test_js_on_a_library_without_the_entries(tmp_path):
    """the sparse classes throw an Error that names what is missing"""
    run_js('sparse_tree', 'double', tmp_path, js_expectations)


@needs_node
@pytest.mark.gpu
def test_js_on_hip(tmp_path):
    run_js('sparse_tree', 'hip', tmp_path, js_expectations)


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    rng = random.Random(q % 65521)
    f = PrimeField(backend=be)
    for family in hades_families(f) + [Family('rescue', random_rescue(f, rng, 3, 2), 1)]:
        check_against_dense(family, (3,), (1, 65, 257), rng)
        check_depth_36(family, rng, on_device=True)
    print(f'runtime sparse tree: modulus {q} ok')
