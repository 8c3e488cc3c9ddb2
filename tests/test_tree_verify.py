"""Batches of Merkle paths and update records checked in bulk: include/gstark_tree_verify.h, csrc/tree_verify.h, the path-walk kernels
of csrc/hades.hip and csrc/rescue.hip, FieldMerkleTree.pathRoots / verifyMany / verifyUpdates (genstark_amd/field_tree.py) and the same
members of js/field_tree.js.

Every comparison is equality of field elements.  CPU tier: the header and the binding table, and the members on libraries without the
entries (host integers) — every path of proveMany, the records of updateMany, every kind of tampering, the refusals.  GPU tier: the two
kernels at the seams of a lane group's wave, of a wave and of a workgroup against the root of the device tree (which the suites of the
tree builds hold to host integers) and, for a few paths, against verify_path on host integers; the tamperings; the `leaves` argument on
update records; the public root of a ComputeMerkleRoot statement taken from pathRoots; the library's refusals; the node binding.
`python tests/test_tree_verify.py runtime <q>` is the check of the runtime-modulus flavour (one modulus per process)."""
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
from sponge_common import ROOT, check_header_is_plain_c, check_symbol_table, flavour_fixture, needs_node, run_js


# ---- CPU tier: header and binding table -------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    check_header_is_plain_c('tree_verify')


def test_symbol_table_matches_the_header():
    assert _abi.TREE_VERIFY_SYMBOLS == ('gs_hades_merkle_path_roots', 'gs_rescue_merkle_path_roots')
    check_symbol_table('tree_verify', _abi.TREE_VERIFY_SYMBOLS,
                       (_abi.EXPORTED_SYMBOLS, _abi.OPTIONAL_SYMBOLS, _abi.HADES_SYMBOLS, _abi.RESCUE_SYMBOLS, _abi.TREE_UPDATE_SYMBOLS))
    header = open(os.path.join(ROOT, 'include', 'gstark_tree_verify.h')).read()
    assert '2^20' in header and '1 .. 36' in header                       # the caps are part of the contract


def test_the_double_lacks_the_entries(oracle_backend):
    assert not any(hasattr(oracle_backend.lib, name) for name in _abi.TREE_VERIFY_SYMBOLS)


# ---- what both tiers share ----------------------------------------------------------------------------------------------------------
def bump(node, p, element=0):
    """a node with one element changed"""
    if isinstance(node, int):
        return (node + 1) % p
    return tuple((v + 1) % p if e == element else v for e, v in enumerate(node))


def tamperings(paths, indexes, depth, digest, p, places):
    """The corruptions of the issue's list, one per path at the positions `places` yields: {name: (place, index, path)} — a sibling
    changed at each level, only the second element of a sibling, an index bit flipped at each level, the leaf changed."""
    out = {}

    def put(name, index_of, path_of):
        k = next(places)
        out[name] = (k, index_of(indexes[k]), path_of(list(paths[k])))
    for l in range(1, depth + 1):
        put(f'sibling {l}', lambda i: i, lambda path, l=l: path[:l] + [bump(path[l], p)] + path[l + 1:])
        put(f'bit {l - 1}', lambda i, l=l: i ^ (1 << (l - 1)), lambda path: path)
    if digest == 2:
        put('second element', lambda i: i, lambda path: path[:depth] + [bump(path[depth], p, 1)])
    put('leaf', lambda i: i, lambda path: [bump(path[0], p)] + path[1:])
    return out


def check_negatives_one_by_one(cls, hash, root, indexes, paths, depth, digest, p):
    """every tampering alone in the batch: exactly the tampered path is False"""
    places = iter(range(10 ** 6))
    cases = tamperings(paths, indexes, depth, digest, p, (k % len(paths) for k in places))
    for name, (k, index, path) in cases.items():
        got = cls.verifyMany(root, indexes[:k] + [index] + indexes[k + 1:], paths[:k] + [path] + paths[k + 1:], hash)
        assert got == [j != k for j in range(len(paths))], name
    if digest == 2:
        assert cls.verifyMany((root[0], (root[1] + 1) % p), indexes, paths, hash) == [False] * len(paths)
        assert cls.verifyMany(((root[0] + 1) % p, root[1]), indexes, paths, hash) == [False] * len(paths)
    else:
        assert cls.verifyMany((root + 1) % p, indexes, paths, hash) == [False] * len(paths)


def check_update_records(cls, hash, old_root, indexes, new, records, p):
    """verifyUpdates: all valid; a tampered root fails its record and the next; a tampered sibling fails only its record"""
    count = len(records)
    assert cls.verifyUpdates(old_root, indexes, new, records, hash) == [True] * count
    assert cls.pathRoots(hash, indexes, [r.before for r in records], leaves=new) == [r.root for r in records]
    assert cls.pathRoots(hash, indexes, [r.before for r in records]) == [old_root] + [r.root for r in records[:-1]]
    for j in sorted({0, count // 2, count - 1}):
        bad = records[:j] + [TreeUpdate(records[j].before, bump(records[j].root, p, len(records[j].before[0]) - 1 if isinstance(records[j].root, tuple) else 0))] + records[j + 1:]
        assert cls.verifyUpdates(old_root, indexes, new, bad, hash) == [k not in (j, j + 1) for k in range(count)], j
        level = 1 + j % (len(records[j].before) - 1)
        before = records[j].before[:level] + [bump(records[j].before[level], p)] + records[j].before[level + 1:]
        bad = records[:j] + [TreeUpdate(before, records[j].root)] + records[j + 1:]
        assert cls.verifyUpdates(old_root, indexes, new, bad, hash) == [k != j for k in range(count)], j
    wrong = list(new)
    wrong[count - 1] = bump(wrong[count - 1], p)                          # another new leaf than the one the record was made with
    assert cls.verifyUpdates(old_root, indexes, wrong, records, hash) == [True] * (count - 1) + [False]


def distinct(rng, p, count, digest):
    seen = set()
    while len(seen) < count * digest:
        seen.add(rng.randrange(p))
    values = list(seen)
    rng.shuffle(values)
    return values[:count] if digest == 1 else [tuple(values[2 * k:2 * k + 2]) for k in range(count)]


def remembering(fn, key=lambda *a: a):
    seen = {}

    def call(*args):
        k = key(*args)
        if k not in seen:
            seen[k] = fn(*args)
        return seen[k]
    return call


# ---- CPU tier: the members on libraries without the entries -----------------------------------------------------------------------
@pytest.fixture(scope='module')
def p224_double():
    from test_wide_fields import oracle_for
    be = oracle_for('p224')
    yield be
    be.close()


def check_on_the_host(cls, tree, leaves, digest, rng):
    hash, n, depth, p = tree.hash, tree.leafCount, tree.depth, tree.field.modulus
    assert tree.deviceNodes is None and not hash.onDevice
    root, indexes = tree.root, list(range(n))
    paths = tree.proveMany(indexes)
    assert cls.pathRoots(hash, indexes, paths) == [root] * n
    assert cls.verifyMany(root, indexes, paths, hash) == [True] * n
    assert cls.pathRoots(hash, [], []) == [] and cls.verifyMany(root, [], [], hash) == [] and cls.verifyUpdates(root, [], [], [], hash) == []
    # values are taken mod p; the leaves argument replaces the path's own leaf
    lifted = [[v + p if isinstance(v, int) else (v[0] + p, v[1]) for v in path] for path in paths[:2]]
    assert cls.pathRoots(hash, indexes[:2], lifted) == [root] * 2
    assert cls.pathRoots(hash, indexes[:2], [[bump(path[0], p)] + path[1:] for path in paths[:2]], leaves=leaves[:2]) == [root] * 2
    sample = sorted({0, n - 1, n // 3})
    check_negatives_one_by_one(cls, hash, root, [indexes[i] for i in sample], [paths[i] for i in sample], depth, digest, p)
    # the records of a batch with repeated indexes verify in order
    i = rng.randrange(n)
    batch = [i, i ^ 1, i, rng.randrange(n), i ^ 1]
    new = distinct(rng, p, len(batch), digest)
    records = tree.updateMany(batch, new)
    check_update_records(cls, hash, root, batch, new, records, p)


@pytest.mark.parametrize('n', [2, 4, 64])
def test_host_members_on_the_poseidon_trees(oracle_backend, p224_double, n):
    rng = random.Random(0x7E1 + n)
    f = PrimeField(backend=oracle_backend)
    leaves = distinct(rng, f.modulus, n, 2)
    tree = lib128.poseidon_tree(f, leaves)
    tree.hash.hash = remembering(tree.hash.hash, key=tuple)             # the tamperings walk mostly the same nodes again
    check_on_the_host(HadesMerkleTree, tree, leaves, 2, rng)
    f224 = PrimeField(backend=p224_double)
    leaves = distinct(rng, f224.modulus, n, 1)
    tree = lib224.poseidon_tree(f224, leaves)
    tree.hash.hash = remembering(tree.hash.hash, key=tuple)
    check_on_the_host(HadesMerkleTree, tree, leaves, 1, rng)


@pytest.mark.parametrize('n', [2, 4, 64])
def test_host_members_on_the_rescue_tree(oracle_backend, n):
    rng = random.Random(0x7E2 + n)
    f = PrimeField(backend=oracle_backend)
    h = rescue4x128(f)
    h.hash2 = remembering(h.hash2)
    leaves = distinct(rng, f.modulus, n, 1)
    check_on_the_host(RescueMerkleTree, RescueMerkleTree(h, leaves), leaves, 1, rng)


def test_host_members_take_device_arrays_of_a_library_without_the_entries(oracle_backend):
    """a Matrix of paths and an array of leaves on the double are read and walked on host integers"""
    f = PrimeField(backend=oracle_backend)
    rng = random.Random(3)
    h3, h6 = HadesHash(f, 3, 2, 1, 3), HadesHash(f, 3, 2, 1, 6)
    for h, digest in ((h3, 1), (h6, 2)):
        leaves = distinct(rng, f.modulus, 8, digest)
        tree = HadesMerkleTree(h, leaves, digest)
        paths = tree.proveMany(range(8))
        flat = f.newMatrixFrom([[v for node in path for v in ((node,) if digest == 1 else node)] for path in paths])
        assert HadesMerkleTree.pathRoots(h, range(8), flat, digest=digest) == [tree.root] * 8
        new = distinct(rng, f.modulus, 8, digest)
        want = HadesMerkleTree.pathRoots(h, range(8), paths, leaves=new)
        assert want != [tree.root] * 8
        assert HadesMerkleTree.pathRoots(h, range(8), flat, leaves=f.newMatrixFrom([[v] if digest == 1 else list(v) for v in new]), digest=digest) == want
        with pytest.raises(GstarkError, match='^HadesMerkleTree: paths on the device do not tell'):
            HadesMerkleTree.pathRoots(h, range(8), flat)


def test_refusals(oracle_backend):
    f = PrimeField(backend=oracle_backend)
    h3, h6 = HadesHash(f, 3, 2, 1, 3), HadesHash(f, 3, 2, 1, 6)
    r3 = RescueHash(f, 3, -3, 3, 2, [[1, 2, 3], [4, 5, 7], [9, 8, 11]], list(range(1, 16)))
    single, pairs, rescue = HadesMerkleTree(h3, [1, 2, 3, 4], 1), HadesMerkleTree(h6, [(1, 2), (3, 4), (5, 6), (7, 8)], 2), RescueMerkleTree(r3, [1, 2, 3, 4])
    for tree in (single, pairs, rescue):
        cls, h, who = type(tree), tree.hash, tree._who
        paths, root = tree.proveMany([0, 3]), tree.root
        with pytest.raises(GstarkError, match=f'^{who}: the paths have unequal lengths'):
            cls.pathRoots(h, [0, 3], [paths[0], paths[1][:-1]])
        for indexes in ([0], [0, 3, 1], []):
            with pytest.raises(GstarkError, match=f'^{who}: {len(indexes)} indexes and 2 paths'):
                cls.verifyMany(root, indexes, paths, h)
        for bad in (4, -1, 1 << 40):
            with pytest.raises(GstarkError, match=f'^{who}: index {bad} is outside of the 4 leaves'):
                cls.pathRoots(h, [0, bad], paths)
        for empty in ([paths[0][:1], paths[1][:1]], [[], []]):
            with pytest.raises(GstarkError, match=f'^{who}: a path is a leaf and at least one sibling'):
                cls.pathRoots(h, [0, 3], empty)
        with pytest.raises(GstarkError, match=f'^{who}: 2 paths and 1 leaves'):
            cls.pathRoots(h, [0, 3], paths, leaves=[paths[0][0]])
        records = tree.updateMany([1, 1], [paths[0][0], paths[1][0]])
        with pytest.raises(GstarkError, match=f'^{who}: 2 paths and 1 leaves'):
            cls.verifyUpdates(root, [1, 1], [paths[0][0]], records, h)
        with pytest.raises(GstarkError, match=f'^{who}: 1 indexes and 2 paths'):
            cls.verifyUpdates(root, [1], [paths[0][0], paths[1][0]], records, h)
    with pytest.raises(GstarkError, match='^HadesMerkleTree: every node of a path has 1 element'):
        HadesMerkleTree.pathRoots(h3, [0], [[1, (2, 3)]])
    with pytest.raises(GstarkError, match='^HadesMerkleTree: nodes of 2 elements'):
        HadesMerkleTree.pathRoots(h3, [0], [[(1, 2), (2, 3)]])           # a digest that does not fit the width
    r2 = RescueHash(f, 3, -3, 2, 2, [[1, 2], [3, 5]], list(range(1, 9)))
    with pytest.raises(GstarkError, match='^RescueMerkleTree: two nodes do not fit a state of 2'):
        RescueMerkleTree.pathRoots(r2, [0], [[1, 2]])
    with pytest.raises(GstarkError, match='^RescueMerkleTree: two nodes do not fit a state of 2'):
        RescueMerkleTree.verifyMany(1, [0], [[1, 2]], r2)


def test_a_device_hash_without_the_entry_says_so(oracle_backend):
    """a library with gs_<family>_hash but without the new entry: the members raise and name it; they do not hash on the host"""
    import types
    f = PrimeField(backend=oracle_backend)
    for cls, h, entry in ((HadesMerkleTree, HadesHash(f, 3, 2, 1, 3), 'gs_hades_merkle_path_roots'),
                          (RescueMerkleTree, RescueHash(f, 3, -3, 3, 2, [[1, 2, 3], [4, 5, 7], [9, 8, 11]], list(range(1, 16))), 'gs_rescue_merkle_path_roots')):
        lib = types.SimpleNamespace(**{f'gs_{h._family}_hash': None})
        h.field = types.SimpleNamespace(modulus=f.modulus, backend=types.SimpleNamespace(lib=lib, ctx=None))
        assert h.onDevice
        with pytest.raises(GstarkError, match=f'^{cls._who}: the library has no {entry} \\(include/gstark_tree_verify.h\\)'):
            cls.pathRoots(h, [0], [[1, 2]])
        with pytest.raises(GstarkError, match=entry):
            cls.verifyUpdates(1, [0], [3], [TreeUpdate([1, 2], 5)], h)


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 15, 16, 17, 63, 64, 65, 257, 1000)       # the seams of a lane group's wave (64 / G paths), of a wave, of a 256-thread workgroup
SIZES = (2, 4, 1 << 11)
HADES = ((3, 1), (5, 2), (6, 2), (8, 1), (8, 2))      # (width, digest)
RESCUE = (3, 4, 5, 8)                                 # widths: G = 4, 4, 8, 8

flavour = flavour_fixture()


def index_patterns(n, count, rng):
    """0, n - 1, 0b0101.., 0b1010.., random ones, and repeats of all of them"""
    special = [0, n - 1, 0x5555555555 % n, 0xAAAAAAAAAA % n]
    fresh = special + [rng.randrange(n) for _ in range(count // 2)]
    return (fresh + [rng.choice(fresh) for _ in range(count)])[:count]


def device_paths(tree, indexes):
    """the path gather's output as it lies on the device: one row per path"""
    be, count = tree.field.backend, len(indexes)
    out = Matrix(be, count, (tree.depth + 1) * tree.digest)
    be.call('gs_hades_merkle_paths', C.c_void_p(tree.deviceNodes.ptr), tree.leafCount, tree.digest, (C.c_uint64 * count)(*indexes), count, C.c_void_p(out.ptr))
    return out


def as_lists(flat_rows, digest):
    return [[row[l] if digest == 1 else tuple(row[2 * l:2 * l + 2]) for l in range(len(row) // digest)] for row in flat_rows]


def check_parity(cls, f, hash, make_tree, digest, rng, sizes, counts, host_node=None, host_paths=0):
    be, p = f.backend, f.modulus
    for n in sizes:
        leaves = [[rng.randrange(p) for _ in range(digest)] for _ in range(n)]
        tree = make_tree(leaves)
        root, indexes = tree.root, index_patterns(n, max(counts), rng)
        gathered = device_paths(tree, indexes)
        lists = as_lists(gathered.toValues(), digest)
        for k in counts:
            where = (hash.width, digest, n, k)
            head = Matrix(be, k, gathered.colCount, owner=gathered._owner)                    # the first k rows, where they lie
            assert cls.pathRoots(hash, indexes[:k], head, digest=digest) == [root] * k, where
            assert cls.pathRoots(hash, indexes[:k], lists[:k]) == [root] * k, where
            assert cls.verifyMany(root, indexes[:k], lists[:k], hash) == [True] * k, where
        if host_node and n == sizes[-1]:
            for i, path in list(zip(indexes, lists))[:host_paths]:                           # an independent model: host integers
                assert verify_path(root, i, path, host_node), (hash.width, digest, n, i)


def random_rescue(f, rng, width, rounds):
    p = f.modulus
    return RescueHash(f, 3, -3, width, rounds, [[rng.randrange(p) for _ in range(width)] for _ in range(width)], [rng.randrange(p) for _ in range(width * (width + 2))])


def check_hades(be, rng, configs=HADES, sizes=SIZES, counts=COUNTS, host_paths=4):
    f = PrimeField(backend=be)
    assert hasattr(be.lib, 'gs_hades_merkle_path_roots')
    for width, digest in configs:
        h = HadesHash(f, 3, 2, 1, width)
        node = (lambda a, b: h.hash([a, b])[0]) if digest == 1 else (lambda a, b: tuple(h.hash(list(a) + list(b))[:2]))
        check_parity(HadesMerkleTree, f, h, lambda leaves: HadesMerkleTree(h, f.newMatrixFrom(leaves), digest), digest, rng, sizes, counts, node,
                     host_paths if width in (3, 6) else 0)


def check_rescue(be, rng, widths=RESCUE, sizes=SIZES, counts=COUNTS, host_paths=4):
    f = PrimeField(backend=be)
    assert hasattr(be.lib, 'gs_rescue_merkle_path_roots')
    for width in widths:
        h = random_rescue(f, rng, width, 2)
        check_parity(RescueMerkleTree, f, h, lambda leaves: RescueMerkleTree(h, f.newVectorFrom([v[0] for v in leaves])), 1, rng, sizes, counts, h.hash2,
                     host_paths if width in (4, 5) else 0)


@pytest.mark.gpu
def test_hades_path_roots_at_the_seams(flavour):
    check_hades(flavour, random.Random(0x9A7))


@pytest.mark.gpu
def test_rescue_path_roots_at_the_seams(flavour):
    check_rescue(flavour, random.Random(0x9A8))


@pytest.mark.gpu
def test_reference_parameter_sets_against_host_integers(hip_backend):
    """the full-round parameter sets (lib128's Poseidon, Rescue 4x128): a few paths against verify_path on host integers"""
    f = PrimeField(backend=hip_backend)
    rng = random.Random(0x9A9)
    leaves = distinct(rng, f.modulus, 16, 2)
    tree = lib128.poseidon_tree(f, leaves)
    paths = tree.proveMany([0, 9, 15])
    assert HadesMerkleTree.pathRoots(tree.hash, [0, 9, 15], paths) == [tree.root] * 3
    assert all(HadesMerkleTree.verify(tree.root, i, path, tree.hash) for i, path in zip([0, 9, 15], paths))
    h = rescue4x128(f)
    rtree = RescueMerkleTree(h, distinct(rng, f.modulus, 8, 1))
    paths = rtree.proveMany([2, 7])
    assert RescueMerkleTree.pathRoots(h, [2, 7], paths) == [rtree.root] * 2
    assert all(RescueMerkleTree.verify(rtree.root, i, path, h.hash2) for i, path in zip([2, 7], paths))


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    from test_runtime_modulus import PRIMES
    q = PRIMES[12]                                    # 127 bits
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(q)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'runtime tree verify: modulus {q} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


def device_cases(f, rng):
    """(class, hash, tree builder over distinct leaves, digest) of the negatives and of the update records: nodes of two elements, the Rescue tree"""
    h6, r4 = HadesHash(f, 3, 2, 1, 6), random_rescue(f, rng, 4, 2)
    return ((HadesMerkleTree, h6, lambda leaves: HadesMerkleTree(h6, leaves, 2), 2), (RescueMerkleTree, r4, lambda leaves: RescueMerkleTree(r4, leaves), 1))


@pytest.mark.gpu
def test_tampered_paths_on_the_device(hip_backend):
    """depth 11, 257 paths, every tampering of the list in ONE batch: exactly the tampered paths are False"""
    f = PrimeField(backend=hip_backend)
    rng, p, n, count = random.Random(0x9AA), f.modulus, 1 << 11, 257
    for cls, h, build, digest in device_cases(f, rng):
        tree = build(distinct(rng, p, n, digest))
        indexes = index_patterns(n, count, rng)
        paths, root = tree.proveMany(indexes), tree.root
        places = list(range(count))
        rng.shuffle(places)
        cases = tamperings(paths, indexes, tree.depth, digest, p, iter(places))
        assert len(cases) == 2 * tree.depth + digest
        for _, (k, index, path) in cases.items():
            indexes[k], paths[k] = index, path
        tampered = {k for k, _, _ in cases.values()}
        assert cls.verifyMany(root, indexes, paths, h) == [k not in tampered for k in range(count)]
        flat = f.newMatrixFrom([[v for node in path for v in ((node,) if digest == 1 else node)] for path in paths])
        assert cls.verifyMany(root, indexes, flat, h) == [k not in tampered for k in range(count)]
        got = cls.pathRoots(h, indexes, flat, digest=digest)
        assert [r == root for r in got] == [k not in tampered for k in range(count)]
        if digest == 2:                               # only the second element of the root changed: no path implies it
            assert cls.verifyMany((root[0], (root[1] + 1) % p), indexes, paths, h) == [False] * count


@pytest.mark.gpu
def test_update_records_on_the_device(hip_backend):
    """1000 updates with repeats on 2^11 leaves: the `leaves` argument gives the recorded roots; verifyUpdates and its two tamperings"""
    f = PrimeField(backend=hip_backend)
    rng, p, n, count = random.Random(0x9AB), f.modulus, 1 << 11, 1000
    for cls, h, build, digest in device_cases(f, rng):
        tree = build(distinct(rng, p, n, digest))
        old_root = tree.root
        indexes = index_patterns(n, count, rng)
        new = distinct(rng, p, count, digest)
        records = tree.updateMany(indexes, new)
        assert records[-1].root == tree.root and len(set(indexes)) < count
        check_update_records(cls, h, old_root, indexes, new, records, p)
        on_device = f.newVectorFrom(new) if digest == 1 else f.newMatrixFrom([list(v) for v in new])     # leaves already on the device
        assert cls.verifyUpdates(old_root, indexes, on_device, records, h) == [True] * count


def check_reference_shape(be, lib):
    """ComputeMerkleRoot at depth 8 with the public root taken from pathRoots"""
    from genstark_amd._mirror.stark import Stark
    from genstark_amd.errors import StarkError
    from test_lib128 import OPTS
    f = PrimeField(backend=be)
    rng, depth, index = random.Random(0x9AC), 8, 42
    leaves = distinct(rng, f.modulus, 1 << depth, 2 if lib is lib128 else 1)
    tree = lib.poseidon_tree(f, leaves)
    assert tree.deviceNodes is not None
    path = tree.prove(index)
    root, = HadesMerkleTree.pathRoots(tree.hash, [index], [path])
    assert root == tree.root == lib.PoseidonMerkleTree(f, leaves).root
    bits = [0] + [(index >> j) & 1 for j in range(depth)][:-1]
    air = lib.compute_merkle_root_air(f, bits)
    inputs, first = lib.merkle_inputs(f, path[0], path[1:])
    last = 64 * depth - 1
    assertions = [{'step': last, 'register': e, 'value': v} for e, v in enumerate(root if lib is lib128 else (root,))]
    stark = Stark(air, OPTS)
    data = stark.serialize(stark.prove(assertions, inputs, first))
    assert stark.verify(assertions, stark.parse(data))
    with pytest.raises(StarkError):
        stark.verify([dict(assertions[0], value=assertions[0]['value'] ^ 1)] + assertions[1:], stark.parse(data))


@pytest.mark.gpu
def test_path_roots_feed_the_merkle_root_stark_lib128(hip_backend):
    check_reference_shape(hip_backend, lib128)


@pytest.mark.gpu
def test_path_roots_feed_the_merkle_root_stark_lib224():
    be = Backend(device=0, modulus=_abi.MODULUS_224)
    try:
        check_reference_shape(be, lib224)
    finally:
        be.close()


@pytest.mark.gpu
def test_bad_arguments_are_refused_by_the_library(hip_backend):
    f = PrimeField(backend=hip_backend)
    call = hip_backend.call
    rng = random.Random(2)
    h3, r3 = HadesHash(f, 3, 2, 1, 3), random_rescue(f, rng, 3, 2)
    tree = HadesMerkleTree(h3, [1, 2, 3, 4], 1)
    buf, out = device_paths(tree, [0, 3]), f.newMatrix(64, 2)
    paths, ptr, two = C.c_void_p(buf.ptr), C.c_void_p(out.ptr), (C.c_uint64 * 2)(3, 4)
    families = (('hades_merkle_path_roots', h3, (1,)), ('rescue_merkle_path_roots', r3, ()))
    other = Backend(device=0)
    try:
        fo = PrimeField(backend=other)
        for (entry, _, digest), foreign in zip(families, (HadesHash(fo, 3, 2, 1, 3), random_rescue(fo, rng, 3, 2))):
            with pytest.raises(GstarkError, match=f'{entry}: the handle belongs to another context'):
                call('gs_' + entry, foreign.handle(), paths, 2, *digest, two, None, 1, ptr)
    finally:
        other.close()
    for entry, h, digest in families:
        for depth in (0, 37, 1 << 31):
            with pytest.raises(GstarkError, match=f'{entry}: a depth of {depth} levels is outside 1 .. 36'):
                call('gs_' + entry, h.handle(), paths, depth, *digest, two, None, 1, ptr)
        with pytest.raises(GstarkError, match=f'{entry}: index 4 is outside of the 4 leaves'):
            call('gs_' + entry, h.handle(), paths, 2, *digest, two, None, 2, ptr)
        with pytest.raises(GstarkError, match=f'{entry}: at most 2\\^20 paths'):
            call('gs_' + entry, h.handle(), paths, 2, *digest, two, None, (1 << 20) + 1, ptr)
        for nulls in ((None, two, ptr), (paths, None, ptr), (paths, two, None)):
            with pytest.raises(GstarkError, match=f'{entry}: the paths, their indexes and the array of the roots are required'):
                call('gs_' + entry, h.handle(), nulls[0], 2, *digest, nulls[1], None, 1, nulls[2])
        call('gs_' + entry, h.handle(), None, 2, *digest, None, None, 0, None)               # an empty batch is no error
    for digest in (0, 2, 3):
        with pytest.raises(GstarkError, match='hades_merkle_path_roots: nodes of'):
            call('gs_hades_merkle_path_roots', h3.handle(), paths, 2, digest, two, None, 1, ptr)
    be64 = Backend(device=0, modulus=_abi.MODULUS_64)
    try:
        f64 = PrimeField(backend=be64)
        h2, spare = rescue2x64(f64), f64.newVector(64)
        with pytest.raises(GstarkError, match='rescue_merkle_path_roots: two nodes do not fit a state of 2'):
            be64.call('gs_rescue_merkle_path_roots', h2.handle(), C.c_void_p(spare.ptr), 2, two, None, 1, C.c_void_p(spare.ptr))
    finally:
        be64.close()
    # afterwards the context still works
    assert HadesMerkleTree.pathRoots(h3, [0, 3], buf, digest=1) == [tree.root] * 2


# ---- node ---------------------------------------------------------------------------------------------------------------------------
def js_expectations(path):
    """what tests/js_tree_verify.js must find, from host integers: per field a tree of pairs (width 6), a tree of single elements
    (width 3) and a Rescue tree (width 4, 3 rounds) of 16 leaves each with some paths, one batch of updates, and the replacing leaves"""
    from test_rescue_hash import random_hash
    rng = random.Random(0x76)
    s = lambda v: [s(x) for x in v] if isinstance(v, (list, tuple)) else str(v)
    out = []
    for modulus in (_abi.MODULUS_128, _abi.MODULUS_64):
        f = HostField(modulus)
        h6, h3, hr = HadesHash(f, 5, 8, 55, 6), HadesHash(f, 3, 8, 5, 3), random_hash(f, rng, 4, 3)
        indexes, updates = [0, 15, 5, 10, 5], [5, 4, 5, 11]
        rec = {'modulus': str(modulus), 'indexes': indexes, 'updates': updates,
               'rescue': {'alpha': '3', 'invAlpha': str(hr.invAlpha), 'rounds': 3, 'mds': s(hr.mds), 'constants': s(hr.iConstants + [v for row in hr.cMatrix for v in row] + hr.cConstants)}}
        for key, digest, tree in (('pairs', 2, lambda v: HadesMerkleTree(h6, v, 2)), ('singles', 1, lambda v: HadesMerkleTree(h3, v, 1)), ('rescued', 1, lambda v: RescueMerkleTree(hr, v))):
            leaves = distinct(rng, modulus, 16, digest)
            t = tree(leaves)
            cls, root, paths = type(t), t.root, t.proveMany(indexes)
            new = distinct(rng, modulus, len(updates), digest)
            records = t.updateMany(updates, new)
            swapped = cls.pathRoots(t.hash, indexes, paths, leaves=[leaves[(i + 1) % 16] for i in indexes])
            rec[key] = {'leaves': s(leaves), 'root': s(root), 'paths': s(paths), 'other': s([leaves[(i + 1) % 16] for i in indexes]), 'swapped': s(swapped),
                        'new': s(new), 'before': s([r.before for r in records]), 'roots': s([r.root for r in records])}
        out.append(rec)
    with open(path, 'w') as fh:
        json.dump(out, fh)


@needs_node
def test_js_on_a_library_without_the_entries(tmp_path):
    """pathRoots, verifyMany and verifyUpdates throw an Error that names the entry and the header"""
    run_js('tree_verify', 'double', tmp_path, js_expectations)


@needs_node
@pytest.mark.gpu
def test_js_on_hip(tmp_path):
    run_js('tree_verify', 'hip', tmp_path, js_expectations)


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    rng = random.Random(q % 65521)
    check_hades(be, rng, configs=((3, 1), (8, 2)), sizes=(2, 1 << 11), counts=(1, 65, 257), host_paths=4)
    check_rescue(be, rng, widths=(3, 8), sizes=(2, 1 << 11), counts=(1, 17, 257), host_paths=4)
    print(f'runtime tree verify: modulus {q} ok')
