"""Poseidon hashes and Poseidon Merkle trees on the device: include/gstark_hades.h, csrc/hades.hip, genstark_amd/hades.py, js/hades.js.

Every comparison is equality of field elements against host integers.  CPU tier: the header, the binding table, and the whole Python
layer on the tests' double (which lacks the entry points: the host fallback) against the existing PoseidonMerkleTree / poseidon_hash
controls.  GPU tier: the kernels at the seams of a wave and of a workgroup, every width / arity / round shape / exponent / digest, the
tree at the seam between its wide levels and its one-workgroup top, the path gather, and a device-built tree feeding the ComputeMerkleRoot
STARKs of lib128 / lib224.  `python tests/test_hades.py runtime <q>` is the check of the runtime-modulus flavour (one modulus per process)."""
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

from genstark_amd import _abi, lib128, lib224, poseidon
from genstark_amd._abi import Backend, GstarkError
from genstark_amd.field import PrimeField
from genstark_amd.hades import HadesHash, HadesMerkleTree
from sponge_common import FLAVOURS, ROOT, check_header_is_plain_c, check_symbol_table, flavour_fixture, heap_nodes, input_rows, needs_node, run_js


# ---- CPU tier: header and binding table -------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    check_header_is_plain_c('hades')


def test_symbol_table_matches_the_header():
    assert len(_abi.HADES_SYMBOLS) == 6
    check_symbol_table('hades', _abi.HADES_SYMBOLS, (_abi.EXPORTED_SYMBOLS, _abi.OPTIONAL_SYMBOLS))


def test_the_double_lacks_the_entries_and_loads(oracle_backend):
    assert not any(hasattr(oracle_backend.lib, name) for name in _abi.HADES_SYMBOLS)
    f = PrimeField(backend=oracle_backend)
    assert not HadesHash(f, 5, 8, 55, 6).onDevice


# ---- CPU tier: the Python layer on the host fallback ------------------------------------------------------------------------------
def lib_hash(lib, f):
    """HadesHash with a library's own parameters, built as poseidon_tree builds it"""
    return lib.poseidon_tree(f, [0, 0] if lib is lib224 else [(0, 0), (0, 0)]).hash


def test_hash_equals_the_controls(oracle_backend):
    f = PrimeField(backend=oracle_backend)
    p = f.modulus
    rows = [[1, 2, 3, 4], [0, 1, p - 1, 7], [p - 1, p - 2, 5, 0]]
    h128, derived = lib_hash(lib128, f), HadesHash(f, 5, 8, 55, 6)
    for row in rows:
        assert h128.hash(row) == lib128.poseidon_hash(f, row)
        assert derived.hash(row) == derived(row) == poseidon.poseidon_hash(f, row)
        assert derived.hash(row[:1]) == poseidon.poseidon_hash(f, row[:1])
    assert derived.hashMany(rows).toValues() == [poseidon.poseidon_hash(f, r) for r in rows]
    assert derived.hashMany(f.newMatrixFrom(rows), 1).toValues() == [poseidon.poseidon_hash(f, r)[:1] for r in rows]


def test_hash_equals_lib224(p224_double):
    f = PrimeField(backend=p224_double)
    h = lib_hash(lib224, f)
    for row in ([42, 43], [0, f.modulus - 1], [1]):
        assert h.hash(row) == lib224.poseidon_hash(f, row)


@pytest.fixture(scope='module')
def p224_double():
    from test_wide_fields import oracle_for
    be = oracle_for('p224')
    yield be
    be.close()


def check_tree_against_control(tree, control, n):
    assert tree.nodes == control.nodes and tree.root == control.root
    paths = tree.proveMany(list(range(n)))
    for i in range(n):
        assert tree.prove(i) == control.prove(i) == paths[i]
        assert HadesMerkleTree.verify(tree.root, i, paths[i], tree.hash)
        for k in range(len(paths[i])):               # one element of the path changed: refused
            bad = list(paths[i])
            bad[k] = bad[k] + 1 if isinstance(bad[k], int) else (bad[k][0], bad[k][1] ^ 1)
            assert not HadesMerkleTree.verify(tree.root, i, bad, tree.hash)


@pytest.mark.parametrize('n', [2, 4, 64])
def test_trees_equal_the_controls(oracle_backend, p224_double, n):
    rng = random.Random(n)
    f = PrimeField(backend=oracle_backend)
    leaves = [(rng.randrange(f.modulus), rng.randrange(f.modulus)) for _ in range(n)]
    check_tree_against_control(lib128.poseidon_tree(f, leaves), lib128.PoseidonMerkleTree(f, leaves), n)
    f = PrimeField(backend=p224_double)
    leaves = [rng.randrange(f.modulus) for _ in range(n)]
    check_tree_against_control(lib224.poseidon_tree(f, leaves), lib224.PoseidonMerkleTree(f, leaves), n)
    if n == 4:                                       # leaves already on a device: the same tree
        assert lib224.poseidon_tree(f, f.newVectorFrom(leaves)).nodes == lib224.PoseidonMerkleTree(f, leaves).nodes


def test_bad_shapes_raise(oracle_backend):
    f = PrimeField(backend=oracle_backend)
    for args in ((5, 8, 55, 1), (5, 8, 55, 9), (5, 7, 55, 3), (5, 0, 55, 3), (1, 8, 55, 3), (5, 8, -1, 3)):
        with pytest.raises(GstarkError):
            HadesHash(f, *args)
    with pytest.raises(GstarkError):
        HadesHash(f, 5, 8, 55, 3, round_constants=[[1, 2, 3]] * 62)
    with pytest.raises(GstarkError):
        HadesHash(f, 5, 8, 55, 3, mds=[[1, 2, 3]] * 2)
    h3, h6 = HadesHash(f, 5, 2, 1, 3), HadesHash(f, 5, 2, 1, 6)
    for bad in ([], [1, 2, 3]):
        with pytest.raises(GstarkError):
            h3.hash(bad)
    with pytest.raises(GstarkError):
        h3.hashMany([[1, 2, 3]])
    with pytest.raises(GstarkError):
        h3.hashMany([[1, 2]], digest=3)
    for hash, leaves, digest in ((h3, [1, 2, 3], 1), (h3, [1], 1), (h3, [(1, 2)] * 4, 2), (h6, [(1, 2)] * 4, 3), (h6, [1, 2], 2), (h3, [], 1)):
        with pytest.raises(GstarkError):
            HadesMerkleTree(hash, leaves, digest)
    tree = HadesMerkleTree(h3, [1, 2, 3, 4], 1)
    for bad in (4, -1):
        with pytest.raises(GstarkError):
            tree.prove(bad)


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 257, 1000)                   # the seams of a wave (64 lanes) and of a workgroup (256 threads)
WIDTHS = (2, 3, 6, 8)
ROUND_SHAPES = ((2, 0), (8, 1), (8, 55))
ALPHAS = (3, 5, 17)


flavour = flavour_fixture()


def check_counts(be, rng):
    """every count at every width (the LDS stage of the kernel is sized by the width), both digests; cheap rounds keep the host reference
    short, and the Poseidon shape of the reference runs at the counts around one workgroup"""
    f = PrimeField(backend=be)
    cases = [(w, w - 1, 2, 0, 3, COUNTS) for w in WIDTHS] + [(6, 4, 8, 55, 5, (65, 257)), (3, 2, 8, 55, 5, (65, 257))]
    for width, arity, rf, rp, alpha, counts in cases:
        h = HadesHash(f, alpha, rf, rp, width)
        assert h.onDevice
        rows = input_rows(rng, f.modulus, max(counts), arity)
        want = [h.hash(r) for r in rows]              # once, shared by every count and both digests
        for count in counts:
            src = f.newMatrixFrom(rows[:count])
            assert h.hashMany(src, 2).toValues() == want[:count], (width, count)
            assert h.hashMany(src, 1).toValues() == [w[:1] for w in want[:count]], (width, count)


def check_shapes(be, rng, count=9):
    """every width x arity x round shape x exponent x digest, on rows that hold 0, 1 and p - 1"""
    f = PrimeField(backend=be)
    for width in WIDTHS:
        for rf, rp in ROUND_SHAPES:
            for alpha in ALPHAS:
                h = HadesHash(f, alpha, rf, rp, width)
                for arity in range(1, width):
                    rows = input_rows(rng, f.modulus, count, arity)
                    want = [h.hash(r) for r in rows]
                    assert h.hashMany(rows, 2).toValues() == want, (width, rf, rp, alpha, arity)
                    assert h.hashMany(rows, 1).toValues() == [w[:1] for w in want], (width, rf, rp, alpha, arity)


@pytest.mark.gpu
def test_permutations_at_the_seams(flavour):
    check_counts(flavour, random.Random(0x4AD5))


@pytest.mark.gpu
def test_permutations_of_every_shape(flavour):
    check_shapes(flavour, random.Random(0x4AD6))


def host_tree(h, leaves, digest):
    return heap_nodes([list(leaf) for leaf in leaves], lambda left, right: h.hash(left + right)[:digest], [0] * digest)


def check_trees(be, rng, sizes=None):
    """digest 1 at width 3 and digest 2 at width 6; every node; the same tree twice back to back; the paths of one call"""
    f = PrimeField(backend=be)
    t = be.lib.gs_hades_merkle_top()
    assert t >= 4 and not t & (t - 1)
    sizes = sizes or (2, 4, t // 2, t, 2 * t, 4 * t, 1 << 11)      # the top alone, exactly the top, one and two wide levels below it
    for digest, width in ((1, 3), (2, 6)):
        h = HadesHash(f, 3, 2, 1, width)                          # few rounds: the host reference of 2^11 leaves stays short
        for n in sizes:
            leaves = [[rng.randrange(f.modulus) for _ in range(digest)] for _ in range(n)]
            want = host_tree(h, leaves, digest)
            src = f.newMatrixFrom(leaves)
            tree, again = HadesMerkleTree(h, src, digest), HadesMerkleTree(h, src, digest)
            raw = tree.deviceNodes.toBuffer()
            assert tree.deviceNodes.toValues() == want, (digest, n)
            assert again.deviceNodes.toBuffer() == raw, (digest, n)
            indexes = [0, n - 1, n // 2, n // 2] + [rng.randrange(n) for _ in range(100)]
            paths = tree.proveMany(indexes)
            shape = (lambda v: v[0]) if digest == 1 else tuple
            for i, path in zip(indexes, paths):
                assert path == [shape(want[n + i])] + [shape(want[((n + i) >> l) ^ 1]) for l in range(n.bit_length() - 1)], (digest, n, i)
            with pytest.raises(GstarkError, match='outside'):
                tree.proveMany([0, n])
    # the Poseidon shape of the reference across the seam: 2t leaves of two elements
    h = HadesHash(f, 5, 8, 55, 6)
    leaves = [[rng.randrange(f.modulus), rng.randrange(f.modulus)] for _ in range(min(2 * t, max(sizes)))]
    assert HadesMerkleTree(h, leaves, 2).deviceNodes.toValues() == host_tree(h, leaves, 2)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['p128', 'p224'])
def test_trees_and_paths(name):
    be = Backend(device=0, modulus=FLAVOURS[name])
    try:
        check_trees(be, random.Random(0x7EE))
    finally:
        be.close()


@pytest.mark.gpu
def test_bad_shapes_are_refused_by_the_library(hip_backend):
    f = PrimeField(backend=hip_backend)
    es, call = f.elementSize, hip_backend.call
    h = C.c_void_p()
    for width, rf, alpha in ((1, 8, 5), (9, 8, 5), (3, 7, 5), (3, 8, 1)):
        with pytest.raises(GstarkError, match='hades_create'):
            call('gs_hades_create', width, rf, 1, alpha, bytes(9 * 9 * es), bytes(9 * 9 * es), C.byref(h))
    h3 = HadesHash(f, 5, 2, 1, 3)
    buf = f.newMatrix(16, 2)
    ptr = C.c_void_p(buf.ptr)
    with pytest.raises(GstarkError, match='do not fit'):
        call('gs_hades_hash', h3.handle(), ptr, 4, 3, 1, ptr)
    with pytest.raises(GstarkError, match='digest'):
        call('gs_hades_hash', h3.handle(), ptr, 4, 2, 3, ptr)
    for n, digest in ((3, 1), (1, 1), (0, 1), (4, 2)):
        with pytest.raises(GstarkError, match='hades_merkle'):
            call('gs_hades_merkle', h3.handle(), ptr, n, digest, ptr)
    with pytest.raises(GstarkError, match='outside'):
        call('gs_hades_merkle_paths', ptr, 4, 1, (C.c_uint64 * 2)(3, 4), 2, ptr)


def merkle_statement(lib, f, tree, index, depth):
    """ComputeMerkleRoot of `lib` for the path of leaf `index`: (stark, assertions over `tree.root`, inputs, first row)"""
    from genstark_amd._mirror.stark import Stark
    from test_lib128 import OPTS
    path = tree.prove(index)
    bits = [0] + [(index >> j) & 1 for j in range(depth)][:-1]
    air = lib.compute_merkle_root_air(f, bits)
    inputs, first = lib.merkle_inputs(f, path[0], path[1:])
    last, top = 64 * depth - 1, (index >> (depth - 1)) & 1
    if lib is lib128:
        assertions = [{'step': last, 'register': 6 * top + k, 'value': tree.root[k]} for k in range(2)]
    else:
        assertions = [{'step': last, 'register': 3 * top, 'value': tree.root}]
    return Stark(air, OPTS), assertions, inputs, first


def check_end_to_end(be, lib):
    from genstark_amd.errors import StarkError
    from genstark_amd.native import NativeProver
    f = PrimeField(backend=be)
    rng = random.Random(16)
    leaves = [rng.randrange(f.modulus) for _ in range(16)] if lib is lib224 else [(rng.randrange(f.modulus), rng.randrange(f.modulus)) for _ in range(16)]
    tree, control = lib.poseidon_tree(f, leaves), lib.PoseidonMerkleTree(f, leaves)
    assert tree.deviceNodes is not None and tree.root == control.root
    proofs = []
    for t in (tree, control):
        stark, assertions, inputs, first = merkle_statement(lib, f, t, 11, 4)
        nat = NativeProver(stark)
        proofs.append(nat.prove_bytes(assertions, inputs, first))
    assert proofs[0] == proofs[1]
    assert nat.verify_bytes(assertions, proofs[0]) is True
    with pytest.raises(StarkError):
        nat.verify_bytes([dict(assertions[0], value=assertions[0]['value'] ^ 1)] + assertions[1:], proofs[0])


@pytest.mark.gpu
def test_device_tree_feeds_the_merkle_root_stark_lib128(hip_backend):
    check_end_to_end(hip_backend, lib128)


@pytest.mark.gpu
def test_device_tree_feeds_the_merkle_root_stark_lib224():
    be = Backend(device=0, modulus=_abi.MODULUS_224)
    try:
        check_end_to_end(be, lib224)
    finally:
        be.close()


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    from test_runtime_modulus import PRIMES
    q = PRIMES[12]                                    # 127 bits
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(q)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'runtime hades: modulus {q} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---- node ---------------------------------------------------------------------------------------------------------------------------
def js_expectations(path):
    """what tests/js_hades.js must find, from host integers: per field a width-6 hash and tree of pairs, a width-3 tree of single elements"""
    from genstark_amd.hostfield import HostField
    rng = random.Random(0x15)
    out = []
    for modulus in (_abi.MODULUS_128, _abi.MODULUS_64):
        f = HostField(modulus)
        h6, h3 = HadesHash(f, 5, 8, 55, 6), HadesHash(f, 3, 8, 5, 3)
        rows = [[0, 1, modulus - 1, 5]] + [[rng.randrange(modulus) for _ in range(4)] for _ in range(69)]
        pairs = [[rng.randrange(modulus), rng.randrange(modulus)] for _ in range(8)]
        singles = [rng.randrange(modulus) for _ in range(16)]
        out.append({'modulus': str(modulus), 'rows': [[str(v) for v in r] for r in rows], 'digests': [[str(v) for v in h6.hash(r)] for r in rows],
                    'pairs': [[str(v) for v in r] for r in pairs], 'pairNodes': [[str(v) for v in r] for r in host_tree(h6, pairs, 2)[1:]],
                    'singles': [str(v) for v in singles], 'singleNodes': [str(r[0]) for r in host_tree(h3, [[v] for v in singles], 1)[1:]]})
    with open(path, 'w') as fh:
        json.dump(out, fh)


@needs_node
def test_js_on_a_library_without_the_entries(tmp_path):
    """createHash's function is host arithmetic and equals the Python host; the device members throw an Error that names what is missing"""
    run_js('hades', 'double', tmp_path, js_expectations)


@needs_node
@pytest.mark.gpu
def test_js_on_hip(tmp_path):
    run_js('hades', 'hip', tmp_path, js_expectations)


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    rng = random.Random(q % 65521)
    f = PrimeField(backend=be)
    h = HadesHash(f, 5, 8, 55, 3)
    for arity in (1, 2):
        rows = input_rows(rng, q, 300, arity)
        assert h.hashMany(rows, 2).toValues() == [h.hash(r) for r in rows]
    check_trees(be, rng, sizes=(64,))
    print(f'runtime hades: modulus {q} ok')
