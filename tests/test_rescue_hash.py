"""Rescue hashes and Rescue Merkle trees on the device: include/gstark_rescue.h, csrc/rescue.hip, genstark_amd/rescue_hash.py, js/rescue.js.

Every comparison is equality of field elements against host integers.  CPU tier: the header, the binding table, the reference's known
answers, agreement with the existing key schedule and hash AIR, the tree on the tests' double (which lacks the entry points: the host
fallback) and the Merkle path statement under the mirror Stark.  GPU tier: both kernel forms at the seams of a lane group, a wave and the
spread limit, every width / sponge / digest, every branch of the exponent schedule, trees level by level, the path gather, and a
device-built tree feeding the native prover.  `python tests/test_rescue_hash.py runtime <q>` is the check of the runtime-modulus flavour
(one modulus per process).  Long host references are avoided with rounds = 2: one double round in the modified form, two in the other."""
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

from genstark_amd import _abi, rescue
from genstark_amd._abi import Backend, GstarkError
from genstark_amd.field import PrimeField
from genstark_amd.hostfield import HostField
from genstark_amd.rescue_hash import (RescueHash, RescueMerkleTree, rescue2x64, rescue4x128, rescue_merkle_inputs,
                                      rescue_merkle_proof_air)
from sponge_common import FLAVOURS, ROOT, check_header_is_plain_c, check_symbol_table, flavour_fixture, heap_nodes, input_rows, needs_node, run_js

OPTS = {'hashAlgorithm': 'blake2s256', 'extensionFactor': 16, 'exeQueryCount': 60, 'friQueryCount': 24}        # merkleProof.ts:43-49


def random_hash(f, rng, width, rounds, alpha=3, inv=None):
    """a parameter set of random constants; the inverse exponent need not invert alpha for values to be compared: any full-size one"""
    p = f.modulus
    inv = rng.randrange(1 << (p.bit_length() - 1), p - 1) if inv is None else inv
    return RescueHash(f, alpha, inv, width, rounds, [[rng.randrange(p) for _ in range(width)] for _ in range(width)],
                      [rng.randrange(p) for _ in range(width * (width + 2))])


# ---- CPU tier: header and binding table -------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    check_header_is_plain_c('rescue')


def test_symbol_table_matches_the_header():
    assert len(_abi.RESCUE_SYMBOLS) == 5 and len(_abi.HADES_SYMBOLS) == 6
    check_symbol_table('rescue', _abi.RESCUE_SYMBOLS, (_abi.EXPORTED_SYMBOLS, _abi.OPTIONAL_SYMBOLS, _abi.HADES_SYMBOLS))


def test_the_double_lacks_the_entries_and_loads(oracle_backend):
    assert not any(hasattr(oracle_backend.lib, name) for name in _abi.RESCUE_SYMBOLS)
    assert not rescue4x128(PrimeField(backend=oracle_backend)).onDevice


# ---- CPU tier: host integers ------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_reference():
    trace = rescue4x128(HostField(_abi.MODULUS_128)).sponge([42, 43])[1]
    assert trace[64][:2] == [302524937772545017647250309501879538110, 205025454306577433144586673939030012640]      # hash4x128.ts:116-117
    assert rescue2x64(HostField(_abi.MODULUS_64)).sponge([42])[1][64][0] == 14354339131598895532                      # hash2x64.ts:106


def test_constants_equal_the_existing_schedules():
    f = HostField(_abi.MODULUS_128)
    h = rescue4x128(f)
    assert len(h.unrollConstants()) == 67
    assert h.groupConstants(h.unrollConstants()) == rescue.key_schedule(f)
    f = HostField(_abi.MODULUS_64)
    assert rescue2x64(f).groupConstants() == rescue.key_schedule_2x64(f)


def test_hash2_equals_the_hash_air(oracle_backend):
    f = PrimeField(backend=oracle_backend)
    h, air = rescue4x128(f), rescue.rescue4x128_air(32, field=f)
    rng = random.Random(2)
    for a, b in ((42, 43), (0, 0), (f.modulus - 1, 1), (rng.randrange(f.modulus), rng.randrange(f.modulus))):
        row = [a, b, 0, 0]
        for step in range(31):
            row = air.transitionProgram.run(row, None, [col[step] for col in air.staticRegisters])
        assert h.hash2(a, b) == row[0]
        state, trace = h.modifiedSponge([a, b, 0, 0])
        assert len(trace) == 63 and trace[-1] == row and state == row


def check_tree(tree, leaves):
    h, n = tree.hash, len(leaves)
    want = heap_nodes(leaves, h.hash2, None)
    assert tree.nodes == want and tree.root == want[1]
    paths = tree.proveMany(list(range(n)))
    for i in range(n):
        assert tree.prove(i) == paths[i] == [want[n + i]] + [want[((n + i) >> l) ^ 1] for l in range(n.bit_length() - 1)]
    for i in sorted({0, n - 1, n // 3}):
        assert RescueMerkleTree.verify(tree.root, i, paths[i], h.hash2)
        for k in range(len(paths[i])):                # one element of the path changed: refused
            bad = list(paths[i])
            bad[k] = (bad[k] + 1) % h.field.modulus
            assert not RescueMerkleTree.verify(tree.root, i, bad, h.hash2)


@pytest.mark.parametrize('n', [2, 4, 64])
def test_trees_on_the_fallback(oracle_backend, n):
    f = PrimeField(backend=oracle_backend)
    rng = random.Random(n)
    leaves = [rng.randrange(f.modulus) for _ in range(n)]
    h = rescue4x128(f) if n < 64 else random_hash(f, rng, 3, 3)
    tree = RescueMerkleTree(h, leaves)
    assert tree.deviceNodes is None
    check_tree(tree, leaves)
    if n == 4:                                       # leaves already on a device: the same tree
        assert RescueMerkleTree(h, f.newVectorFrom(leaves)).nodes == tree.nodes


def test_the_shared_tree_base_keeps_the_two_faces_apart(oracle_backend):
    """both trees over the same 8 leaves: each one's proveMany is its own prove, index by index, and each refuses under its own name"""
    from genstark_amd.hades import HadesHash, HadesMerkleTree
    f = PrimeField(backend=oracle_backend)
    rng = random.Random(8)
    leaves = [rng.randrange(f.modulus) for _ in range(8)]
    for name, tree in (('RescueMerkleTree', RescueMerkleTree(random_hash(f, rng, 3, 2), leaves)), ('HadesMerkleTree', HadesMerkleTree(HadesHash(f, 3, 2, 1, 3), leaves, 1))):
        paths = tree.proveMany(list(range(8)))
        for i in range(8):
            assert tree.prove(i) == paths[i] and paths[i][0] == leaves[i] and len(paths[i]) == 4 and all(isinstance(v, int) for v in paths[i])
        for bad in (8, -1):
            with pytest.raises(GstarkError, match=f'^{name}: an index is outside of the 8 leaves'):
                tree.proveMany([0, bad])
    with pytest.raises(GstarkError, match='^RescueMerkleTree: 0 leaves'):                # an n x 1 Matrix is leaves of the Hades face alone
        RescueMerkleTree(random_hash(f, rng, 3, 2), f.newMatrixFrom([[v] for v in leaves]))


def test_bad_shapes_raise(oracle_backend):
    f = PrimeField(backend=oracle_backend)
    p = f.modulus
    good = dict(alpha=3, inv_alpha=-rescue.INV_ALPHA, width=4, rounds=32, mds=rescue.MDS, constants=rescue.SEED_CONSTANTS)
    for change in (dict(width=1), dict(width=9), dict(rounds=0), dict(alpha=1), dict(constants=rescue.SEED_CONSTANTS[:-1]),
                   dict(constants=rescue.SEED_CONSTANTS + [1]), dict(mds=rescue.MDS[:3]), dict(mds=[row[:3] for row in rescue.MDS]),
                   dict(inv_alpha=0), dict(inv_alpha=p - 1), dict(inv_alpha=-(p - 1))):
        with pytest.raises(GstarkError):
            RescueHash(f, **dict(good, **change))
    rng = random.Random(5)
    h4, h2 = random_hash(f, rng, 4, 2), random_hash(f, rng, 2, 2)
    for bad in ([], [1, 2, 3, 4, 5]):
        with pytest.raises(GstarkError):
            h4.sponge(bad)
        with pytest.raises(GstarkError):
            h4.modifiedSponge(bad)
        with pytest.raises(GstarkError):
            h4.hashMany([bad])
    with pytest.raises(GstarkError):
        h4.hashMany([[1, 2]], digest=3)
    with pytest.raises(GstarkError):
        h4.hashMany([[1, 2], [1]])
    for hash, leaves in ((h2, [1, 2]), (h4, [1, 2, 3]), (h4, [1]), (h4, [])):
        with pytest.raises(GstarkError):
            RescueMerkleTree(hash, leaves)
    tree = RescueMerkleTree(h4, [1, 2, 3, 4])
    for bad in (4, -1):
        with pytest.raises(GstarkError):
            tree.prove(bad)
    assert h4.hashMany([[1, 2]], digest=2).toValues() == [h4.modifiedSponge([1, 2])[1][-1][:2]]
    assert h4.hashMany([[1, 2, 3, 4]], modified=False).toValues() == [h4.sponge([1, 2, 3, 4])[0][:1]]


def merkle_statement(f, tree, index, depth):
    """RescueMP for the path of leaf `index`: (stark, assertions over `tree.root`, inputs, first row)"""
    from genstark_amd._mirror.stark import Stark
    path = tree.prove(index)
    bits = [0] + [(index >> j) & 1 for j in range(depth)][:-1]          # merkleProof.ts:162-164
    air = rescue_merkle_proof_air(f, bits)
    inputs, first = rescue_merkle_inputs(f, path[0], path[1:])
    top = (index >> (depth - 1)) & 1
    return Stark(air, OPTS), [{'step': 32 * depth - 1, 'register': 4 * top, 'value': tree.root}], inputs, first


def test_merkle_statement_under_the_mirror_stark(oracle_backend):
    from genstark_amd.errors import StarkError
    f = PrimeField(backend=oracle_backend)
    rng = random.Random(7)
    leaves = [rng.randrange(f.modulus) for _ in range(4)]
    tree = RescueMerkleTree(rescue4x128(f), leaves)
    for index in (1, 2):                             # the root in register 0, and in register 4
        stark, assertions, inputs, first = merkle_statement(f, tree, index, 2)
        assert first == [leaves[index], leaves[index ^ 1], 0, 0, leaves[index ^ 1], leaves[index], 0, 0]
        trace = stark.air.hostTrace(first, inputs=inputs)
        assert trace[63][assertions[0]['register']] == tree.root
        if index == 2:
            continue
        proof = stark.prove(assertions, inputs, first)
        data = stark.serialize(proof)
        assert stark.verify(assertions, stark.parse(data))
        with pytest.raises(StarkError):
            stark.verify([dict(assertions[0], value=tree.root ^ 1)], stark.parse(data))


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------
WIDTHS = (2, 3, 4, 8)
SEAM_COUNTS = (1, 7, 8, 9, 63, 64, 65, 257, 1000)        # the seams of a group of 8 lanes and of a wave; several workgroups
DISTINCT = 997                                           # rows beyond this repeat the first ones: no longer host reference, other places


flavour = flavour_fixture('p128', 'q64', 'p224')


def check_both_forms(h, rows, counts, sponges=(True, False), digests=(1, 2), forms=(0, 1, 2)):
    f = h.field
    base = {m: [(h.modifiedSponge if m else h.sponge)(r)[1][-1][:2] for r in rows[:DISTINCT]] for m in sponges}      # once, shared
    for count in counts:
        src = f.newMatrixFrom([rows[i % DISTINCT] for i in range(count)])
        for m in sponges:
            want = [base[m][i % DISTINCT] for i in range(count)]
            for digest in digests:
                for form in forms:
                    got = h.hashMany(src, digest, m, form).toValues()
                    assert got == [w[:digest] for w in want], (h.width, count, m, digest, form)


@pytest.mark.gpu
@pytest.mark.parametrize('width', WIDTHS)
def test_permutations_at_the_seams(flavour, width):
    f = PrimeField(backend=flavour)
    rng = random.Random(0x5E5C + width)
    limit = flavour.lib.gs_rescue_spread_limit()
    assert limit >= 1
    counts = sorted(set(SEAM_COUNTS + (min(limit, 4096), min(limit + 1, 4096))))
    h = random_hash(f, rng, width, 2)
    assert h.onDevice
    for arity in sorted({1, width - 1, width}):
        check_both_forms(h, input_rows(rng, f.modulus, DISTINCT if arity == width else 65, arity), counts if arity == width else (9, 65))
    rows = input_rows(rng, f.modulus, 65, width)
    one = random_hash(f, rng, width, 1)              # no double round in the modified form: the identity on the inputs
    assert one.hashMany(rows, 2, True).toValues() == [r[:2] for r in rows]
    check_both_forms(one, rows, (65,))
    check_both_forms(random_hash(f, rng, width, 3, alpha=5), rows, (65,))


@pytest.mark.gpu
def test_example_shapes():
    be = Backend(device=0)
    try:
        f = PrimeField(backend=be)
        h = rescue4x128(f)
        rows = input_rows(random.Random(4), f.modulus, 65, 2)
        check_both_forms(h, rows, (3, 65), digests=(2,), forms=(1, 2))
        assert h.hashMany([[42, 43]], 2, False).toValues() == [h.sponge([42, 43])[0]]
    finally:
        be.close()
    be = Backend(device=0, modulus=_abi.MODULUS_64)
    try:
        f = PrimeField(backend=be)
        check_both_forms(rescue2x64(f), input_rows(random.Random(5), f.modulus, 65, 1), (65,), digests=(2,), forms=(1, 2))
    finally:
        be.close()


@pytest.mark.gpu
def test_every_branch_of_the_exponent_schedule(flavour):
    """an exponent of one word, of trailing squarings only, of one window, of every window value, of a long run of zeros"""
    f = PrimeField(backend=flavour)
    p = f.modulus
    bits = p.bit_length()
    rng = random.Random(0xE)
    rows = input_rows(rng, p, 9, 3)
    alternating = int('10' * (bits // 2), 2) % (p - 1)
    for e in (1, 2, 3, p - 2, alternating, (1 << (bits - 1)) + 1, int('1111000101' * (bits // 10), 2) % (p - 1)):
        h = random_hash(f, rng, 3, 2, inv=e)
        assert h.invExponent == e
        check_both_forms(h, rows, (9,), digests=(2,), forms=(1, 2))
        # ... and against pow alone: one double round by hand
        s = [pow(x, 3, p) for x in rows[-1]]
        s = [(sum(a * b for a, b in zip(row, s)) + k) % p for row, k in zip(h.mds, h.keys[2])]
        s = [pow(x, e, p) for x in s]
        s = [(sum(a * b for a, b in zip(row, s)) + k) % p for row, k in zip(h.mds, h.keys[3])]
        assert h.hashMany([rows[-1]], 2).toValues() == [s[:2]]


def host_nodes(h, leaves):
    return heap_nodes(leaves, h.hash2, 0)


def check_trees(be, rng, sizes=(2, 4, 64, 128, 256, 512, 1 << 11)):
    """every node; the same tree twice back to back; the paths of one call"""
    f = PrimeField(backend=be)
    h = random_hash(f, rng, 3, 2)                    # few rounds: the host reference of 2^11 leaves stays short
    for n in sizes:
        leaves = [rng.randrange(f.modulus) for _ in range(n)]
        want = host_nodes(h, leaves)
        src = f.newVectorFrom(leaves)
        tree, again = RescueMerkleTree(h, src), RescueMerkleTree(h, src)
        raw = tree.deviceNodes.toBuffer()
        assert tree.deviceNodes.toValues() == want, n
        assert again.deviceNodes.toBuffer() == raw, n
        assert tree.root == want[1] and tree.nodes[1:] == want[1:] and tree.nodes[0] is None
        indexes = [0, n - 1, n // 2, n // 2] + [rng.randrange(n) for _ in range(100)]
        paths = tree.proveMany(indexes)
        for i, path in zip(indexes, paths):
            assert path == [want[n + i]] + [want[((n + i) >> l) ^ 1] for l in range(n.bit_length() - 1)], (n, i)
        with pytest.raises(GstarkError, match='outside'):
            tree.proveMany([0, n])
    # leaves already in place: no copy
    n = sizes[-1] if len(sizes) == 1 else 64
    leaves = [rng.randrange(f.modulus) for _ in range(n)]
    nodes = f.newVectorFrom([7] * n + leaves)
    be.call('gs_rescue_merkle', h.handle(), C.c_void_p(nodes.ptr + n * f.elementSize), n, C.c_void_p(nodes.ptr))
    assert nodes.toValues() == host_nodes(h, leaves)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['p128', 'p224'])
def test_trees_and_paths(name):
    be = Backend(device=0, modulus=FLAVOURS[name])
    try:
        check_trees(be, random.Random(0x7EE))
        if name == 'p128':                           # the example's parameter set, width 4
            f = PrimeField(backend=be)
            h = rescue4x128(f)
            leaves = [random.Random(3).randrange(f.modulus) for _ in range(16)]
            tree = RescueMerkleTree(h, leaves)
            assert tree.deviceNodes.toValues() == host_nodes(h, leaves)
            assert RescueMerkleTree.verify(tree.root, 11, tree.prove(11), h.hash2)
    finally:
        be.close()


@pytest.mark.gpu
def test_bad_shapes_are_refused_by_the_library(hip_backend):
    f = PrimeField(backend=hip_backend)
    es, call = f.elementSize, hip_backend.call
    h = C.c_void_p()
    blob = bytes(19 * 9 * es)
    for width, rounds, alpha, e in ((1, 8, 3, 5), (9, 8, 3, 5), (3, 0, 3, 5), (3, 8, 1, 5), (3, 8, 3, 0), (3, 8, 3, f.modulus - 1), (3, 8, 3, f.modulus)):
        with pytest.raises(GstarkError, match='rescue_create'):
            call('gs_rescue_create', width, rounds, alpha, e.to_bytes(es, 'little'), blob, blob, C.byref(h))
    rng = random.Random(1)
    h3, h2 = random_hash(f, rng, 3, 2), random_hash(f, rng, 2, 2)
    buf = f.newMatrix(16, 3)
    ptr = C.c_void_p(buf.ptr)
    for arity in (0, 4):
        with pytest.raises(GstarkError, match='rescue_hash: .*do not fit'):
            call('gs_rescue_hash', h3.handle(), ptr, 4, arity, 1, 1, 0, ptr)
    with pytest.raises(GstarkError, match='rescue_hash: a digest'):
        call('gs_rescue_hash', h3.handle(), ptr, 4, 2, 3, 1, 0, ptr)
    with pytest.raises(GstarkError, match='rescue_hash: modified'):
        call('gs_rescue_hash', h3.handle(), ptr, 4, 2, 1, 2, 0, ptr)
    with pytest.raises(GstarkError, match='rescue_hash: form'):
        call('gs_rescue_hash', h3.handle(), ptr, 4, 2, 1, 1, 3, ptr)
    with pytest.raises(GstarkError, match='rescue_hash: form 2'):
        call('gs_rescue_hash', h3.handle(), ptr, (1 << 24) + 1, 2, 1, 1, 2, ptr)
    for n in (3, 1, 0):
        with pytest.raises(GstarkError, match='rescue_merkle: the number of leaves'):
            call('gs_rescue_merkle', h3.handle(), ptr, n, ptr)
    with pytest.raises(GstarkError, match='rescue_merkle: two nodes do not fit'):
        call('gs_rescue_merkle', h2.handle(), ptr, 4, ptr)


@pytest.mark.gpu
def test_device_tree_feeds_the_merkle_proof_stark(hip_backend):
    from genstark_amd.errors import StarkError
    from genstark_amd.native import NativeProver
    f = PrimeField(backend=hip_backend)
    rng = random.Random(16)
    leaves = [rng.randrange(f.modulus) for _ in range(16)]
    h = rescue4x128(f)
    tree = RescueMerkleTree(h, leaves)
    assert tree.deviceNodes is not None

    class Control:                                    # the same tree from host integers
        nodes = host_nodes(h, leaves)
        root = nodes[1]
        prove = staticmethod(lambda i: [Control.nodes[16 + i]] + [Control.nodes[((16 + i) >> l) ^ 1] for l in range(4)])
    assert tree.root == Control.root
    proofs = []
    for t in (tree, Control):
        stark, assertions, inputs, first = merkle_statement(f, t, 11, 4)
        nat = NativeProver(stark)
        proofs.append(nat.prove_bytes(assertions, inputs, first))
    assert proofs[0] == proofs[1]
    assert nat.verify_bytes(assertions, proofs[0]) is True
    with pytest.raises(StarkError):
        nat.verify_bytes([dict(assertions[0], value=assertions[0]['value'] ^ 1)], proofs[0])


@pytest.mark.gpu
def test_runtime_modulus_flavour():
    from test_runtime_modulus import PRIMES
    q = PRIMES[12]                                    # 127 bits
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'runtime', str(q)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'runtime rescue: modulus {q} ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---- node ---------------------------------------------------------------------------------------------------------------------------
def js_expectations(path):
    """what tests/js_rescue.js must find, from host integers: per field a width-4 hash of random constants (3 rounds) — both sponges over
    rows of two inputs, hash2, and a tree of 16 leaves —, and for the 128-bit field the example's constants after unrollConstants"""
    rng = random.Random(0x25)
    out = []
    for modulus in (_abi.MODULUS_128, _abi.MODULUS_64):
        f = HostField(modulus)
        h = random_hash(f, rng, 4, 3)
        rows = [[0, 1], [modulus - 1, 5]] + [[rng.randrange(modulus) for _ in range(2)] for _ in range(68)]
        leaves = [rng.randrange(modulus) for _ in range(16)]
        s = lambda v: [s(x) for x in v] if isinstance(v, list) else str(v)
        out.append({'modulus': str(modulus), 'alpha': '3', 'invAlpha': str(h.invAlpha), 'rounds': 3, 'mds': s(h.mds),
                    'constants': s(h.iConstants + [v for row in h.cMatrix for v in row] + h.cConstants), 'keys': s(h.keys), 'rows': s(rows),
                    'modified': s([h.modifiedSponge(r)[1][-1][:2] for r in rows]), 'sponge': s([h.sponge(r)[1][-1][:2] for r in rows]),
                    'trace': s(h.sponge(rows[2])[1]), 'leaves': s(leaves), 'nodes': s(host_nodes(h, leaves)[1:]),
                    'example': {'invAlpha': str(rescue.INV_ALPHA), 'mds': s(rescue.MDS), 'constants': s(rescue.SEED_CONSTANTS)},
                    'exampleKeys': s(rescue4x128(f).keys[:3] + rescue4x128(f).keys[-1:]) if modulus == _abi.MODULUS_128 else None})
    with open(path, 'w') as fh:
        json.dump(out, fh)


@needs_node
def test_js_on_a_library_without_the_entries(tmp_path):
    """the host members equal the Python host; the device members throw an Error that names what is missing"""
    run_js('rescue', 'double', tmp_path, js_expectations)


@needs_node
@pytest.mark.gpu
def test_js_on_hip(tmp_path):
    run_js('rescue', 'hip', tmp_path, js_expectations)


if __name__ == '__main__':
    q = int(sys.argv[2])
    be = Backend(device=0, modulus=q)
    assert be.name == 'hip-gfx950' and be.element_size == 32 and be.modulus == q
    rng = random.Random(q % 65521)
    f = PrimeField(backend=be)
    for width in (2, 4, 5):
        h = random_hash(f, rng, width, 2)
        check_both_forms(h, input_rows(rng, q, 300, width), (9, 300))
    check_trees(be, rng, sizes=(64,))
    print(f'runtime rescue: modulus {q} ok')
