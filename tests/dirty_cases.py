"""One case per user of the context's block cache (gs_alloc / gs_tmp_alloc, csrc/ctx.hip), for tests/test_dirty_workspace.py.  Not a test
module.

The cache hands a freed block straight back with whatever its last user left in it, so from its second call on every entry runs on
dirty memory.  A case makes that state on purpose: `decoy` and `probe` are two inputs of ONE shape (the same workspace and output
sizes, so the probe's blocks are the decoy's), the decoy dense where the probe is sparse, so that what the decoy leaves behind is
wrong for the probe.

    Case.make(rng, shape, f) -> Made(decoy, probe, run, want, kernels)
        f         anything with .modulus, .elementSize and .le(): a PrimeField, or a FieldShape (no backend: the CPU tier)
        run(f, x) the entry on PrimeField f, every output byte of it (outputs go back to the cache when run returns)
        want      the bytes run(f, probe) must return: from Python integers, hashlib, or the host members of the package over a
                  HostField (hades.py, rescue_hash.py, field_tree.py, sparse_tree.py, curve.py, the _host_* functions of field.py), which
                  the CPU tier of their own test modules holds to their definitions.  Never from the library under test.
        kernels   names (or their beginnings) that Backend.traffic() must show after run(f, probe): the case reaches the launch, and
                  with it the allocation, it is there for

WORKSPACE_SITES is the number of `gs_alloc(` / `gs_tmp_alloc(` call sites per file of csrc/; tests/test_dirty_workspace.py compares it
with the sources, and every file of it is named by a case — but for DEFINITION_SITES, the definitions in ctx.hip and the declaration in
common.h, which are counted and use nothing: a new user of the cache fails there until it has a case here."""
import collections
import ctypes as C
import hashlib
import os
import random

from genstark_amd._abi import HASH_ALGS, MODULUS_64, MODULUS_128, MODULUS_224, FriLayer
from genstark_amd.curve import Curve
from genstark_amd.field import Matrix, PrimeField, Vector, _host_divmod, _host_eval, _host_interpolate, _host_mul_linear, host_sqrt
from genstark_amd.hades import HadesHash, HadesMerkleTree
from genstark_amd.hostfield import HostField
from genstark_amd.rescue_hash import RescueHash, RescueMerkleTree
from genstark_amd.sparse_tree import HadesSparseMerkleTree, RescueSparseMerkleTree

DEFINITION_SITES = {'common.h': 1, 'ctx.hip': 3}      # the declaration and the two definitions (one calls the other): counted, and no case's to name
WORKSPACE_SITES = {
    'air_mimc.hip': 1, 'air_vm.hip': 1, 'boundary.hip': 1, 'common.h': 1, 'ctx.hip': 3, 'diagnose.hip': 1, 'field_tree.hip': 5, 'hash.hip': 2, 'msm.hip': 1,
    'ntt.hip': 14, 'pointwise.hip': 3, 'poly.hip': 1, 'prover.cc': 1, 'scan.hip': 1, 'sponge_common.h': 2,
}

Case = collections.namedtuple('Case', 'name flavours shapes make files')
Made = collections.namedtuple('Made', 'decoy probe run want kernels')
ALL = ('p128', 'p224', 'q64', 'rt')
CASES = []


def case(name, shapes, files, flavours=ALL):
    def register(make):
        CASES.append(Case(name, tuple(flavours), tuple(shapes), make, tuple(files)))
        return make
    return register


class FieldShape:
    """what make() reads of a field, without a backend"""

    def __init__(self, modulus, element_size):
        self.modulus, self.elementSize = modulus, element_size

    def le(self, v):
        return int(v).to_bytes(self.elementSize, 'little')


def le(f, values):
    return b''.join(f.le(v) for v in values)


def flat(f, obj):
    """the bytes of a result of the package's members: elements little-endian, bools and None as one byte, sequences in order"""
    if isinstance(obj, (bytes, bytearray)):
        return bytes(obj)
    if isinstance(obj, bool):
        return b'\x01' if obj else b'\x00'
    if obj is None:
        return b'\xfe'
    if isinstance(obj, int):
        return f.le(obj)
    return b''.join(flat(f, x) for x in obj)


def two_adicity(p):
    return ((p - 1) & -(p - 1)).bit_length() - 1


def root_of_unity(p, order):
    """an element of that order (a power of two), as PrimeField.getRootOfUnity finds it: the first g^((p-1)/order) of order `order`"""
    return HostField(p).getRootOfUnity(order)


def sprinkle(rng, values, fill, every):
    out = list(values)
    for i in range(0, len(out), every):
        out[i] = fill
    return out


def ntt_ints(p, coeffs, w, n):
    """sum_k coeffs[k] w^(i k), i < n: radix 2 on Python integers (coeffs zero-extended to n)"""
    a = list(coeffs) + [0] * (n - len(coeffs))
    if n == 1:
        return a
    even, odd = ntt_ints(p, a[0::2], w * w % p, n // 2), ntt_ints(p, a[1::2], w * w % p, n // 2)
    out, t = [0] * n, 1
    for i in range(n // 2):
        x = t * odd[i] % p
        out[i], out[i + n // 2] = (even[i] + x) % p, (even[i] - x) % p
        t = t * w % p
    return out


def host_hash(alg):
    return (lambda b: hashlib.sha256(b).digest()) if alg == 'sha256' else (lambda b: hashlib.blake2s(b, digest_size=32).digest())


def merkle_nodes(leaves, H):
    """the heap layout: 32 zero bytes at node 0, H(left || right) above the leaves (which are not part of the node array)"""
    n = len(leaves)
    nodes = [bytes(32)] * n + list(leaves)
    for i in range(n - 1, 0, -1):
        nodes[i] = H(nodes[2 * i] + nodes[2 * i + 1])
    return nodes[:n]


# ---- pointwise.hip -----------------------------------------------------------------------------------------------------------------------
@case('eval_poly_at', (1, 257, 1000), ('pointwise.hip',))
def _eval_poly_at(rng, n, f):
    """gs_eval_poly_at: the power series of x in a temporary, then a dot product"""
    p = f.modulus
    decoy = ([p - 1] * n, p - 1)
    probe = ([rng.randrange(1, p)] + sprinkle(rng, [rng.randrange(p) for _ in range(n - 1)], 0, 7), rng.randrange(2, p))

    def run(f, x):
        return f.le(f.evalPolyAt(f.newVectorFrom(x[0]), x[1]))
    return Made(decoy, probe, run, f.le(_host_eval(probe[0], [probe[1]], p)[0]), ('k_power_series',))


@case('batch_inverse', (257, 16384 + 300), ('pointwise.hip',))
def _batch_inverse(rng, n, f):
    """gs_vec_inv / gs_vec_div: a thread per element below 16 384, several elements per thread above; zeros sprinkled in, and as the
    whole share of a workgroup"""
    p = f.modulus
    decoy = ([rng.randrange(1, p) for _ in range(n)], [p - 1] * n)
    xs = sprinkle(rng, [rng.randrange(1, p) for _ in range(n)], 0, 5)
    at = 256 if n > 512 else 0
    xs[at:at + 256] = [0] * min(256, n - at)
    xs[-1] = rng.randrange(1, p)
    probe = (xs, [rng.randrange(p) for _ in range(n)])

    def run(f, x):
        a, b = f.newVectorFrom(x[0]), f.newVectorFrom(x[1])
        return f.invVectorElements(a).toBuffer() + f.divVectorElements(b, a).toBuffer()
    inv = [pow(x, -1, p) if x else 0 for x in probe[0]]
    return Made(decoy, probe, run, le(f, inv) + le(f, [y * i % p for y, i in zip(probe[1], inv)]), ('k_batch_inv',))


@case('combine_many', ((65, 300), (130, 257)), ('pointwise.hip',))
def _combine_many(rng, shape, f):
    """gs_combine_many over more vectors than one launch carries (GS_MAX_COMBINE = 64): the later launches add to what the first wrote"""
    count, n = shape
    p = f.modulus
    decoy = ([[p - 1] * n for _ in range(count)], [p - 1] * count)
    probe = ([sprinkle(rng, [rng.randrange(p) for _ in range(n)], 0, 3) for _ in range(count)], sprinkle(rng, [rng.randrange(p) for _ in range(count)], 0, 4))

    def run(f, x):
        return f.combineManyVectors([f.newVectorFrom(col) for col in x[0]], x[1]).toBuffer()
    want = [sum(col[i] * k for col, k in zip(*probe)) % p for i in range(n)]
    return Made(decoy, probe, run, le(f, want), ('k_combine_many',))


# ---- ntt.hip -----------------------------------------------------------------------------------------------------------------------------
def _ntt_kernels(f, logn):
    if f.modulus != MODULUS_128:
        return ()                                                            # (the passes of the other flavours are not tallied)
    return ('k_ntt_pass_lz',) if logn < 10 else ('k_ntt_wave',)


@case('ntt_eval', (9, 10, 13), ('ntt.hip',))
def _ntt_eval(rng, logn, f):
    """gs_eval_polys_at_roots at a size of two passes (in -> temporary -> out): full-length rows, then ragged short ones — one
    coefficient (the Horner route), n / 16 (a low-degree extension) and an odd length — which the first pass zero-extends as it loads"""
    p, n, rows = f.modulus, 1 << logn, 3
    w = root_of_unity(p, n)
    plens = (1, n // 16, n // 2 + 1)
    decoy = [(n, [[p - 1] * n for _ in range(rows)]) for _ in plens]
    probe = [(plen, [[rng.randrange(p) for _ in range(plen)] for _ in range(rows)]) for plen in plens]

    def run(f, x):
        out = b''
        for plen, polys in x:
            m, ev = f.newMatrixFrom(polys), f.newMatrix(rows, n)
            f.backend.call('gs_eval_polys_at_roots', C.c_void_p(m.ptr), rows, plen, f.le(w), n, C.c_void_p(ev.ptr))
            out += ev.toBuffer()
        return out
    want = b''.join(le(f, ntt_ints(p, poly, w, n)) for _, polys in probe for poly in polys)
    return Made(decoy, probe, run, want, _ntt_kernels(f, logn))


@case('ntt_inverse', (9, 12), ('ntt.hip',))
def _ntt_inverse(rng, logn, f):
    """gs_interpolate_roots (the 1 / n scale rides on the last pass), rows of evaluations of short polynomials: the high coefficients
    of the result are zeros the transform has to produce"""
    p, n, rows = f.modulus, 1 << logn, 2
    w = root_of_unity(p, n)
    decoy = [[p - 1 - i for i in range(n)] for _ in range(rows)]
    coeffs = [[rng.randrange(p) for _ in range(plen)] + [0] * (n - plen) for plen in (3, n // 16)]
    probe = [ntt_ints(p, c, w, n) for c in coeffs]

    def run(f, x):
        m, out = f.newMatrixFrom(x), f.newMatrix(rows, n)
        f.backend.call('gs_interpolate_roots', C.c_void_p(m.ptr), rows, f.le(w), n, C.c_void_p(out.ptr))
        return out.toBuffer()
    return Made(decoy, probe, run, b''.join(le(f, c) for c in coeffs), _ntt_kernels(f, logn))


# ---- hash.hip ----------------------------------------------------------------------------------------------------------------------------
@case('row_hash_65_columns', (('sha256', 300), ('blake2s256', 257)), ('hash.hip',))
def _row_hash(rng, shape, f):
    """gs_hash_merge_rows over 65 columns: more than the kernel-argument table holds, the pointers travel through a temporary"""
    alg, n = shape
    p, count, H = f.modulus, 65, host_hash(alg)
    decoy = [[p - 1] * n for _ in range(count)]
    probe = [sprinkle(rng, [rng.randrange(p) for _ in range(n)], 0, 2) for _ in range(count)]

    def run(f, x):
        be = f.backend
        vecs = [f.newVectorFrom(col) for col in x]
        out = Vector(be, n, element_size=32)
        be.call('gs_hash_merge_rows', HASH_ALGS[alg], be.ptr_array([v.ptr for v in vecs]), count, n, C.c_void_p(out.ptr))
        return out.toBuffer()
    want = b''.join(H(b''.join(f.le(col[i]) for col in probe)) for i in range(n))
    return Made(decoy, probe, run, want, (f'k_hash_merge_rows_table<{HASH_ALGS[alg]}>',))


@case('merkle_commit', (('sha256', 9, 1), ('blake2s256', 9, 3), ('blake2s256', 16, 1), ('sha256', 16, 3)), ('hash.hip',))
def _merkle_commit(rng, shape, f):
    """gs_merkle_commit_rows: 2^9 leaves are the first tree of several subtree workgroups, whose last arrival builds the top (the
    context's arrival counter); 2^16 the first that streams its wide layers"""
    alg, logn, count = shape
    p, n, H = f.modulus, 1 << logn, host_hash(alg)
    mask = (1 << (8 * f.elementSize)) - 1
    decoy = [[p - 1] * n for _ in range(count)]
    probe = [[rng.getrandbits(8 * f.elementSize) % p if i % 3 else 0 for i in range(n)] for _ in range(count)]
    assert all(v <= mask for col in probe for v in col)

    def run(f, x):
        be = f.backend
        vecs = [f.newVectorFrom(col) for col in x]
        leaves, nodes = Vector(be, n, element_size=32), Vector(be, n, element_size=32)
        be.call('gs_merkle_commit_rows', HASH_ALGS[alg], be.ptr_array([v.ptr for v in vecs]), count, n, C.c_void_p(leaves.ptr), C.c_void_p(nodes.ptr))
        return leaves.toBuffer() + nodes.toBuffer()
    leaves = [H(b''.join(f.le(col[i]) for col in probe)) for i in range(n)]
    a = HASH_ALGS[alg]
    kernels = (f'k_merkle_subtree<{a}, {1 if count == 1 else 2}>',) if logn <= 15 else (f'k_merkle_fused<{a}, {1 if count == 1 else 2}>', f'k_merkle_subtree<{a}, 0>')
    return Made(decoy, probe, run, b''.join(leaves) + b''.join(merkle_nodes(leaves, H)), kernels)


@case('merkle_build', (('sha256', 9), ('blake2s256', 11)), ('hash.hip',))
def _merkle_build(rng, shape, f):
    """gs_merkle_build over given digests"""
    alg, logn = shape
    n, H = 1 << logn, host_hash(alg)
    decoy = [b'\xff' * 32] * n
    probe = [bytes(32) if i % 4 == 0 else rng.getrandbits(256).to_bytes(32, 'little') for i in range(n)]

    def run(f, x):
        be = f.backend
        leaves, nodes = Vector(be, n, element_size=32), Vector(be, n, element_size=32)
        be.upload(leaves.ptr, b''.join(x))
        be.call('gs_merkle_build', HASH_ALGS[alg], C.c_void_p(leaves.ptr), n, C.c_void_p(nodes.ptr))
        return nodes.toBuffer()
    return Made(decoy, probe, run, b''.join(merkle_nodes(probe, H)), (f'k_merkle_subtree<{HASH_ALGS[alg]}, 0>',))


def fri_layers_ints(f, alg, w, n, step, vals, x, nlayers):
    """gs_fri_layers layer by layer on Python integers and hashlib (LowDegreeProver.ts:176-221): the cubic through each row's four points at
    the layer's point, the leaves over the rows of the transposed next column, the tree, the root, and the next point = sha256(root)
    as a big-endian integer mod p.  -> per layer (next column, leaves, nodes, root, point)"""
    p, H = f.modulus, host_hash(alg)
    out, m = [], len(vals)
    for _ in range(nlayers):
        rows = m // 4
        nxt = []
        for r in range(rows):
            pts = [(pow(w, (r + c * rows) * step, p), vals[r + c * rows]) for c in range(4)]
            acc = 0
            for j, (xj, yj) in enumerate(pts):
                num = den = 1
                for k, (xk, _) in enumerate(pts):
                    if k != j:
                        num, den = num * (x - xk) % p, den * (xj - xk) % p
                acc = (acc + yj * num * pow(den, -1, p)) % p
            nxt.append(acc)
        q = rows // 4
        leaves = [H(b''.join(f.le(nxt[j + k * q]) for k in range(4))) for j in range(q)]
        nodes = merkle_nodes(leaves, H)
        root = nodes[1] if q > 1 else leaves[0]
        x = int.from_bytes(hashlib.sha256(root).digest(), 'big') % p
        out.append((nxt, leaves, nodes, root, x))
        vals, m, step = nxt, rows, step * 4
    return out


@case('fri_layers', (('blake2s256', 9, 0, 2), ('sha256', 13, 1, 3)), ('hash.hip', 'pointwise.hip'))
def _fri_layers(rng, shape, f):
    """gs_fri_layers: one workgroup runs every layer (2^9), or the first layer is several workgroups whose last arrival builds the top and
    resets the context's arrival counter (2^13); the points between the layers live in a block the context keeps"""
    alg, logm, depth, nlayers = shape
    p, m, step = f.modulus, 1 << logm, 4 ** depth
    n = m * step
    w = root_of_unity(p, n)
    decoy = ([p - 1] * m, p - 1)
    probe = (sprinkle(rng, [rng.randrange(p) for _ in range(m)], 0, 3), rng.randrange(p))

    def run(f, x):
        be = f.backend
        column, xv = f.newVectorFrom(x[0]), f.newVectorFrom([x[1]])
        layers, keep = (FriLayer * nlayers)(), []
        for i in range(nlayers):
            rows = m >> (2 * i + 2)
            keep.append((f.newVector(rows), Vector(be, rows // 4, element_size=32), Vector(be, rows // 4, element_size=32), f.newVector(1) if i % 2 == 0 else None))
            layers[i].next, layers[i].leaves, layers[i].nodes = keep[i][0].ptr, keep[i][1].ptr, keep[i][2].ptr
            layers[i].point_out = keep[i][3].ptr if keep[i][3] is not None else None
        be.call('gs_fri_layers', HASH_ALGS[alg], f.le(w), n, step, C.c_void_p(column.ptr), m, C.c_void_p(xv.ptr), nlayers, C.cast(layers, C.c_void_p))
        out = b''
        for i, (nxt, leaves, nodes, point) in enumerate(keep):
            root = C.create_string_buffer(32)
            be.call('gs_readback_wait', layers[i].ticket, root)
            out += nxt.toBuffer() + leaves.toBuffer() + nodes.toBuffer() + root.raw + (point.toBuffer() if point is not None else b'')
        return out
    want = b''
    for i, (nxt, leaves, nodes, root, point) in enumerate(fri_layers_ints(f, alg, w, n, step, probe[0], probe[1], nlayers)):
        want += le(f, nxt) + b''.join(leaves) + b''.join(nodes) + root + (f.le(point) if i % 2 == 0 else b'')
    return Made(decoy, probe, run, want, (f'k_fri_layers<{HASH_ALGS[alg]}>',))


# ---- the algebraic hash families: sponge_common.h, field_tree.hip ------------------------------------------------------------------------
def random_hades(field, rng, width, rf=4, rp=3, alpha=5):
    p = field.modulus
    return HadesHash(field, alpha, rf, rp, width, [[rng.randrange(p) for _ in range(width)] for _ in range(rf + rp)], [[rng.randrange(p) for _ in range(width)] for _ in range(width)])


def random_rescue(field, rng, width, rounds=2):
    p = field.modulus
    return RescueHash(field, 3, rng.randrange(1 << (p.bit_length() - 1), p - 1), width, rounds, [[rng.randrange(p) for _ in range(width)] for _ in range(width)],
                      [rng.randrange(p) for _ in range(width * (width + 2))])


class Family:
    """one family's hash and trees over a field (a PrimeField: the device; a HostField: host integers), from ONE seed: the same
    constants on both"""

    def __init__(self, kind, seed, digest):
        self.kind, self.seed, self.digest = kind, seed, digest

    def hash(self, field):
        rng = random.Random(self.seed)
        return random_hades(field, rng, 3 if self.digest == 1 else 6) if self.kind == 'hades' else random_rescue(field, rng, 4)

    def tree(self, field, leaves):
        h = self.hash(field)
        return HadesMerkleTree(h, [self.leaf(v) for v in leaves], self.digest) if self.kind == 'hades' else RescueMerkleTree(h, [v[0] for v in leaves])

    def tree_class(self):
        return HadesMerkleTree if self.kind == 'hades' else RescueMerkleTree

    def sparse(self, field, depth, empty):
        h = self.hash(field)
        if self.kind == 'hades':
            return HadesSparseMerkleTree(h, depth, self.digest, empty and self.leaf(empty), slots_hint=8)
        return RescueSparseMerkleTree(h, depth, empty and empty[0], slots_hint=8)

    def leaf(self, values):
        """a leaf as the family's members take it: an integer for nodes of one element, a list for two"""
        return values[0] if self.digest == 1 else list(values)

    def kernel(self, what):
        return f'k_{self.kind}_{what}'


FAMILIES = (('hades', 1), ('hades', 2), ('rescue', 1))


def _leaves(rng, p, n, digest, dense):
    if dense:
        return [[p - 1 - (i + e) % 5 for e in range(digest)] for i in range(n)]
    return [[rng.randrange(p) if (i + e) % 3 else 0 for e in range(digest)] for i in range(n)]


def _few(rng, n, count):
    """few leaves, with a repeat, a sibling pair and both ends"""
    picks = [0, n - 1, n // 2, n // 2 + 1 if n > 3 else 1, n // 2] + [rng.randrange(n) for _ in range(max(count - 5, 0))]
    return [i % n for i in picks[:count]] if count >= 5 else [rng.randrange(n) for _ in range(count)]


@case('field_tree_build_and_paths', tuple((kind, digest, n) for kind, digest in FAMILIES for n in (4, 1 << 11)), ('sponge_common.h', 'field_tree.hip'))
def _field_tree(rng, shape, f):
    """gs_hades_merkle / gs_rescue_merkle (a launch per wide level and one for the top) and the path gather (indexes through a temporary)"""
    kind, digest, n = shape
    fam, p = Family(kind, rng.getrandbits(32), digest), f.modulus
    count = 9
    decoy = (_leaves(rng, p, n, digest, True), [(7 * i) % n for i in range(count)])
    probe = (_leaves(rng, p, n, digest, False), _few(rng, n, count))

    def members(field, x):
        tree = fam.tree(field, x[0])
        unused = tree._host[0] if tree.deviceNodes is None else tree.deviceNodes.toValues()[0]      # node 0: zeros, written by the build
        return [unused, tree.nodes[1:], tree.proveMany(x[1])]

    def run(f, x):
        return flat(f, members(f, x))
    kernels = (('k_hades_merkle_level', 'k_hades_merkle_top') if n > 4 else ('k_hades_merkle_top',)) if kind == 'hades' else ('k_rescue_',)      # (k_rescue_hash<W> or k_rescue_spread<G>: the form is the library's choice by count)
    return Made(decoy, probe, run, flat(f, members(HostField(p, f.elementSize), probe)), kernels)


@case('tree_update', tuple((kind, digest, n, count) for kind, digest in FAMILIES for n, count in ((4, 3), (1 << 11, 70))), ('field_tree.hip', 'sponge_common.h'))
def _tree_update(rng, shape, f):
    """updateMany: the plan, one level's rows and the versions of the levels between share one temporary; then verifyMany and
    verifyUpdates over the records (gs_*_merkle_path_roots).  The decoy touches every leaf it can; the probe few, with a repeat, a
    sibling pair and a no-op (a leaf set to what it holds)"""
    kind, digest, n, count = shape
    fam, p = Family(kind, rng.getrandbits(32), digest), f.modulus
    leaves = _leaves(rng, p, n, digest, False)
    dense = (leaves, [(i * 5) % n for i in range(count)], _leaves(rng, p, count, digest, True))
    idx = _few(rng, n, count)
    new = _leaves(rng, p, count, digest, False)
    new[1] = list(leaves[idx[1]])                                            # a no-op
    probe = (leaves, idx, new)

    def members(field, x):
        tree = fam.tree(field, x[0])
        old_root = tree.root
        records = tree.updateMany(x[1], [fam.leaf(v) for v in x[2]])
        cls, h = fam.tree_class(), tree.hash
        paths = tree.proveMany(x[1])
        ok = cls.verifyMany(tree.root, x[1], paths, h)
        bad = cls.verifyMany(old_root, x[1], paths, h)
        updates = cls.verifyUpdates(old_root, x[1], [fam.leaf(v) for v in x[2]], records, h)
        return [[(r.before, r.root) for r in records], tree.nodes[1:], ok, bad, updates]

    def run(f, x):
        return flat(f, members(f, x))
    return Made(dense, probe, run, flat(f, members(HostField(p, f.elementSize), probe)), ('k_tree_update_gather', 'k_tree_update_commit', fam.kernel('path_roots')))


@case('sparse_tree', tuple((kind, digest, depth, count) for kind, digest in FAMILIES for depth, count in ((3, 6), (20, 40))), ('field_tree.hip', 'sponge_common.h'))
def _sparse_tree(rng, shape, f):
    """sparse trees: set (twice, so the second batch meets stored nodes and the store grows from its 8 slots), get, prove and the root;
    the probe sets few leaves, with repeats, a sibling pair, a no-op and the empty value"""
    kind, digest, depth, count = shape
    fam, p, n = Family(kind, rng.getrandbits(32), digest), f.modulus, 1 << depth
    empty = None if depth == 3 else [rng.randrange(p) for _ in range(digest)]      # None: the default leaf of zeros, which the library clears itself
    dense = (empty, [(i * 2654435761) % n for i in range(count)], _leaves(rng, p, count, digest, True), [(i * 40503) % n for i in range(count)], _leaves(rng, p, count, digest, True))
    first = _few(rng, n, count)
    second = [first[0], first[0] ^ 1, first[2]] + [rng.randrange(n) for _ in range(count - 3)]
    new1, new2 = _leaves(rng, p, count, digest, False), _leaves(rng, p, count, digest, False)
    new2[0] = list(new1[first.index(first[0])] if first.count(first[0]) == 1 else new2[0])       # what it may hold already
    new2[2] = list(empty or [0] * digest)                                    # back to the empty value
    probe = (empty, first, new1, second, new2)

    def members(field, x):
        tree = fam.sparse(field, depth, x[0])
        out = [tree.root]
        for idx, new in ((x[1], x[2]), (x[3], x[4])):
            records = tree.updateMany(idx, [fam.leaf(v) for v in new])
            out += [[(r.before, r.root) for r in records], tree.root, tree.stored]
        asked = x[1][:4] + [(x[1][0] + 1) % n, (x[3][-1] + 2) % n]             # set and never set
        out += [tree.getMany(asked), tree.proveMany(asked), tree.empties]
        return out

    def run(f, x):
        return flat(f, members(f, x))
    return Made(dense, probe, run, flat(f, members(HostField(p, f.elementSize), probe)), ('k_sparse_gather', 'k_sparse_commit', 'k_sparse_paths'))


@case('absorb_many', tuple((kind, n) for kind in ('hades', 'rescue') for n in (9, 300)), ('sponge_common.h',))
def _absorb_many(rng, shape, f):
    """absorbMany: long records first, then records of one element and of exactly `rate`; hashMany of full rows beside them"""
    kind, n = shape
    fam, p = Family(kind, rng.getrandbits(32), 2 if kind == 'hades' else 1), f.modulus
    rate = 4                                                                 # width 6 (hades), width 4 (rescue: given)
    decoy = [[[p - 1] * 23 for _ in range(n)]] * 3
    probe = [[[rng.randrange(p)] for _ in range(n)], [sprinkle(rng, [rng.randrange(p) for _ in range(rate)], 0, 2) for _ in range(n)],
             [[rng.randrange(p) for _ in range(2 * rate + 1)] for _ in range(n)]]

    def members(field, x):
        h = fam.hash(field)
        rate_of = {'rate': 3} if kind == 'rescue' else {'rate': rate}
        return [h.absorbMany(rows, fam.digest, **rate_of).toValues() for rows in x] + [h.hashMany([r[:3] for r in x[2]], fam.digest).toValues()]

    def run(f, x):
        return flat(f, members(f, x))
    return Made(decoy, probe, run, flat(f, members(HostField(p, f.elementSize), probe)), (fam.kernel('absorb'), fam.kernel('hash') if kind == 'hades' else 'k_rescue_'))      # (hashMany: k_rescue_hash<W> or k_rescue_spread<G>, by count)


# ---- poly.hip ----------------------------------------------------------------------------------------------------------------------------
POLY_SWITCH = 1 << 8                                                         # POLY_SWITCH_DEFAULT (csrc/poly_plan.h): child slots up to here are schoolbook


def _distinct(rng, p, n):
    out = set()
    while len(out) < n:
        out.add(rng.randrange(p))
    return sorted(out, key=lambda v: hashlib.sha256(str(v).encode()).digest())


@case('poly_from_roots', (5, 2 * POLY_SWITCH - 1, 2 * POLY_SWITCH + 1), ('poly.hip',))
def _poly_from_roots(rng, n, f):
    p = f.modulus
    decoy = [p - 1 - i for i in range(n)]
    probe = sprinkle(rng, _distinct(rng, p, n), 0, 4)                        # zero as a repeated root: the low coefficients vanish

    def run(f, x):
        return f.polyFromRoots(x).toBuffer()
    want = [1]
    for x in probe:
        want = _host_mul_linear(want, x, p)
    return Made(decoy, probe, run, le(f, want), ('k_poly_pair_schoolbook',) + (('k_poly_pair_pointwise',) if n > 2 * POLY_SWITCH else ()))


@case('poly_div', ((600, 299), (2 * POLY_SWITCH + 1, POLY_SWITCH + 1), (40, 3)), ('poly.hip',))
def _poly_div(rng, shape, f):
    """gs_poly_div: a full-degree pair first; then a dividend that is a multiple of the divisor (a zero remainder) with zeros inside"""
    la, lb = shape
    p = f.modulus
    decoy = ([p - 1] * la, [p - 1] * lb)
    b = sprinkle(rng, [rng.randrange(p) for _ in range(lb)], 0, 3)
    b[-1] = rng.randrange(1, p)
    q = sprinkle(rng, [rng.randrange(p) for _ in range(la - lb + 1)], 0, 2)
    q[-1] = rng.randrange(1, p)
    a = [0] * la
    for i, x in enumerate(q):
        if x:
            for j, y in enumerate(b):
                a[i + j] = (a[i + j] + x * y) % p
    probe = (a, b)

    def run(f, x):
        quotient, rest = f.divModPolys(x[0], x[1])
        return quotient.toBuffer() + rest.toBuffer()
    wq, wr = _host_divmod(a, b, p)
    assert wq == q and not any(wr)
    return Made(decoy, probe, run, le(f, wq) + le(f, wr), ('k_poly_remainder',))


@case('poly_eval_points', ((600, 2 * POLY_SWITCH + 1), (2 * POLY_SWITCH - 1, 2 * POLY_SWITCH - 1), (7, 300)), ('poly.hip',))
def _poly_eval_points(rng, shape, f):
    """gs_poly_eval_points down the subproduct tree: the probe has repeated points, zero among them"""
    plen, n = shape
    p = f.modulus
    decoy = ([p - 1] * plen, [p - 1 - i for i in range(n)])
    xs = [rng.randrange(p) for _ in range(n)]
    xs[1::5] = [xs[0]] * len(xs[1::5])
    xs[2::7] = [0] * len(xs[2::7])
    probe = (sprinkle(rng, [rng.randrange(p) for _ in range(plen)], 0, 3), xs)

    def run(f, x):
        return f.evalPolyAtPoints(x[0], x[1], method='tree').toBuffer()
    return Made(decoy, probe, run, le(f, _host_eval(probe[0], probe[1], p)), ('k_poly_pair_schoolbook', 'k_poly_down_schoolbook'))


@case('poly_interpolate_points', (5, POLY_SWITCH + 1, 2 * POLY_SWITCH + 1), ('poly.hip',))
def _poly_interpolate(rng, n, f):
    """gs_poly_interpolate_points: the flag byte is an output of one byte in a block of 256; the values are those of a short polynomial,
    so the high coefficients of the interpolant are zeros"""
    p = f.modulus
    decoy = ([p - 1 - i for i in range(n)], [p - 1] * n)
    xs = _distinct(rng, p, n)
    short = [rng.randrange(p) for _ in range(min(3, n))]
    probe = (xs, _host_eval(short, xs, p))

    def run(f, x):
        return f.interpolateAtPoints(x[0], x[1]).toBuffer()
    want = _host_interpolate(probe[0], probe[1], p)
    assert want == short + [0] * (n - len(short))
    return Made(decoy, probe, run, le(f, want), ('k_poly_pair_schoolbook', 'k_poly_down_schoolbook', 'k_poly_up_schoolbook'))


# ---- boundary.hip ------------------------------------------------------------------------------------------------------------------------
@case('boundary_polys', ((64, 50, 4), (1 << 10, 600, 3)), ('boundary.hip',))
def _boundary_polys(rng, shape, f):
    """gs_boundary_polys: every register asserted at `width` steps, then two assertions on one register and one on each of the others —
    the rows of I and Z are zero-extended to the widest, and the zeros are part of the output"""
    T, width, registers = shape
    p = f.modulus
    n = 2 * T
    omega = root_of_unity(p, n)
    g = omega * omega % p
    decoy = [(rng.sample(range(T), width), [p - 1] * width) for _ in range(registers)]
    probe = [([0, T - 1], [rng.randrange(p), 0])] + [([rng.randrange(T)], [rng.randrange(p)]) for _ in range(registers - 1)]

    def run(f, x):
        be, es = f.backend, f.elementSize
        rows = len(x)
        steps = (C.c_uint64 * (rows * width))()
        vals = bytearray(rows * width * es)
        for r, (s, v) in enumerate(x):
            for k in range(len(s)):
                steps[r * width + k] = s[k]
                vals[(r * width + k) * es:(r * width + k + 1) * es] = f.le(v[k])
        per_row = (C.c_uint32 * rows)(*[len(s) for s, _ in x])
        i_out, z_out = Matrix(be, rows, width), Matrix(be, rows, width + 1)
        be.call('gs_boundary_polys', f.le(omega), n, T, steps, bytes(vals), per_row, rows, width, C.c_void_p(i_out.ptr), C.c_void_p(z_out.ptr))
        return i_out.toBuffer() + z_out.toBuffer()
    want_i, want_z = [], []
    for s, v in probe:
        xs, z = [pow(g, k, p) for k in s], [1]
        for x in xs:
            z = _host_mul_linear(z, x, p)
        want_i += _host_interpolate(xs, v, p) + [0] * (width - len(s))
        want_z += z + [0] * (width - len(s))
    return Made(decoy, probe, run, le(f, want_i) + le(f, want_z), ('k_bd_pair_schoolbook',))


@case('eval_polys_at_points', ((3, 300, 70), (2, 5000, 9)), ('boundary.hip',))
def _eval_polys_at_points(rng, shape, f):
    """gs_eval_polys_at_points: long rows are cut into segments whose partial sums a second launch adds; the probe's rows are short
    (ragged lengths in rows of one stride)"""
    rows, stride, npoints = shape
    p = f.modulus
    decoy = ([[p - 1] * stride for _ in range(rows)], [p - 1 - i for i in range(npoints)])
    lens = [1, stride // 3, stride][:rows]
    probe = ([[rng.randrange(p) for _ in range(ln)] for ln in lens], sprinkle(rng, [rng.randrange(p) for _ in range(npoints)], 0, 5))

    def run(f, x):
        be = f.backend
        src = f.newMatrixFrom([row + [p - 1] * (stride - len(row)) for row in x[0]])      # what lies beyond a row's length is not read
        out = Matrix(be, rows, npoints)
        be.call('gs_eval_polys_at_points', C.c_void_p(src.ptr), rows, stride, (C.c_uint64 * rows)(*[len(r) for r in x[0]]), le(f, x[1]), npoints, C.c_void_p(out.ptr))
        return out.toBuffer()
    return Made(decoy, probe, run, b''.join(le(f, _host_eval(row, probe[1], p)) for row in probe[0]), ('k_eval_points_partial',))


# ---- sqrt.hip (its tables are the context's: built once, by whichever call comes first) ------------------------------------------------------
def _curve_through(rng, p):
    a, x, y = rng.randrange(1, p - 3), rng.randrange(p), rng.randrange(1, p)
    return a, (y * y - x ** 3 - a * x) % p, (x, y)


@case('field_sqrt', (65, 300), ())
def _field_sqrt(rng, n, f):
    """gs_field_sqrt: every input a square first, then non-squares and zeros (root 0, flags 0 and 1)"""
    p = f.modulus
    decoy = [pow(rng.randrange(1, p), 2, p) for _ in range(n)]
    probe = [0 if i % 4 == 0 else rng.randrange(p) for i in range(n)]

    def run(f, x):
        roots, flags = f.sqrtVectorElements(x)
        return roots.toBuffer() + flags.toBuffer()
    roots = [host_sqrt(x, p) for x in probe]
    assert any(r is None for r in roots) and any(r for r in roots)
    return Made(decoy, probe, run, le(f, [r or 0 for r in roots]) + bytes(r is not None for r in roots), ('k_field_sqrt',))


@case('curve_lift_x', (65, 300), ())
def _curve_lift_x(rng, n, f):
    """gs_curve_lift_x: the x of points first, then any x (half of them of no point: (0, 0) and flag 0) with parities"""
    p = f.modulus
    a, b, base = _curve_through(rng, p)
    host = Curve(HostField(p, f.elementSize), a, b)
    pts = [base]
    while len(pts) < n:
        pts.append(host.add(pts[-1], base) or base)
    decoy = ([pt[0] for pt in pts], [1] * n)
    probe = ([0 if i % 9 == 0 else rng.randrange(p) for i in range(n)], [rng.randrange(2) for _ in range(n)])

    def members(field, x):
        return Curve(field, a, b).liftX(x[0], x[1])

    def run(f, x):
        return flat(f, members(f, x))
    return Made(decoy, probe, run, flat(f, members(HostField(p, f.elementSize), probe)), ('k_curve_lift_x',))


# ---- diagnose.hip ------------------------------------------------------------------------------------------------------------------------
@case('nonzero_spans', ((3, 300, 257), (2, 20000, 19999)), ('diagnose.hip',))
def _nonzero_spans(rng, shape, f):
    """gs_nonzero_spans: every element non-zero first, then all zero (count 0, first = last = n) and one row with a single non-zero"""
    rows, stride, n = shape
    p = f.modulus
    decoy = [[p - 1] * stride for _ in range(rows)]
    probe = [[0] * n + [p - 1] * (stride - n) for _ in range(rows)]          # (what lies beyond n is not scanned)
    probe[-1][n // 2] = 1

    def run(f, x):
        be = f.backend
        m = f.newMatrixFrom(x)
        out = [(C.c_uint64 * rows)() for _ in range(3)]
        be.call('gs_nonzero_spans', C.c_void_p(m.ptr), rows, stride, n, *out)
        return b''.join(bytes(o) for o in out)
    counts = [sum(1 for v in row[:n] if v) for row in probe]
    firsts = [next((i for i, v in enumerate(row[:n]) if v), n) for row in probe]
    lasts = [next((i for i in range(n - 1, -1, -1) if row[i]), n) for row in probe]
    want = b''.join(b''.join(v.to_bytes(8, 'little') for v in part) for part in (counts, firsts, lasts))
    return Made(decoy, probe, run, want, ('k_nonzero_spans',))


# ---- scan.hip ----------------------------------------------------------------------------------------------------------------------------
def scan_tile(f):
    """the elements one workgroup scans: 256 threads of 64 bytes each (asserted against gs_scan_plan by the GPU tier)"""
    return 256 * 64 // f.elementSize


SCAN_LENGTHS = {'T': lambda T: T, 'T + 1': lambda T: T + 1, '2T + 37': lambda T: 2 * T + 37}      # one launch, the first of three, a short last tile


def _scan_shapes():
    return tuple(SCAN_LENGTHS)


def _scan_n(f, which):
    return SCAN_LENGTHS[which](scan_tile(f))


def _segments(values, heads):
    out = []
    for i, v in enumerate(values):
        if i == 0 or heads[i] & 1:
            out.append([])
        out[-1].append(v)
    return out


@case('scan_sum_product', _scan_shapes(), ('scan.hip',))
def _scan_sum_product(rng, which, f):
    """gs_scan: all p - 1 with every head flag set first (every tile aggregate a reset one), then random values with few flags and a
    short last tile"""
    p, n = f.modulus, _scan_n(f, which)
    decoy = ([p - 1] * n, [1] * n)
    heads = [1 if rng.randrange(n // 3 + 1) == 0 else 0 for _ in range(n)]
    probe = (sprinkle(rng, [rng.randrange(p) for _ in range(n)], 0, 401), heads)

    def run(f, x):
        v, hv = f.newVectorFrom(x[0]), Vector(f.backend, n, element_size=1)
        f.backend.upload(hv.ptr, bytes(x[1]))
        return f.prefixSumVectorElements(v, False, hv).toBuffer() + f.prefixProductVectorElements(v, True, hv).toBuffer() + f.prefixProductVectorElements(v).toBuffer()
    sums, prods, whole, acc = [], [], [], 1
    for seg in _segments(*probe):
        s, m = 0, 1
        for v in seg:
            s = (s + v) % p
            sums.append(s)
            prods.append(m)
            m = m * v % p
    for v in probe[0]:
        acc = acc * v % p
        whole.append(acc)
    kernels = ('k_scan_apply<sum>', 'k_scan_apply<product>') + (('k_scan_tiles<sum>', 'k_scan_totals<product>') if n > scan_tile(f) else ())
    return Made(decoy, probe, run, le(f, sums) + le(f, prods) + le(f, whole), kernels)


@case('scan_affine', _scan_shapes(), ('scan.hip',))
def _scan_affine(rng, which, f):
    """gs_scan_affine: x[i] = a[i] x[i-1] + b[i] with zeros in a (the chain forgets) after a decoy of all p - 1 with every head set"""
    p, n = f.modulus, _scan_n(f, which)
    decoy = ([p - 1] * n, [p - 1] * n, [1] * n, p - 1)
    heads = [1 if rng.randrange(n // 2 + 1) == 0 else 0 for _ in range(n)]
    probe = (sprinkle(rng, [rng.randrange(p) for _ in range(n)], 0, 333), [rng.randrange(p) for _ in range(n)], heads, rng.randrange(p))

    def run(f, x):
        hv = Vector(f.backend, n, element_size=1)
        f.backend.upload(hv.ptr, bytes(x[2]))
        return f.linearRecurrence(f.newVectorFrom(x[0]), f.newVectorFrom(x[1]), x[3], False, hv).toBuffer() + f.linearRecurrence(x[0][1], f.newVectorFrom(x[1]), 0, True).toBuffer()
    a, b, heads, x0 = probe
    first, second, x, y = [], [], x0, 0
    for i in range(n):
        if i == 0 or heads[i] & 1:
            x = x0
        x = (a[i] * x + b[i]) % p
        first.append(x)
        second.append(y)
        y = (a[1] * y + b[i]) % p
    return Made(decoy, probe, run, le(f, first) + le(f, second), ('k_scan_apply<affine>',) + (('k_scan_tiles<affine>',) if n > scan_tile(f) else ()))


@case('reduce', _scan_shapes(), ('scan.hip',))
def _reduce(rng, which, f):
    """gs_reduce: one row (two launches above a tile: the totals kernel writes the result) and uniform rows (totals from the apply kernel)"""
    p, n = f.modulus, _scan_n(f, which)
    cols = 37
    rows = n // cols
    decoy = [p - 1] * n
    probe = sprinkle(rng, [rng.randrange(p) for _ in range(n)], 1, 5)

    def run(f, x):
        v = f.newVectorFrom(x)
        m = Matrix(f.backend, rows, cols, owner=v._owner)
        return f.le(f.sumVectorElements(v)) + f.le(f.prodVectorElements(v)) + f.sumMatrixRows(m).toBuffer() + f.prodMatrixRows(m).toBuffer()
    prod = 1
    for v in probe:
        prod = prod * v % p
    row_sums = [sum(probe[r * cols:(r + 1) * cols]) % p for r in range(rows)]
    row_prods = []
    for r in range(rows):
        m = 1
        for v in probe[r * cols:(r + 1) * cols]:
            m = m * v % p
        row_prods.append(m)
    return Made(decoy, probe, run, f.le(sum(probe) % p) + f.le(prod) + le(f, row_sums) + le(f, row_prods),
                ('k_scan_apply<sum>', 'k_scan_apply<product>') + (('k_scan_totals<sum>', 'k_scan_totals<product>') if n > scan_tile(f) else ()))


# ---- msm.hip -----------------------------------------------------------------------------------------------------------------------------
def _msm_terms(rng, f, count):
    """a random curve through a random point, `count` multiples of it, and the scalars of a decoy (every bucket of every window) and of
    a probe (zeros, one scalar many times, a point and its opposite under one scalar: a handful of buckets)"""
    p = f.modulus
    a, b, base = _curve_through(rng, p)
    host = Curve(HostField(p, f.elementSize), a, b)
    steps = [host._hostMul(base, rng.randrange(2, 1 << 20)) for _ in range(8)]
    points = []
    while len(points) < count:
        points.append(host.add(points[-1], steps[len(points) % 8]) if points else base)
        assert points[-1] is not None
    bits = 128 if f.elementSize == 16 else 256
    limit = min(p, 1 << bits)
    dense = [rng.randrange(limit) | 1 for _ in range(count)]
    k = rng.randrange(limit)
    sparse = [0 if i % 3 == 0 else (k if i % 3 == 1 else rng.randrange(1 << 9)) for i in range(count)]
    probe_points = list(points)
    if count >= 3:
        probe_points[-1], sparse[-1], sparse[-2] = host.neg(points[-2]), k, k      # a pair that cancels
        probe_points[1] = probe_points[0]                                     # a repeated point
    return (a, b), host, points, dense, probe_points, sparse, bits


def _host_msm(host, points, scalars):
    total = None
    for pt, k in zip(points, scalars):
        total = host.add(total, host._hostMul(pt, k))
    return total


@case('msm_buckets', ((3, 0), (130, 3), (130, 0)), ('msm.hip',))
def _msm_buckets(rng, shape, f):
    """gs_curve_msm on the bucket route: a forced window of 3 bits (130 odd scalars fill every bucket of every window), and the
    plan's own width (chunks of buckets, lifted by their first digit)"""
    count, window = shape
    (a, b), host, points, dense, probe_points, sparse, bits = _msm_terms(rng, f, count)
    decoy, probe = (points, dense), (probe_points, sparse)

    def run(f, x):
        out, flag = Curve(f, a, b).msm(f.newMatrixFrom([list(pt) for pt in x[0]]), x[1], window=window, device=True)
        return out.toBuffer() + flag.toBuffer()
    total = _host_msm(host, *probe)
    kernels = ('k_msm_pairs<histogram>', 'k_msm_scan', 'k_msm_slices', 'k_msm_chunks', 'k_msm_finish') + (('k_msm_chunk_lift',) if window == 0 else ())
    return Made(decoy, probe, run, le(f, total or (0, 0)) + bytes([total is None]), kernels)


@case('msm_multiply_then_sum', (3, 300), ('msm.hip',))
def _msm_multiply_then_sum(rng, count, f):
    """gs_curve_msm on the multiply-then-sum route (the measurement's handle GSTARK_MSM_ROUTE picks it at any count), the scalars a vector of
    field elements: 16-byte ones are widened into the workspace"""
    (a, b), host, points, dense, probe_points, sparse, bits = _msm_terms(rng, f, count)
    decoy, probe = (points, dense), (probe_points, sparse)

    def run(f, x):
        before = os.environ.get('GSTARK_MSM_ROUTE')
        os.environ['GSTARK_MSM_ROUTE'] = 'multiply_then_sum'
        try:
            out, flag = Curve(f, a, b).msm(f.newMatrixFrom([list(pt) for pt in x[0]]), f.newVectorFrom(x[1]), bits=bits, device=True)
            return out.toBuffer() + flag.toBuffer()
        finally:
            if before is None:
                del os.environ['GSTARK_MSM_ROUTE']
            else:
                os.environ['GSTARK_MSM_ROUTE'] = before
    total = _host_msm(host, *probe)
    return Made(decoy, probe, run, le(f, total or (0, 0)) + bytes([total is None]), ('k_msm_block_sum',))


# ---- air_vm.hip, air_mimc.hip, prover.cc -------------------------------------------------------------------------------------------------
def _quad_air(field, steps, segment=None, init=False):
    """two registers, one cyclic constant: r0' = r0^2 + r1 + k, r1' = r0 * r1 + 3 — small, and not linear; with `segment` the trace is
    steps / segment independent runs, with `init` each run's first row is made from its raw inputs by an init program"""
    from genstark_amd.air_generic import GenericAir
    statics = [[(5 * i + 1) % 97 for i in range(2)]]
    return GenericAir(steps, 2, [2, 2], statics, lambda r, k: [r[0] * r[0] + r[1] + k[0], r[0] * r[1] + 3],
                      lambda r, n, k: [n[0] - (r[0] * r[0] + r[1] + k[0]), n[1] - (r[0] * r[1] + 3)], lambda seed: [seed[0], seed[1]], 16, field,
                      segmentLength=segment, initExpr=(lambda x: [x[0] + x[1], x[0] * x[1] + 7]) if init else None)


@case('air_vm_trace_segments', ((64, 4, False), (64, 2, True)), ('air_vm.hip',), flavours=('p128', 'p224', 'q64'))
def _air_vm_trace_segments(rng, shape, f):
    """gs_air_trace_segments with more segments than a host core takes (GS_HOST_TRACE_MAX_SEGMENTS = 8), so the trace is made on the
    device: the program, the init program (of no instructions in the first shape), the constants, the static values and the first
    rows travel through ONE temporary in 256-byte-aligned parts.  Interpreted (k_air_trace_segments), then compiled (gs_jit_trace),
    on the same context; dense first rows first, then rows of zeros with a few values"""
    steps, segment, init = shape
    p, segments = f.modulus, steps // segment
    assert segments > 8
    decoy = [[p - 1 - s, p - 2 - s] for s in range(segments)]
    probe = [[0, 0] if s % 3 else [rng.randrange(p), rng.randrange(p) if s % 2 else 0] for s in range(segments)]

    def run(f, seeds):
        be, out = f.backend, b''
        try:
            for compiled in (False, True):
                be.jit(compiled)
                out += _quad_air(f, steps, segment, init).initProvingContext([], seeds).generateExecutionTrace().toBuffer()
        finally:
            be.jit(False)                                                    # what the tests' contexts start with
        return out
    rows = _quad_air(HostField(p, f.elementSize), steps, segment, init).hostTrace(probe)
    want = b''.join(le(f, [row[r] for row in rows]) for r in range(2))
    return Made(decoy, probe, run, want + want, ('k_air_trace_segments', 'gs_jit_trace'))


@case('air_vm', (16, 64), ('air_vm.hip',), flavours=('p128', 'p224', 'q64'))
def _air_vm(rng, steps, f):
    """gs_air_constraints through the smallest generic statement: the program and its constants travel through a temporary; Q over
    the composition domain against the evaluation program run point by point on host integers.  (The trace of an unsegmented
    statement is interpreted on a host core and takes nothing from the cache: air_vm_trace_segments is the case of the trace launch.)"""
    p = f.modulus
    decoy, probe = [p - 1, p - 2], [0, rng.randrange(p)]

    def run(f, seed):
        air = _quad_air(f, steps)
        ctx = air.initProvingContext([], seed)
        trace = ctx.generateExecutionTrace()
        polys = f.interpolateRoots(ctx.executionDomain, trace)
        return trace.toBuffer() + ctx.evaluateTransitionConstraints(polys).toBuffer()
    host = HostField(p, f.elementSize)
    air = _quad_air(host, steps)
    rows = air.hostTrace(probe)
    columns = [[row[r] for row in rows] for r in range(2)]
    nc = steps * air.compositionFactor
    wc = pow(air.rootOfUnity, steps * air.extensionFactor // nc, p)
    g = pow(wc, nc // steps, p)                                              # the execution domain's generator
    ninv = pow(steps, -1, p)
    coeffs = [[v * ninv % p for v in ntt_ints(p, col, pow(g, -1, p), steps)] for col in columns]
    over = [ntt_ints(p, c, wc, nc) for c in coeffs]
    vctx, shift = air.initVerificationContext(), nc // steps
    q = [vctx.evaluateConstraintsAt(pow(wc, j, p), [over[0][j], over[1][j]], [over[0][(j + shift) % nc], over[1][(j + shift) % nc]], []) for j in range(nc)]
    want = b''.join(le(f, col) for col in columns) + b''.join(le(f, [row[k] for row in q]) for k in range(2))
    return Made(decoy, probe, run, want, ('k_air_constraints',))


def golden_proofs():
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'oracle_proofs.json')) as fh:
        return json.load(fh)


@case('mimc_proof', tuple(range(len(golden_proofs()))), ('air_mimc.hip', 'prover.cc', 'ntt.hip', 'pointwise.hip', 'hash.hip'), flavours=('p128',))
def _mimc_proof(rng, which, f):
    """a whole MiMC proof by the native driver (every buffer of it a block of the cache, the composition tables the context's) against
    the committed golden bytes; the decoy is the same statement from another seed"""
    import genstark_amd as ga
    golden = golden_proofs()[which]
    options = {'hashAlgorithm': golden['hash_algorithm'], 'extensionFactor': golden['extension_factor'], 'exeQueryCount': golden['exe_query_count'],
               'friQueryCount': golden['fri_query_count']}
    steps = golden['steps']
    probe = ([{'step': a['step'], 'register': a['register'], 'value': int(a['value'])} for a in golden['assertions']], golden['seed'])
    decoy = (None, golden['seed'] + 1 + rng.randrange(1000))                  # (its assertions are read off its own trace when it runs)

    def run(f, x):
        from genstark_amd.native import NativeProver
        stark = ga.instantiateMimc(steps, options, None, backend=f.backend)
        assertions, seed = x
        if assertions is None:
            values = ga.runMimc(f, steps, stark.air.roundConstants, seed)
            assertions = [{'step': 0, 'register': 0, 'value': values[0]}, {'step': steps - 1, 'register': 0, 'value': values[-1]}]
        return NativeProver(stark).prove_bytes(assertions, [], [seed])
    return Made(decoy, probe, run, bytes.fromhex(golden['proofHex']), ('k_mimc_composition',))


# ---- what the tests ask of the table -----------------------------------------------------------------------------------------------------
FLAVOUR_MODULI = {'p128': MODULUS_128, 'p224': MODULUS_224, 'q64': MODULUS_64}
ELEMENT_SIZES = {'p128': 16, 'p224': 32, 'q64': 16, 'rt': 32}


def rng_for(name, shape, seed=0):
    return random.Random(repr((name, shape, seed)))


def made(c, shape, f, seed=0):
    return c.make(rng_for(c.name, shape, seed), shape, f)
