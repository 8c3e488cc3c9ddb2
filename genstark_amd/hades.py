"""Poseidon hashes and Poseidon Merkle trees computed on the device (include/gstark_hades.h, csrc/hades.hip).

`HadesHash` is `createHash` of the reference's examples/poseidon/utils.ts:19-49, `HadesMerkleTree` its `MerkleTree` (digest=2: nodes of
two elements, :126-167) and `MerkleTree2` (digest=1, :169-210): the same values in the same orders.  `hash(inputs)` is host integer
arithmetic like the example's function; `hashMany`, the tree and its paths are one launch each on the context's stream (a tree: one per
wide level and one for the top), with one read-back for any number of paths.

On a backend whose library lacks the entry points (the tests' double) everything is computed on host integers instead and gives the
same values: the layer above the kernels is testable without a GPU.  The product's library has them.
"""
import ctypes as C

from ._abi import GstarkError
from .field import Matrix, Vector
from .poseidon import mds_matrix, round_constants as derived_round_constants


class HadesHash:
    """createHash(field, exp, rf, rp, stateWidth, rc?) — utils.ts:19.  round_constants: (rf + rp) rows of `width` values; mds: `width`
    rows of `width` values; both derived as the example derives them (sha256 over 'Hades<c>', the Cauchy matrix of 'HadesMDSx<i>' and
    'HadesMDSy<j>') when omitted."""

    def __init__(self, field, alpha, full_rounds, partial_rounds, width, round_constants=None, mds=None):
        alpha, rf, rp, width = int(alpha), int(full_rounds), int(partial_rounds), int(width)
        if not 2 <= width <= 8:
            raise GstarkError(f'HadesHash: a state of {width} elements is outside 2 .. 8')
        if rf < 2 or rf % 2 or rp < 0:
            raise GstarkError(f'HadesHash: {rf} full rounds (even, at least 2) and {rp} partial rounds (none or more)')
        if not 2 <= alpha < 1 << 64:
            raise GstarkError(f'HadesHash: alpha {alpha} is outside 2 .. 2^64 - 1')
        p = field.modulus
        rc = derived_round_constants(field, width, rf + rp) if round_constants is None else [[int(v) % p for v in row] for row in round_constants]
        m = mds_matrix(field, width) if mds is None else [[int(v) % p for v in row] for row in mds]
        if len(rc) != rf + rp or any(len(row) != width for row in rc):
            raise GstarkError(f'HadesHash: {rf + rp} rows of {width} round constants are needed')
        if len(m) != width or any(len(row) != width for row in m):
            raise GstarkError(f'HadesHash: the matrix has {width} rows of {width} values')
        self.field, self.alpha, self.fullRounds, self.partialRounds, self.width = field, alpha, rf, rp, width
        self.roundConstants, self.mds = rc, m
        self._handle = None

    # ---- host integers
    def permute(self, state):
        p, m, rf, rp = self.field.modulus, self.width, self.fullRounds, self.partialRounds
        for i in range(rf + rp):
            state = [(s + k) % p for s, k in zip(state, self.roundConstants[i])]
            if i < rf // 2 or i >= rf // 2 + rp:
                state = [pow(s, self.alpha, p) for s in state]
            else:
                state[m - 1] = pow(state[m - 1], self.alpha, p)
            state = [sum(a * b for a, b in zip(row, state)) % p for row in self.mds]
        return state

    def hash(self, inputs):
        """The example's hash function: 1 .. width - 1 values in, the first two elements of the final state out."""
        inputs = list(inputs)
        if not 0 < len(inputs) < self.width:
            raise GstarkError(f'HadesHash: {len(inputs)} inputs do not fit a state of {self.width} (1 .. {self.width - 1})')
        return self.permute([int(v) % self.field.modulus for v in inputs] + [0] * (self.width - len(inputs)))[:2]

    __call__ = hash

    # ---- device
    @property
    def onDevice(self):
        return hasattr(self.field.backend.lib, 'gs_hades_hash')

    def handle(self):
        """the gs_hades of this parameter set on the field's context: constants uploaded once, on first use"""
        if self._handle is None:
            f, be = self.field, self.field.backend
            h = C.c_void_p()
            be.call('gs_hades_create', self.width, self.fullRounds, self.partialRounds, self.alpha,
                    b''.join(f.le(v) for row in self.roundConstants for v in row), b''.join(f.le(v) for row in self.mds for v in row), C.byref(h))
            self._handle = h
        return self._handle

    def __del__(self):
        try:
            be = self.field.backend
            if self._handle is not None and be.ctx:
                be.lib.gs_hades_destroy(be.ctx, self._handle)
            self._handle = None
        except Exception:
            pass

    def hashMany(self, rows, digest=2):
        """One permutation per row of `rows` (a device Matrix, or rows of integers of one length): a Matrix of len(rows) x digest."""
        f, be = self.field, self.field.backend
        if digest not in (1, 2):
            raise GstarkError(f'HadesHash: a digest of 1 or 2 elements, not {digest}')
        if not isinstance(rows, Matrix):
            rows = [list(r) for r in rows]
            if any(len(r) != len(rows[0]) for r in rows):
                raise GstarkError('HadesHash: every row has the same number of inputs')
        count, arity = (rows.rowCount, rows.colCount) if isinstance(rows, Matrix) else (len(rows), len(rows[0]) if rows else 1)
        if not 0 < arity < self.width:
            raise GstarkError(f'HadesHash: {arity} inputs do not fit a state of {self.width} (1 .. {self.width - 1})')
        if not self.onDevice:
            values = rows.toValues() if isinstance(rows, Matrix) else rows
            return f.newMatrixFrom([self.hash(r)[:digest] for r in values]) if count else Matrix(be, 0, digest)
        src = rows if isinstance(rows, Matrix) or not count else f.newMatrixFrom(rows)
        out = Matrix(be, count, digest)
        if count:
            be.call('gs_hades_hash', self.handle(), C.c_void_p(src.ptr), count, arity, digest, C.c_void_p(out.ptr))
        return out


class HadesMerkleTree:
    """MerkleTree (digest=2) / MerkleTree2 (digest=1) of utils.ts over `hash`: 2n x digest elements in the heap layout, leaves at
    n .. 2n - 1, root at 1.  leaves: a device Matrix of n x digest (a Vector of n for digest=1) — then nothing goes through host integers
    —, or a list of n pairs (digest=2) / n integers (digest=1)."""

    def __init__(self, hash, leaves, digest):
        f = hash.field
        if digest not in (1, 2) or 2 * digest >= hash.width:
            raise GstarkError(f'HadesMerkleTree: nodes of {digest} elements (1 or 2): two of them do not fit a state of {hash.width} beside its capacity')
        self.hash, self.field, self.digest = hash, f, digest
        if isinstance(leaves, Vector):
            if digest != 1:
                raise GstarkError('HadesMerkleTree: a Vector holds leaves of one element (digest=1)')
            n = leaves.length
        elif isinstance(leaves, Matrix):
            if leaves.colCount != digest:
                raise GstarkError(f'HadesMerkleTree: the leaf matrix has {leaves.colCount} columns, the nodes {digest} elements')
            n = leaves.rowCount
        else:
            try:
                leaves = [[int(v)] for v in leaves] if digest == 1 else [[int(v) for v in leaf] for leaf in leaves]
            except TypeError:
                leaves = [[]]
            if any(len(leaf) != digest for leaf in leaves):
                raise GstarkError(f'HadesMerkleTree: every leaf has {digest} elements')
            n = len(leaves)
        if n < 2 or n & (n - 1):
            raise GstarkError(f'HadesMerkleTree: {n} leaves: the number of leaves is a power of two, at least 2')
        self.leafCount, self.depth = n, n.bit_length() - 1
        self._host = self._device = None
        if hash.onDevice:
            src = leaves if isinstance(leaves, (Matrix, Vector)) else f.newMatrixFrom(leaves)
            self._device = Matrix(f.backend, 2 * n, digest)
            f.backend.call('gs_hades_merkle', hash.handle(), C.c_void_p(src.ptr), n, digest, C.c_void_p(self._device.ptr))
        else:
            if isinstance(leaves, Vector):
                leaves = [[v] for v in leaves.toValues()]
            elif isinstance(leaves, Matrix):
                leaves = leaves.toValues()
            nodes = [[0] * digest] * n + [[v % f.modulus for v in leaf] for leaf in leaves]
            for i in range(n - 1, 0, -1):
                nodes[i] = hash.hash(nodes[2 * i] + nodes[2 * i + 1])[:digest]
            self._host = nodes

    def _shape(self, node):                  # a node as the reference's classes hold it: a pair, or one integer
        return node[0] if self.digest == 1 else tuple(node)

    @property
    def deviceNodes(self):
        """the 2n x digest Matrix of the tree on the device (None on a library without the entry points)"""
        return self._device

    @property
    def nodes(self):
        """every node on the host, as the reference's `nodes`: index 0 is unused (None)"""
        rows = self._host if self._device is None else self._device.toValues()
        return [None] + [self._shape(r) for r in rows[1:]]

    @property
    def root(self):
        return self._shape(self._host[1] if self._device is None else self._device.row(1).toValues())

    def prove(self, index):
        return self.proveMany([index])[0]

    def proveMany(self, indexes):
        """prove(index) for every index (repeats allowed): per path the leaf, then its siblings bottom-up.  One launch and one read-back."""
        indexes = [int(i) for i in indexes]
        n, d, per = self.leafCount, self.digest, self.depth + 1
        if self._device is None:
            if any(not 0 <= i < n for i in indexes):
                raise GstarkError(f'HadesMerkleTree: an index is outside of the {n} leaves')
            return [[self._shape(self._host[n + i])] + [self._shape(self._host[((n + i) >> l) ^ 1]) for l in range(self.depth)] for i in indexes]
        if any(i < 0 for i in indexes):
            raise GstarkError(f'HadesMerkleTree: an index is outside of the {n} leaves')
        if not indexes:
            return []
        f = self.field
        out = Matrix(f.backend, len(indexes) * per, d)
        f.backend.call('gs_hades_merkle_paths', C.c_void_p(self._device.ptr), n, d, (C.c_uint64 * len(indexes))(*indexes), len(indexes), C.c_void_p(out.ptr))
        rows = out.toValues()
        return [[self._shape(r) for r in rows[k * per:(k + 1) * per]] for k in range(len(indexes))]

    @staticmethod
    def verify(root, index, proof, hash):
        """utils.ts:151-166 / :194-209 — the shape of the nodes (pairs or single integers) is the proof's"""
        single = isinstance(proof[0], int)
        take = (lambda v: v[0]) if single else (lambda v: tuple(v[:2]))
        listed = (lambda v: [v]) if single else list
        index += 1 << (len(proof) - 1)
        v = proof[0]
        for sibling in proof[1:]:
            v = take(hash(listed(sibling) + listed(v))) if index & 1 else take(hash(listed(v) + listed(sibling)))
            index >>= 1
        return (root if single else tuple(root)) == v
