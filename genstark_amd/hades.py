"""Poseidon hashes and Poseidon Merkle trees computed on the device (include/gstark_hades.h, csrc/hades.hip).

`HadesHash` is `createHash` of the reference's examples/poseidon/utils.ts:19-49, `HadesMerkleTree` its `MerkleTree` (digest=2: nodes of
two elements, :126-167) and `MerkleTree2` (digest=1, :169-210): the same values in the same orders.  `hash(inputs)` is host integer
arithmetic like the example's function; `hashMany`, the tree and its paths are one launch each on the context's stream (a tree: one per
wide level and one for the top), with one read-back for any number of paths.  What is not Poseidon's own is field_tree.py, the host
fallback on a library without the entry points included."""
import ctypes as C

from ._abi import GstarkError
from .field import Matrix
from .field_tree import DeviceParameters, FieldMerkleTree, verify_path
from .poseidon import mds_matrix, round_constants as derived_round_constants


class HadesHash(DeviceParameters):
    """createHash(field, exp, rf, rp, stateWidth, rc?) — utils.ts:19.  round_constants: (rf + rp) rows of `width` values; mds: `width`
    rows of `width` values; both derived as the example derives them (sha256 over 'Hades<c>', the Cauchy matrix of 'HadesMDSx<i>' and
    'HadesMDSy<j>') when omitted."""
    _who, _family = 'HadesHash', 'hades'

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
        self.roundConstants, self.mds, self._maxArity = rc, m, width - 1

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

    # ---- device (field_tree.DeviceParameters)
    def _create(self, out):
        f = self.field
        f.backend.call('gs_hades_create', self.width, self.fullRounds, self.partialRounds, self.alpha,
                       b''.join(f.le(v) for row in self.roundConstants for v in row), b''.join(f.le(v) for row in self.mds for v in row), out)

    def hashMany(self, rows, digest=2):
        """One permutation per row of `rows` (a device Matrix, or rows of integers of one length): a Matrix of len(rows) x digest."""
        return self._hashRows(rows, digest, self.hash)

    def absorb(self, inputs, digest=2, rate=None):
        """The digest of a record of any length (1 .. 2^16 values) on host integers: state = zeros with state[rate] = len(inputs); per
        block of `rate` inputs, the block is ADDED to state[0 .. rate) and the state permuted; the first `digest` elements of the last
        state.  rate defaults to width - 1 up to a state of 3 and to width - 2 above.  On purpose this is NOT hash(inputs) for short
        inputs: the length in the capacity keeps [a] and [a, 0] apart."""
        return self._absorbHost(list(inputs), digest, self._absorbShape(digest, rate), self.permute)

    def absorbMany(self, rows, digest=2, rate=None, columns=False):
        """absorb(row) for every row, one launch (gs_hades_absorb, include/gstark_absorb.h): a Matrix of count x digest.  rows: a device
        Matrix of count x L, or lists of one length; with columns=True the register-major L x count Matrix of a trace, or a list of L
        Vectors of one length (put side by side as evalPolysAtPoints does): record k is column k.  Like absorb, not hashMany of short rows."""
        return self._absorbRows(rows, digest, rate, columns, self.permute)


class HadesMerkleTree(FieldMerkleTree):
    """MerkleTree (digest=2) / MerkleTree2 (digest=1) of utils.ts over `hash`: 2n x digest elements in the heap layout, leaves at
    n .. 2n - 1, root at 1.  leaves: a device Matrix of n x digest (a Vector of n for digest=1) — then nothing goes through host integers
    —, or a list of n pairs (digest=2) / n integers (digest=1).  deviceNodes is the 2n x digest Matrix."""
    _who = 'HadesMerkleTree'

    def __init__(self, hash, leaves, digest):
        if digest not in (1, 2) or 2 * digest >= hash.width:
            raise GstarkError(f'HadesMerkleTree: nodes of {digest} elements (1 or 2): two of them do not fit a state of {hash.width} beside its capacity')
        super().__init__(hash, leaves, digest)

    def _newNodes(self, count):
        return Matrix(self.field.backend, count, self.digest)

    def _buildOnDevice(self, src, out):
        self.field.backend.call('gs_hades_merkle', self.hash.handle(), C.c_void_p(src.ptr), self.leafCount, self.digest, C.c_void_p(out.ptr))

    _updateEntry = 'gs_hades_merkle_update'

    def _updateOnDevice(self, indexes, count, src, before, roots):
        self.field.backend.call(self._updateEntry, self.hash.handle(), C.c_void_p(self.deviceNodes.ptr), self.leafCount, self.digest, indexes, C.c_void_p(src.ptr), count,
                                C.c_void_p(before.ptr), C.c_void_p(roots.ptr))

    def _node(self, left, right):
        return self.hash.hash(left + right)[:self.digest]

    _pathRootsEntry = 'gs_hades_merkle_path_roots'

    @classmethod
    def _checkDigest(cls, hash, digest):
        if digest not in (1, 2) or 2 * digest >= hash.width:
            raise GstarkError(f'HadesMerkleTree: nodes of {digest} elements (1 or 2): two of them do not fit a state of {hash.width} beside its capacity')

    @classmethod
    def _pathRootsOnDevice(cls, hash, paths, depth, digest, indexes, leaves, count, roots):
        hash.field.backend.call(cls._pathRootsEntry, hash.handle(), paths, depth, digest, indexes, leaves, count, roots)

    @staticmethod
    def verify(root, index, proof, hash):
        """utils.ts:151-166 / :194-209 — the shape of the nodes (pairs or single integers) is the proof's"""
        if isinstance(proof[0], int):
            return verify_path(root, index, proof, lambda left, right: hash([left, right])[0])
        return verify_path(tuple(root), index, proof, lambda left, right: tuple(hash(list(left) + list(right))[:2]))
