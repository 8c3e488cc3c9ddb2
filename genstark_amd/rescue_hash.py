"""Rescue hashes and Rescue Merkle trees computed on the device (include/gstark_rescue.h, csrc/rescue.hip), and the Merkle path
statement over them.

`RescueHash` is the `Rescue` class of the reference's examples/rescue/utils.ts:19-228, `hash2` its `makeHashFunction` (:11-15),
`RescueMerkleTree` its `MerkleTree` (:232-273): the same values in the same orders.  `sponge`, `modifiedSponge` and `hash2` are host
integer arithmetic like the example's; `hashMany`, the tree and its paths run on the context's stream (a tree: one launch per level),
with one read-back for any number of paths.  `rescue_merkle_proof_air` is the RescueMP script of examples/rescue/merkleProof.ts:51-146 as
a GenericAir.  What is not Rescue's own is field_tree.py, the host fallback on a library without the entry points included."""
import ctypes as C

from . import rescue as _params
from ._abi import GstarkError
from .air_generic import GenericAir, mat_vec
from .field import Matrix, Vector
from .field_tree import DeviceParameters, FieldMerkleTree, verify_path

STEPS_PER_HASH = 32


class RescueHash(DeviceParameters):
    """new Rescue(field, alpha, invAlpha, registers, rounds, mds, constants) — utils.ts:33.  inv_alpha may be negative, as in the
    examples: x^inv_alpha is then (1/x)^|inv_alpha|, which is x^(p - 1 - |inv_alpha|) for every x, 0 included (0 -> 0).  constants:
    width initial, width x width matrix and width additive key constants, flat (splitConstants, :204-227)."""
    _who, _family = 'RescueHash', 'rescue'

    def __init__(self, field, alpha, inv_alpha, width, rounds, mds, constants):
        alpha, inv_alpha, width, rounds = int(alpha), int(inv_alpha), int(width), int(rounds)
        p = field.modulus
        if not 2 <= width <= 8:
            raise GstarkError(f'RescueHash: a state of {width} elements is outside 2 .. 8')
        if rounds < 1:
            raise GstarkError(f'RescueHash: {rounds} rounds (at least 1)')
        if not 2 <= alpha < 1 << 64:
            raise GstarkError(f'RescueHash: alpha {alpha} is outside 2 .. 2^64 - 1')
        exponent = inv_alpha if inv_alpha > 0 else p - 1 + inv_alpha
        if not 1 <= exponent < p - 1:
            raise GstarkError('RescueHash: the inverse exponent is outside 1 .. p - 2')
        try:
            m = [[int(v) % p for v in row] for row in mds]
            c = [int(v) % p for v in constants]
        except TypeError:
            m, c = [], []
        if len(m) != width or any(len(row) != width for row in m):
            raise GstarkError(f'RescueHash: the matrix has {width} rows of {width} values')
        if len(c) != width * (width + 2):
            raise GstarkError(f'RescueHash: {width * (width + 2)} key constants are needed ({width} initial, {width} x {width}, {width} additive)')
        self.field, self.alpha, self.invAlpha, self.invExponent, self.width, self.rounds, self.mds = field, alpha, inv_alpha, exponent, width, rounds, m
        self.iConstants, self.cConstants = c[:width], c[width + width * width:]
        self.cMatrix = [c[width + i * width:width + (i + 1) * width] for i in range(width)]
        self._keys, self._maxArity = None, width

    # ---- host integers
    def _mmul(self, m, v):
        p = self.field.modulus
        return [sum(a * b for a, b in zip(row, v)) % p for row in m]

    def _half(self, state, exponent, key):
        p = self.field.modulus
        return [(a + b) % p for a, b in zip(self._mmul(self.mds, [pow(x, exponent, p) for x in state]), key)]

    def unrollConstants(self):
        """utils.ts:128-159: the 2 * rounds + 3 key rows"""
        p = self.field.modulus
        vadd = lambda a, b: [(x + y) % p for x, y in zip(a, b)]
        state, injection = list(self.iConstants), self.iConstants
        result = [list(state)]
        for _ in range(self.rounds + 1):
            for exponent in (self.invExponent, self.alpha):
                injection = vadd(self._mmul(self.cMatrix, injection), self.cConstants)
                state = self._half(state, exponent, injection)
                result.append(list(state))
        return result

    @property
    def keys(self):
        if self._keys is None:
            self._keys = self.unrollConstants()
        return self._keys

    def groupConstants(self, keys=None):
        """utils.ts:161-180: (initialConstants, roundConstants) — 2 * width columns of `rounds` values"""
        keys = self.keys if keys is None else keys
        n = self.width
        rc = [[0] * self.rounds for _ in range(2 * n)]
        for i in range(self.rounds):
            for j in range(n):
                rc[j][i] = keys[2 + 2 * i][j]
                rc[n + j][i] = keys[3 + 2 * i][j]
        return list(keys[0]) + list(keys[1]), rc

    def _state(self, inputs):
        inputs = [int(v) % self.field.modulus for v in inputs]
        if not 0 < len(inputs) <= self.width:
            raise GstarkError(f'RescueHash: {len(inputs)} inputs do not fit a state of {self.width} (1 .. {self.width})')
        return inputs + [0] * (self.width - len(inputs))

    def sponge(self, inputs, keys=None):
        """utils.ts:49-88: (hash, trace) — the hash has as many elements as there were inputs"""
        keys = self.keys if keys is None else keys
        state = self._state(inputs)
        trace = [list(state)]
        state = [(a + b) % self.field.modulus for a, b in zip(state, keys[0])]
        trace.append(list(state))
        for r in range(self.rounds):
            for exponent, key in ((self.invExponent, keys[2 * r + 1]), (self.alpha, keys[2 * r + 2])):
                state = self._half(state, exponent, key)
                trace.append(list(state))
        return state[:len(inputs)], trace

    def modifiedSponge(self, inputs, keys=None):
        """utils.ts:90-124: (hash, trace)"""
        keys = self.keys if keys is None else keys
        state = self._state(inputs)
        trace = [list(state)]
        for r in range(self.rounds - 1):
            for exponent, key in ((self.alpha, keys[2 * r + 2]), (self.invExponent, keys[2 * r + 3])):
                state = self._half(state, exponent, key)
                trace.append(list(state))
        return state[:len(inputs)], trace

    def hash2(self, v1, v2):
        """makeHashFunction (utils.ts:11-15)"""
        return self.modifiedSponge([v1, v2] + [0] * (self.width - 2))[0][0]

    # ---- device (field_tree.DeviceParameters)
    def _create(self, out):
        f = self.field
        f.backend.call('gs_rescue_create', self.width, self.rounds, self.alpha, f.le(self.invExponent), b''.join(f.le(v) for row in self.mds for v in row),
                       b''.join(f.le(v) for row in self.keys for v in row), out)

    def hashMany(self, rows, digest=1, modified=True, form=0):
        """One permutation per row of `rows` (a device Matrix, or rows of integers of one length): a Matrix of len(rows) x digest, the
        leading elements of the final states.  form: 0 the library chooses, 1 a thread per permutation, 2 a lane per state element."""
        def check():
            if form not in (0, 1, 2):
                raise GstarkError(f'RescueHash: form is 0, 1 or 2, not {form}')
        run = self.modifiedSponge if modified else self.sponge
        return self._hashRows(rows, digest, lambda r: run(r)[1][-1], 1 if modified else 0, form, check=check)

    def _permutation(self, modified):
        """what hashMany(modified=..) applies to a full-width row: the whole last state"""
        run = self.modifiedSponge if modified else self.sponge
        return lambda state: run(state)[1][-1]

    def absorb(self, inputs, digest=1, rate=None, modified=True):
        """The digest of a record of any length (1 .. 2^16 values) on host integers: state = zeros with state[rate] = len(inputs); per
        block of `rate` inputs, the block is ADDED to state[0 .. rate) and the state permuted (modifiedSponge of the full state, or
        sponge with modified=False); the first `digest` elements of the last state.  rate defaults to width - 1 up to a state of 3 and
        to width - 2 above.  On purpose this is NOT the sponge of short inputs: the length in the capacity keeps [a] and [a, 0] apart."""
        return self._absorbHost(list(inputs), digest, self._absorbShape(digest, rate), self._permutation(modified))

    def absorbMany(self, rows, digest=1, rate=None, columns=False, modified=True):
        """absorb(row) for every row, one launch (gs_rescue_absorb, include/gstark_absorb.h): a Matrix of count x digest.  rows: a device
        Matrix of count x L, or lists of one length; with columns=True the register-major L x count Matrix of a trace, or a list of L
        Vectors of one length: record k is column k.  Like absorb, not hashMany of short rows."""
        return self._absorbRows(rows, digest, rate, columns, self._permutation(modified), 1 if modified else 0)


class RescueMerkleTree(FieldMerkleTree):
    """MerkleTree of utils.ts:232-273 over hash.hash2: 2n elements in the heap layout, leaves at n .. 2n - 1, root at 1.  leaves: a device
    Vector of n elements — then nothing goes through host integers —, or n integers.  deviceNodes is the Vector of 2n nodes."""
    _who = 'RescueMerkleTree'
    _unreadable = []                         # leaves that are no integers are no leaves: the message of the leaf count

    def __init__(self, hash, leaves):
        if hash.width < 3:
            raise GstarkError(f'RescueMerkleTree: two nodes do not fit a state of {hash.width} beside its capacity (width 3 .. 8)')
        super().__init__(hash, () if isinstance(leaves, Matrix) else leaves, 1)      # a Matrix is no leaves here: the message of the leaf count

    def _newNodes(self, count):
        return Vector(self.field.backend, count)

    def _buildOnDevice(self, src, out):
        self.field.backend.call('gs_rescue_merkle', self.hash.handle(), C.c_void_p(src.ptr), self.leafCount, C.c_void_p(out.ptr))

    _updateEntry = 'gs_rescue_merkle_update'

    def _updateOnDevice(self, indexes, count, src, before, roots):
        self.field.backend.call(self._updateEntry, self.hash.handle(), C.c_void_p(self.deviceNodes.ptr), self.leafCount, indexes, C.c_void_p(src.ptr), count,
                                C.c_void_p(before.ptr), C.c_void_p(roots.ptr))

    def _node(self, left, right):
        return [self.hash.hash2(left[0], right[0])]

    _pathRootsEntry, _digest = 'gs_rescue_merkle_path_roots', 1

    @classmethod
    def _checkDigest(cls, hash, digest):
        if hash.width < 3:
            raise GstarkError(f'RescueMerkleTree: two nodes do not fit a state of {hash.width} beside its capacity (width 3 .. 8)')
        if digest != 1:
            raise GstarkError(f'RescueMerkleTree: nodes of one element, not {digest}')

    @classmethod
    def _pathRootsOnDevice(cls, hash, paths, depth, digest, indexes, leaves, count, roots):
        hash.field.backend.call(cls._pathRootsEntry, hash.handle(), paths, depth, indexes, leaves, count, roots)

    @staticmethod
    def verify(root, index, proof, hash2):
        """utils.ts:257-272"""
        return verify_path(root, index, proof, hash2)


def rescue4x128(field):
    """the parameter set of examples/rescue/hash4x128.ts and merkleProof.ts: x^3, 4 registers, 32 rounds"""
    return RescueHash(field, _params.ALPHA, -_params.INV_ALPHA, 4, STEPS_PER_HASH, _params.MDS, _params.SEED_CONSTANTS)


def rescue2x64(field):
    """the parameter set of examples/rescue/hash2x64.ts: x^3, 2 registers, 32 rounds, over 2^64 - 21 * 2^30 + 1"""
    if field.modulus != _params.MODULUS_2X64:
        raise GstarkError('Rescue 2x64 is defined over 2^64 - 21*2^30 + 1')
    return RescueHash(field, _params.ALPHA, -_params.INV_ALPHA_2X64, 2, STEPS_PER_HASH, _params.MDS_2X64, _params.SEED_CONSTANTS_2X64)


# ---- the Merkle path statement (merkleProof.ts:51-146) ----------------------------------------------------------------------------
def _held(values, steps, total):
    """the column of an input held `steps` steps and rotated by one: values[j] on steps j * steps - 1 .. (j + 1) * steps - 2, so that
    the transition INTO the first row of a level already sees that level's value"""
    return [values[((i + 1) // steps) % len(values)] for i in range(total)]


def rescue_merkle_proof_air(field, index_bits, extensionFactor=16):
    """RescueMP for ONE authentication path of depth len(index_bits) (a power of two).  index_bits is the PUBLIC input register, already
    shifted as merkleProof.ts:162-164 does ([0] + the index's bits, least significant first, without the last).  Eight trace registers:
    0 .. 3 run hash2(h, node), 4 .. 7 hash2(node, h), 32 steps per level; prove(assertions, inputs, first) takes what
    rescue_merkle_inputs() returns.  The root is in register 0 at step 32 * depth - 1 — in register 4 when the top bit of the index is 1.

    Static registers: k[0] index bit, k[1] leaf mask (1 on the last step of the trace), k[2] node mask (1 on the last step of every
    level: the next row is an init row), k[3 .. 10] the round constants (groupConstants), then the secret registers leaf and node.  A
    hash step enforces mds # r^alpha + k1 = (inv_mds # (n - k2))^alpha (:134-139); an init row enforces n = [h, node, 0, 0, node, h, 0,
    0] with h = bit ? r4 : r0 (:128-129), the first of all n = [leaf, node, 0, 0, node, leaf, 0, 0] (:123)."""
    if field.modulus != 2**128 - 9 * 2**32 + 1:
        raise GstarkError('RescueMP is defined over 2^128 - 9*2^32 + 1')
    h = rescue4x128(field)
    depth = len(index_bits)
    total = STEPS_PER_HASH * depth
    rc = h.groupConstants()[1]
    mask = lambda steps: [0] * (steps - 1) + [1]
    public = [_held([b % field.modulus for b in index_bits], STEPS_PER_HASH, total), mask(total), mask(STEPS_PER_HASH)] + rc
    npub = len(public)
    mds, inv_mds, alpha, inv = _params.MDS, _params.INV_MDS, h.alpha, h.invExponent
    add = lambda a, b: [x + y for x, y in zip(a, b)]

    def init_row(r, k):
        bit, leaf_mask, (leaf, node) = k[0], k[1], k[npub:npub + 2]
        v = leaf * leaf_mask + (r[4] * bit + r[0] * (1 - bit)) * (1 - leaf_mask)
        return [v, node, 0, 0, node, v, 0, 0]

    def forward(r, k):                            # mds # r^alpha + roundConstants[0..3], both halves
        return add(mat_vec(mds, [x ** alpha for x in r[0:4]]), k[3:7]) + add(mat_vec(mds, [x ** alpha for x in r[4:8]]), k[3:7])

    def transition(r, k):
        s = forward(r, k)
        step = add(mat_vec(mds, [x ** inv for x in s[0:4]]), k[7:11]) + add(mat_vec(mds, [x ** inv for x in s[4:8]]), k[7:11])
        return [a * k[2] + b * (1 - k[2]) for a, b in zip(init_row(r, k), step)]

    def evaluation(r, n, k):
        s = forward(r, k)
        back = [x ** alpha for x in mat_vec(inv_mds, [a - b for a, b in zip(n[0:4], k[7:11])])] + \
               [x ** alpha for x in mat_vec(inv_mds, [a - b for a, b in zip(n[4:8], k[7:11])])]
        return [(x - a) * k[2] + (b - c) * (1 - k[2]) for x, a, b, c in zip(n, init_row(r, k), s, back)]

    return GenericAir(total, 8, [4] * 8, public, transition, evaluation, lambda seed: list(seed), extensionFactor, field, secretRegisters=2)


def rescue_merkle_inputs(field, leaf, nodes):
    """The secret columns of RescueMP and its first row (merkleProof.ts:93) from an authentication path: leaf, and nodes bottom-up
    (tree.prove(index)[0] and [1:])."""
    total = STEPS_PER_HASH * len(nodes)
    p = field.modulus
    cols = [[leaf % p] * total, _held([v % p for v in nodes], STEPS_PER_HASH, total)]
    return cols, [v % p for v in (leaf, nodes[0], 0, 0, nodes[0], leaf, 0, 0)]
