"""What the algebraic hash families (hades.py, rescue_hash.py) share above the C ABI, as csrc/sponge_common.h is below it: a parameter
set with a device handle, and the heap-layout Merkle tree of nodes of `digest` field elements with its authentication paths.  On a
backend whose library lacks the entry points (the tests' double) everything is computed on host integers and gives the same values."""
import collections
import ctypes as C
import types

from ._abi import GstarkError
from .field import Matrix, Vector


class DeviceParameters:
    """A parameter set whose constants live on the field's context once they are needed.  A subclass names itself (`_who`, the front of
    every message) and its entry points (`_family`: gs_<family>_*), and has `_maxArity` and `_create(out)` (the upload)."""
    _who = _family = _handle = None

    @property
    def onDevice(self):
        be = getattr(self.field, 'backend', None)              # a HostField has none
        return be is not None and hasattr(be.lib, f'gs_{self._family}_hash')

    def handle(self):
        """the gs_<family> of this parameter set on the field's context: constants uploaded once, on first use"""
        if self._handle is None:
            h = C.c_void_p()
            self._create(C.byref(h))
            self._handle = h
        return self._handle

    def __del__(self):
        try:
            if self._handle is not None and self.field.backend.ctx:
                getattr(self.field.backend.lib, f'gs_{self._family}_destroy')(self.field.backend.ctx, self._handle)
            self._handle = None
        except Exception:
            pass

    def _hashRows(self, rows, digest, host_row, *options, check=None):
        """hashMany: host_row(row) is the final state on host integers, options what gs_<family>_hash takes between `digest` and `out`,
        check() the subclass's own refusals (their place is after the digest's)"""
        f, be = self.field, self.field.backend
        if digest not in (1, 2):
            raise GstarkError(f'{self._who}: a digest of 1 or 2 elements, not {digest}')
        if check:
            check()
        if not isinstance(rows, Matrix):
            rows = [list(r) for r in rows]
            if any(len(r) != len(rows[0]) for r in rows):
                raise GstarkError(f'{self._who}: every row has the same number of inputs')
        count, arity = (rows.rowCount, rows.colCount) if isinstance(rows, Matrix) else (len(rows), len(rows[0]) if rows else 1)
        if not 0 < arity <= self._maxArity:
            raise GstarkError(f'{self._who}: {arity} inputs do not fit a state of {self.width} (1 .. {self._maxArity})')
        if not self.onDevice:
            values = rows.toValues() if isinstance(rows, Matrix) else rows
            return f.newMatrixFrom([host_row(r)[:digest] for r in values]) if count else Matrix(be, 0, digest)
        src = rows if isinstance(rows, Matrix) or not count else f.newMatrixFrom(rows)
        out = Matrix(be, count, digest)
        if count:
            be.call(f'gs_{self._family}_hash', self.handle(), C.c_void_p(src.ptr), count, arity, digest, *options, C.c_void_p(out.ptr))
        return out


    # ---- records of any length (include/gstark_absorb.h) ---------------------------------------------------------------------------
    def _absorbShape(self, digest, rate):
        """the rate (default: width - 1 up to a state of 3, width - 2 above) after the refusals that need no input"""
        rate = (self.width - 1 if self.width <= 3 else self.width - 2) if rate is None else int(rate)
        if not 1 <= rate < self.width:
            raise GstarkError(f'{self._who}: absorb: a rate of {rate} does not leave a capacity in a state of {self.width} (1 .. {self.width - 1})')
        if digest not in (1, 2) or digest > rate:
            raise GstarkError(f'{self._who}: absorb: a digest of 1 or 2 elements and at most the rate ({rate}), not {digest}')
        return rate

    def _absorbLength(self, length):
        if not 1 <= length <= ABSORB_MAX_LENGTH:
            raise GstarkError(f'{self._who}: absorb: a record of {length} elements (1 .. {ABSORB_MAX_LENGTH})')

    def _absorbHost(self, inputs, digest, rate, permute):
        """the definition on host integers: the length in the first capacity element, `rate` inputs added per permutation"""
        p = self.field.modulus
        inputs = [int(v) % p for v in inputs]
        self._absorbLength(len(inputs))
        state = [0] * self.width
        state[rate] = len(inputs) % p
        for at in range(0, len(inputs), rate):
            for j, v in enumerate(inputs[at:at + rate]):
                state[j] = (state[j] + v) % p
            state = permute(state)
        return state[:digest]

    def _absorbRows(self, rows, digest, rate, columns, permute, *options):
        """absorbMany: `options` is what gs_<family>_absorb takes between `digest` and `out`.  rows: a device Matrix (count x L, or
        L x count with columns=True), equal-length lists of integers, or with columns=True a list of L Vectors of one length."""
        f = self.field
        rate = self._absorbShape(digest, rate)
        if not isinstance(rows, Matrix):
            rows = list(rows)
            if columns and rows and all(isinstance(r, Vector) for r in rows):
                if any(r.length != rows[0].length for r in rows):
                    raise GstarkError(f'{self._who}: absorb: every column has the same number of elements')
                rows = f.newMatrixFromVectors(rows) if rows[0].length else [[] for _ in rows]
            else:
                rows = [list(r) for r in rows]
                if any(len(r) != len(rows[0]) for r in rows):
                    raise GstarkError(f'{self._who}: absorb: every {"column" if columns else "row"} has the same number of elements')
        if isinstance(rows, Matrix):
            outer, inner = rows.rowCount, rows.colCount
        else:
            outer, inner = len(rows), len(rows[0]) if rows else 0
            if not outer and not columns:
                return Matrix(f.backend, 0, digest)
        count, length = (inner, outer) if columns else (outer, inner)
        self._absorbLength(length)
        if not count:
            return Matrix(f.backend, 0, digest)
        entry = f'gs_{self._family}_absorb'
        if not self.onDevice:
            values = rows.toValues() if isinstance(rows, Matrix) else rows
            if columns:
                values = [list(r) for r in zip(*values)]
            return f.newMatrixFrom([self._absorbHost(r, digest, rate, permute) for r in values])
        if not hasattr(f.backend.lib, entry):                                # a hash that lives on the device absorbs there: no quiet host path
            raise GstarkError(f'{self._who}: the library has no {entry} (include/gstark_absorb.h)')
        src = rows if isinstance(rows, Matrix) else f.newMatrixFrom(rows)
        out = Matrix(f.backend, count, digest)
        row_stride, elem_stride = (1, count) if columns else (length, 1)
        f.backend.call(entry, self.handle(), C.c_void_p(src.ptr), count, length, row_stride, elem_stride, rate, digest, *options, C.c_void_p(out.ptr))
        return out


ABSORB_MAX_LENGTH = 1 << 16                  # the longest record of absorb / absorbMany


def path_root(index, proof, node):
    """the root a path (the leaf, then its siblings bottom-up) implies: node(left, right) level by level, sides by the index bits"""
    index += 1 << (len(proof) - 1)
    v = proof[0]
    for sibling in proof[1:]:
        v = node(sibling, v) if index & 1 else node(v, sibling)
        index >>= 1
    return v


def verify_path(root, index, proof, node):
    """a path against a root"""
    return root == path_root(index, proof, node)


TreeUpdate = collections.namedtuple('TreeUpdate', 'before root')     # one record of FieldMerkleTree.updateMany


class FieldMerkleTree:
    """2n nodes of `digest` elements in the heap layout: leaves at n .. 2n - 1, root at 1, node 0 unused.  leaves: a device Matrix of
    n x digest (a Vector of n for digest=1) — then nothing goes through host integers —, or n host values.  A subclass names itself
    (`_who`) and has `_newNodes(count)` (the kind of array deviceNodes is), `_buildOnDevice(src, out)` and `_node(left, right)` on host
    integers.  The path gather is the family-neutral one (gs_hades_merkle_paths reads nothing but the node array)."""
    _unreadable = [[]]                       # what leaves that cannot be read as host values count as
    _digest = None                           # the size of a node where the family fixes it (pathRoots over device paths)

    def __init__(self, hash, leaves, digest):
        f = hash.field
        self.hash, self.field, self.digest = hash, f, digest
        leaves, n = self._readLeaves(leaves)
        if n < 2 or n & (n - 1):
            raise GstarkError(f'{self._who}: {n} leaves: the number of leaves is a power of two, at least 2')
        self.leafCount, self.depth = n, n.bit_length() - 1
        self._host = self.deviceNodes = None      # deviceNodes: the 2n nodes on the device (None on a library without the entry points)
        if hash.onDevice:
            src = leaves if isinstance(leaves, (Matrix, Vector)) else f.newMatrixFrom(leaves)
            self.deviceNodes = self._newNodes(2 * n)
            self._buildOnDevice(src, self.deviceNodes)
        else:
            if isinstance(leaves, (Matrix, Vector)):
                leaves = _rows(leaves)
            nodes = [[0] * digest] * n + leaves
            for i in range(n - 1, 0, -1):
                nodes[i] = self._node(nodes[2 * i], nodes[2 * i + 1])
            self._host = nodes

    def _readLeaves(self, leaves):
        """(leaves, how many): a device Vector or Matrix as it is, host values as rows of `digest` integers — the constructor's leaves
        and updateMany's"""
        f, digest = self.field, self.digest
        if isinstance(leaves, Vector):
            if digest != 1:
                raise GstarkError(f'{self._who}: a Vector holds leaves of one element (digest=1)')
            return leaves, leaves.length
        if isinstance(leaves, Matrix):
            if leaves.colCount != digest:
                raise GstarkError(f'{self._who}: the leaf matrix has {leaves.colCount} columns, the nodes {digest} elements')
            return leaves, leaves.rowCount
        try:
            leaves = [[int(v) % f.modulus] for v in leaves] if digest == 1 else [[int(v) % f.modulus for v in leaf] for leaf in leaves]
        except TypeError:
            leaves = self._unreadable
        if any(len(leaf) != digest for leaf in leaves):
            raise GstarkError(f'{self._who}: every leaf has {digest} elements')
        return leaves, len(leaves)

    def _shape(self, node):                  # a node as the reference's classes hold it: a pair, or one integer
        return node[0] if self.digest == 1 else tuple(node)

    @property
    def nodes(self):
        """every node on the host, as the reference's `nodes`: index 0 is unused (None)"""
        rows = self._host if self.deviceNodes is None else _rows(self.deviceNodes)
        return [None] + [self._shape(r) for r in rows[1:]]

    @property
    def root(self):
        d = self.deviceNodes
        return self._shape(self._host[1] if d is None else [d.getValue(1)] if isinstance(d, Vector) else d.row(1).toValues())

    def prove(self, index):
        return self.proveMany([index])[0]

    def proveMany(self, indexes):
        """prove(index) for every index (repeats allowed): per path the leaf, then its siblings bottom-up.  One launch and one read-back."""
        indexes = [int(i) for i in indexes]
        n, d, per = self.leafCount, self.digest, self.depth + 1
        if self.deviceNodes is None:
            if any(not 0 <= i < n for i in indexes):
                raise GstarkError(f'{self._who}: an index is outside of the {n} leaves')
            return [[self._shape(self._host[n + i])] + [self._shape(self._host[((n + i) >> l) ^ 1]) for l in range(self.depth)] for i in indexes]
        if any(i < 0 for i in indexes):
            raise GstarkError(f'{self._who}: an index is outside of the {n} leaves')
        if not indexes:
            return []
        out = self._newNodes(len(indexes) * per)
        self.field.backend.call('gs_hades_merkle_paths', C.c_void_p(self.deviceNodes.ptr), n, d, (C.c_uint64 * len(indexes))(*indexes), len(indexes), C.c_void_p(out.ptr))
        rows = _rows(out)
        return [[self._shape(r) for r in rows[k * per:(k + 1) * per]] for k in range(len(indexes))]

    def update(self, index, leaf):
        """updateMany([index], [leaf])[0]"""
        return self.updateMany([index], [leaf])[0]

    def updateMany(self, indexes, leaves):
        """Sets leaf indexes[j] to leaves[j] for j = 0, 1, .. in that order (repeated indexes allowed) and returns one TreeUpdate per
        update: `before`, what prove(indexes[j]) would have returned just before update j (the old leaf, then its siblings bottom-up),
        and `root`, the root just after it — the witness of the reference's ComputeMerkleUpdate, whose old root is the update before's
        `root` (this tree's root at the call for the first).  Afterwards root, nodes, prove and proveMany see the last tree.  On the
        device: one upload of the leaves, a hash launch per level over the whole batch, one read-back of all witnesses and roots."""
        indexes = [int(i) for i in indexes]
        leaves, count = self._readLeaves(leaves)
        if leaves is self._unreadable:
            raise GstarkError(f'{self._who}: every leaf has {self.digest} elements')
        n, per = self.leafCount, self.depth + 1
        if count != len(indexes):
            raise GstarkError(f'{self._who}: {len(indexes)} indexes and {count} leaves: an update is one of each')
        if any(not 0 <= i < n for i in indexes):
            raise GstarkError(f'{self._who}: an index is outside of the {n} leaves')
        if not count:
            return []
        if self.deviceNodes is None:
            if not isinstance(leaves, list):
                leaves = _rows(leaves)
            nodes, out = self._host, []
            for i, leaf in zip(indexes, leaves):
                at = n + i
                before = [self._shape(nodes[at])] + [self._shape(nodes[(at >> l) ^ 1]) for l in range(self.depth)]
                nodes[at] = list(leaf)
                while at > 1:
                    at >>= 1
                    nodes[at] = self._node(nodes[2 * at], nodes[2 * at + 1])
                out.append(TreeUpdate(before, self._shape(nodes[1])))
            return out
        if not hasattr(self.field.backend.lib, self._updateEntry):       # a tree built on the device is updated there: no quiet host path
            raise GstarkError(f'{self._who}: the library has no {self._updateEntry} (include/gstark_tree_update.h)')
        src = leaves if isinstance(leaves, (Matrix, Vector)) else self.field.newMatrixFrom(leaves)
        before, roots = self._newNodes(count * per), self._newNodes(count)
        self._updateOnDevice((C.c_uint64 * count)(*indexes), count, src, before, roots)
        rows, roots = _rows(before), _rows(roots)
        return [TreeUpdate([self._shape(r) for r in rows[j * per:(j + 1) * per]], self._shape(roots[j])) for j in range(count)]

    # ---- the consuming side (include/gstark_tree_verify.h): a verifier holds a root and a hash, not a tree ------------------------
    @classmethod
    def pathRoots(cls, hash, indexes, proofs, leaves=None, digest=None):
        """The root each path implies, in the shape `root` has (an integer for nodes of one element, a tuple for two).  proofs: paths as
        prove / proveMany return them (the leaf, then its siblings bottom-up), or a device Matrix of one row of (depth + 1) * digest
        elements per path — the layout the path gather and updateMany's witnesses have on the device.  indexes[k] is the leaf index of
        path k.  leaves (a list, or a device array as in updateMany): path k starts from leaves[k] instead of its own leaf.  digest is
        that of the first path's leaf when not given.  On the device: ONE launch walks every level of every path."""
        indexes, depth, digest, paths = cls._readPaths(hash, indexes, proofs, digest)
        return cls._impliedRoots(hash, indexes, depth, digest, paths, leaves)

    @classmethod
    def verifyMany(cls, root, indexes, proofs, hash):
        """verify(root, indexes[k], proofs[k], ..) for every k: one bool per path"""
        root, digest = cls._readRoot(hash, root)
        return [r == root for r in cls.pathRoots(hash, indexes, proofs, digest=digest)]

    @classmethod
    def verifyUpdates(cls, old_root, indexes, leaves, records, hash):
        """One bool per record of updateMany(indexes, leaves) on a tree whose root was old_root: update j is valid when records[j].before
        at indexes[j] implies the root before it (old_root, then records[j - 1].root as claimed) AND the same siblings under leaves[j]
        imply records[j].root.  Two device calls in all."""
        old_root, digest = cls._readRoot(hash, old_root)
        records = list(records)
        claimed = [cls._readRoot(hash, r.root)[0] for r in records]
        indexes, depth, digest, paths = cls._readPaths(hash, indexes, [r.before for r in records], digest)
        if not indexes:
            cls._impliedRoots(hash, indexes, depth, digest, paths, leaves)       # (the refusals of leaves that are no leaves of no updates)
            return []
        if cls._walksOnDevice(hash) and not isinstance(paths, Matrix):
            paths = hash.field.newMatrixFrom([[v for node in path for v in node] for path in paths])      # one upload serves both calls
        before = cls._impliedRoots(hash, indexes, depth, digest, paths, None)
        after = cls._impliedRoots(hash, indexes, depth, digest, paths, leaves)
        return [b == was and a == now for b, was, a, now in zip(before, [old_root] + claimed[:-1], after, claimed)]

    @classmethod
    def _walksOnDevice(cls, hash):
        """False on a library without the family's entry points (the tests' double): host integers.  A hash that lives on the device
        walks its paths there: no quiet host path where only the entry of include/gstark_tree_verify.h is missing."""
        if not hash.onDevice:
            return False
        if not hasattr(hash.field.backend.lib, cls._pathRootsEntry):
            raise GstarkError(f'{cls._who}: the library has no {cls._pathRootsEntry} (include/gstark_tree_verify.h)')
        return True

    @classmethod
    def _readRoot(cls, hash, root):
        """(the root mod p in the shape `root` has, its digest)"""
        p = hash.field.modulus
        try:
            return (int(root) % p, 1) if not isinstance(root, (tuple, list)) else (tuple(int(v) % p for v in root), len(root))
        except (TypeError, ValueError):
            raise GstarkError(f'{cls._who}: a root is one integer or a tuple of integers') from None

    @classmethod
    def _readPaths(cls, hash, indexes, proofs, digest):
        """(indexes, depth, digest, paths): paths the device Matrix as it is, or per path depth + 1 rows of `digest` integers mod p"""
        p = hash.field.modulus
        indexes = [int(i) for i in indexes]
        if isinstance(proofs, Matrix):
            digest = cls._digest if digest is None else digest
            if digest is None:
                raise GstarkError(f'{cls._who}: paths on the device do not tell the size of a node: pass digest=')
            cls._checkDigest(hash, digest)
            count, depth = proofs.rowCount, proofs.colCount // digest - 1
            if proofs.colCount % digest or depth < 1:
                raise GstarkError(f'{cls._who}: a row of {proofs.colCount} elements is no leaf of {digest} with at least one sibling')
            paths = proofs
        else:
            proofs = [list(path) for path in proofs]
            count = len(proofs)
            if digest is None:
                first = proofs[0][0] if proofs and proofs[0] else 0
                digest = len(first) if isinstance(first, (tuple, list)) else 1
            cls._checkDigest(hash, digest)
            if any(len(path) != len(proofs[0]) for path in proofs):
                raise GstarkError(f'{cls._who}: the paths have unequal lengths: one call checks paths of one depth')
            depth = len(proofs[0]) - 1 if proofs else 1
            if depth < 1:
                raise GstarkError(f'{cls._who}: a path is a leaf and at least one sibling')
            try:
                paths = [[[int(node) % p] if digest == 1 else [int(v) % p for v in node] for node in path] for path in proofs]
            except TypeError:
                paths = [[[]]]
            if any(len(node) != digest for path in paths for node in path):
                raise GstarkError(f'{cls._who}: every node of a path has {digest} element{"s" if digest > 1 else ""}')
        if count != len(indexes):
            raise GstarkError(f'{cls._who}: {len(indexes)} indexes and {count} paths: a path is checked at one index')
        for i in indexes:
            if not 0 <= i < 1 << depth:
                raise GstarkError(f'{cls._who}: index {i} is outside of the {1 << depth} leaves of a path of {depth} siblings')
        return indexes, depth, digest, paths

    @classmethod
    def _impliedRoots(cls, hash, indexes, depth, digest, paths, leaves):
        f, count = hash.field, len(indexes)
        reader = types.SimpleNamespace(hash=hash, field=f, digest=digest, _who=cls._who, _unreadable=cls._unreadable)      # what _readLeaves and _node look at
        shape = (lambda node: node[0]) if digest == 1 else tuple
        if leaves is not None:
            leaves, given = cls._readLeaves(reader, leaves)
            if leaves is cls._unreadable or given != count:
                raise GstarkError(f'{cls._who}: {count} paths and {given} leaves of {digest} element{"s" if digest > 1 else ""}: a path starts from one leaf')
        if not count:
            return []
        if not cls._walksOnDevice(hash):
            if isinstance(paths, Matrix):
                paths = [[row[l * digest:(l + 1) * digest] for l in range(depth + 1)] for row in paths.toValues()]
            if leaves is not None:
                starts = leaves if isinstance(leaves, list) else _rows(leaves)
                paths = [[list(leaf)] + path[1:] for leaf, path in zip(starts, paths)]
            return [shape(path_root(i, path, lambda left, right: cls._node(reader, left, right))) for i, path in zip(indexes, paths)]
        be = f.backend
        if not isinstance(paths, Matrix):
            paths = f.newMatrixFrom([[v for node in path for v in node] for path in paths])
        if leaves is not None and not isinstance(leaves, (Matrix, Vector)):
            leaves = f.newMatrixFrom(leaves)
        roots = Matrix(be, count, digest)
        cls._pathRootsOnDevice(hash, C.c_void_p(paths.ptr), depth, digest, (C.c_uint64 * count)(*indexes), C.c_void_p(leaves.ptr) if leaves is not None else None,
                               count, C.c_void_p(roots.ptr))
        return [shape(r) for r in roots.toValues()]


def _rows(array):                            # the nodes of a device array as rows of `digest` integers
    return array.toValues() if isinstance(array, Matrix) else [[v] for v in array.toValues()]
