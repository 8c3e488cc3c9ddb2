"""Sparse Merkle trees of fixed depth kept on the device (include/gstark_sparse_tree.h, csrc/field_tree.hip, csrc/sparse_tree_plan.h):
the producing side for key spaces no dense tree can hold, with the interface of the dense trees of field_tree.py.

A tree of depth d (1 .. 36) IS the dense heap tree of 2^d leaves whose leaves all hold `empty` until they are set: root, paths and update
records are bit for bit those of HadesMerkleTree / RescueMerkleTree over [empty] * 2^d after the same calls.  Only nodes with something
set below them are stored; every other node is empties[level].  On a library without the family's entry points (the tests' double, a
HostField) the same values come from host integers: a dict per level and the subclass's `_node`."""
import ctypes as C

from ._abi import GstarkError
from .field import Matrix, Vector
from .field_tree import FieldMerkleTree, TreeUpdate, _rows
from .hades import HadesMerkleTree
from .rescue_hash import RescueMerkleTree

MAX_DEPTH = 36
MAX_PER_CALL = 1 << 20


class SparseFieldMerkleTree(FieldMerkleTree):
    """The tree of 2^depth leaves that all hold `empty` (default: zeros) until set.  `root`, `prove`, `proveMany`, `update` and
    `updateMany` are FieldMerkleTree's; a path of an index never set starts with `empty` (the non-membership path); pathRoots, verifyMany
    and verifyUpdates are inherited unchanged.  Memory: each stored leaf costs up to `depth` stored nodes on the device and as many
    entries of the host index; the store grows by doubling from `slots_hint` slots and never past 2^31.  Setting a leaf back to `empty`
    keeps its nodes stored — nothing is pruned — and the values are still those of the definition.  At most 2^20 updates or paths per
    call.  A refused call leaves the tree as it was.  The tree holds its hash object, so the hash outlives it; drop a tree before closing
    its backend (a tree that outlives the context is not freed by the library).  A subclass is a dense tree class (its `_node`, its refusals) with `_createEntry`
    and `_createOnDevice(empty_bytes, slots_hint, out)`."""
    _header = 'include/gstark_sparse_tree.h'
    _entries = ('gs_sparse_update', 'gs_sparse_paths', 'gs_sparse_root', 'gs_sparse_empties', 'gs_sparse_stored', 'gs_sparse_destroy')

    def __init__(self, hash, depth, digest, empty=None, slots_hint=1024):
        f = hash.field
        self.hash, self.field, self.digest = hash, f, digest
        depth, slots_hint = int(depth), int(slots_hint)
        if not 1 <= depth <= MAX_DEPTH:
            raise GstarkError(f'{self._who}: a depth of 1 .. {MAX_DEPTH}, not {depth}')
        if not 1 <= slots_hint <= 1 << 31:
            raise GstarkError(f'{self._who}: slots_hint is 1 .. 2^31, not {slots_hint}')
        rows, given = self._readLeaves([[0] * digest if digest > 1 else 0] if empty is None else [empty])
        if rows is self._unreadable or given != 1:
            raise GstarkError(f'{self._who}: the empty leaf has {digest} element{"s" if digest > 1 else ""}')
        self.depth, self.leafCount, self.deviceNodes = depth, 1 << depth, None
        self._tree = self._levels = self._emptyRows = None
        if hash.onDevice:
            lib = f.backend.lib
            for name in (self._createEntry,) + self._entries:
                if not hasattr(lib, name):                    # a hash that lives on the device keeps its trees there: no quiet host path
                    raise GstarkError(f'{self._who}: the library has no {name} ({self._header})')
            tree = C.c_void_p()
            self._createOnDevice(b''.join(f.le(v) for v in rows[0]), slots_hint, C.byref(tree))
            self._tree = tree
        else:
            self._emptyRows = [list(rows[0])]
            for _ in range(depth):
                self._emptyRows.append(self._node(self._emptyRows[-1], self._emptyRows[-1]))
            self._levels = [{} for _ in range(depth + 1)]

    def __del__(self):
        try:
            if self._tree is not None and self.field.backend.ctx:
                self.field.backend.lib.gs_sparse_destroy(self.field.backend.ctx, self._tree)
            self._tree = None
        except Exception:
            pass

    # ---- what the tree holds
    @property
    def nodes(self):
        raise GstarkError(f'{self._who}: a sparse tree has no node array: root, prove and proveMany read it')

    @property
    def empties(self):
        """empties[0 .. depth]: the node of every level above nothing but empty leaves"""
        if self._emptyRows is None:
            out = Matrix(self.field.backend, self.depth + 1, self.digest)
            self.field.backend.call('gs_sparse_empties', self._tree, C.c_void_p(out.ptr))
            self._emptyRows = out.toValues()
        return [self._shape(r) for r in self._emptyRows]

    @property
    def stored(self):
        """the number of stored nodes per level 0 (leaves) .. depth (the root)"""
        if self._tree is None:
            return [len(level) for level in self._levels]
        return [int(self.field.backend.lib.gs_sparse_stored(self._tree, l)) for l in range(self.depth + 1)]

    @property
    def root(self):
        if self._tree is None:
            return self._shape(self._levels[self.depth].get(0, self._emptyRows[self.depth]))
        out = Matrix(self.field.backend, 1, self.digest)
        self.field.backend.call('gs_sparse_root', self._tree, C.c_void_p(out.ptr))
        return self._shape(out.toValues()[0])

    def get(self, index):
        """the leaf at `index`: `empty` where none was set"""
        return self.getMany([index])[0]

    def getMany(self, indexes):
        return [path[0] for path in self.proveMany(indexes)]

    def _readIndexes(self, indexes, what):
        indexes = [int(i) for i in indexes]
        if len(indexes) > MAX_PER_CALL:
            raise GstarkError(f'{self._who}: at most 2^20 {what} per call, not {len(indexes)}')
        for i in indexes:
            if not 0 <= i < self.leafCount:
                raise GstarkError(f'{self._who}: index {i} is outside of the 2^{self.depth} leaves')
        return indexes

    def _at(self, level, node):
        return self._levels[level].get(node, self._emptyRows[level])

    def proveMany(self, indexes, device=False):
        """prove(index) for every index (repeats allowed), set or not: per path the leaf, then its siblings bottom-up.  device=True: the
        paths as a Matrix of one row of (depth + 1) * digest elements per path, which pathRoots and verifyMany take without a read-back."""
        indexes = self._readIndexes(indexes, 'paths')
        count, per, d = len(indexes), self.depth + 1, self.digest
        if self._tree is None:
            paths = [[self._at(0, i)] + [self._at(l, (i >> l) ^ 1) for l in range(self.depth)] for i in indexes]
            if device:
                return self.field.newMatrixFrom([[v for node in path for v in node] for path in paths]) if count else Matrix(self.field.backend, 0, per * d)
            return [[self._shape(node) for node in path] for path in paths]
        out = Matrix(self.field.backend, count, per * d)
        if count:
            self.field.backend.call('gs_sparse_paths', self._tree, (C.c_uint64 * count)(*indexes), count, C.c_void_p(out.ptr))
        if device:
            return out
        return [[self._shape(row[l * d:(l + 1) * d]) for l in range(per)] for row in out.toValues()] if count else []

    def updateMany(self, indexes, leaves):
        """FieldMerkleTree.updateMany on the tree of 2^depth leaves: updates apply in call order, repeated indexes and a leaf equal to the
        old one are allowed; one TreeUpdate(before, root) per update, `before` what prove(index) returned just before it and `root` the
        root just after it.  On the device: one upload of the leaves and of the plan, a hash launch per level over the whole batch, one
        read-back of all witnesses and roots."""
        indexes = self._readIndexes(indexes, 'updates')
        leaves, count = self._readLeaves(leaves)
        if leaves is self._unreadable:
            raise GstarkError(f'{self._who}: every leaf has {self.digest} elements')
        if count != len(indexes):
            raise GstarkError(f'{self._who}: {len(indexes)} indexes and {count} leaves: an update is one of each')
        if not count:
            return []
        per, d = self.depth + 1, self.digest
        if self._tree is None:
            if not isinstance(leaves, list):
                leaves = _rows(leaves)
            out = []
            for i, leaf in zip(indexes, leaves):
                before = [self._shape(self._at(0, i))] + [self._shape(self._at(l, (i >> l) ^ 1)) for l in range(self.depth)]
                self._levels[0][i] = list(leaf)
                for l in range(self.depth):
                    node = i >> l
                    self._levels[l + 1][node >> 1] = self._node(self._at(l, node & ~1), self._at(l, node | 1))
                out.append(TreeUpdate(before, self._shape(self._levels[self.depth][0])))
            return out
        src = leaves if isinstance(leaves, (Matrix, Vector)) else self.field.newMatrixFrom(leaves)
        before, roots = Matrix(self.field.backend, count, per * d), Matrix(self.field.backend, count, d)
        self.field.backend.call('gs_sparse_update', self._tree, (C.c_uint64 * count)(*indexes), C.c_void_p(src.ptr), count, C.c_void_p(before.ptr), C.c_void_p(roots.ptr))
        roots = roots.toValues()
        return [TreeUpdate([self._shape(row[l * d:(l + 1) * d]) for l in range(per)], self._shape(roots[j])) for j, row in enumerate(before.toValues())]


class HadesSparseMerkleTree(SparseFieldMerkleTree, HadesMerkleTree):
    """The sparse form of HadesMerkleTree(hash, [empty] * 2^depth, digest): nodes of `digest` elements (1 or 2), 2 * digest < width."""
    _who, _createEntry = 'HadesSparseMerkleTree', 'gs_hades_sparse_create'

    def __init__(self, hash, depth, digest, empty=None, slots_hint=1024):
        if digest not in (1, 2) or 2 * digest >= hash.width:
            raise GstarkError(f'{self._who}: nodes of {digest} elements (1 or 2): two of them do not fit a state of {hash.width} beside its capacity')
        SparseFieldMerkleTree.__init__(self, hash, depth, digest, empty, slots_hint)

    def _createOnDevice(self, empty, slots_hint, out):
        self.field.backend.call(self._createEntry, self.hash.handle(), self.depth, self.digest, empty, slots_hint, out)


class RescueSparseMerkleTree(SparseFieldMerkleTree, RescueMerkleTree):
    """The sparse form of RescueMerkleTree(hash, [empty] * 2^depth): nodes of one element, width 3 .. 8."""
    _who, _createEntry = 'RescueSparseMerkleTree', 'gs_rescue_sparse_create'

    def __init__(self, hash, depth, empty=None, slots_hint=1024):
        if hash.width < 3:
            raise GstarkError(f'{self._who}: two nodes do not fit a state of {hash.width} beside its capacity (width 3 .. 8)')
        SparseFieldMerkleTree.__init__(self, hash, depth, 1, empty, slots_hint)

    def _createOnDevice(self, empty, slots_hint, out):
        self.field.backend.call(self._createEntry, self.hash.handle(), self.depth, empty, slots_hint, out)
