'use strict';
// js/field_tree.js — what js/hades.js and js/rescue.js share above the addon's table: a device handle made on first use and destroyed
// when its owner is collected, one permutation per row of a device Matrix, and the heap-layout Merkle tree of nodes of `digest` field
// elements with its paths (the gather is the family-neutral gs_hades_merkle_paths: it reads nothing but the node array) and its batched
// updates (include/gstark_tree_update.h: update / updateMany return every update's witness), and the consuming side of both
// (include/gstark_tree_verify.h: static pathRoots / verifyMany / verifyUpdates check batches of paths and update records in one launch),
// and the sparse tree of fixed depth over the same node functions (include/gstark_sparse_tree.h: SparseDeviceTree).
const { Matrix, Vector } = require('./galois.js');

/** a registry that destroys the handle of a collected owner through `symbol` (null where the engine has none) */
function destroyRegistry(symbol) {
    if (typeof FinalizationRegistry === 'undefined') return null;
    return new FinalizationRegistry(({ lib, ctx, handle }) => { try { lib.call(symbol, ctx, handle); } catch (e) { /* context gone */ } });
}

/** throws when the field's library lacks the gs_<family>_* entry points (they are optional on an implementation of the ABI) */
function needDevice(field, family, what) {
    if (!field.lib.has || !field.lib.has(`gs_${family}_hash`)) {
        throw new Error(`the library of the field of ${field.modulus} elements has no gs_${family}_* entry points (include/gstark_${family}.h): ${what} hashes and trees are not computed on this device library`);
    }
}

/** throws when the field's library lacks `symbol` of include/gstark_tree_update.h (optional in the same way) */
function needUpdate(field, symbol) {
    if (!field.lib.has || !field.lib.has(symbol)) {
        throw new Error(`the library of the field of ${field.modulus} elements has no ${symbol} entry point (include/gstark_tree_update.h): trees are not updated on this device library`);
    }
}

/** throws when the field's library lacks `symbol` of include/gstark_tree_verify.h (optional in the same way) */
function needVerify(field, symbol) {
    if (!field.lib.has || !field.lib.has(symbol)) {
        throw new Error(`the library of the field of ${field.modulus} elements has no ${symbol} entry point (include/gstark_tree_verify.h): batches of paths are not checked on this device library`);
    }
}

/** handle(): the parameter set on the field's context (a BigInt); create(out) uploads it on first use, the registry destroys it after owner() */
function lazyHandle(field, need, registry, owner, create) {
    let handle = null;
    return function () {
        if (handle === null) {
            need(field);
            const out = Buffer.alloc(8);
            create(out);
            handle = out.readBigUInt64LE(0);
            if (registry) registry.register(owner(), { lib: field.lib, ctx: field.ctx, handle });
        }
        return handle;
    };
}

/** one permutation per row of a device Matrix (or of rows of BigInts); options: what `symbol` takes between `digest` and `out` */
function hashMany(field, symbol, handle, rows, digest, ...options) {
    if (!(rows instanceof Matrix)) rows = field.newMatrixFrom(rows);
    field._own(rows);
    const out = new Matrix(field, rows.rowCount, digest);
    field.lib.call(symbol, field.ctx, handle, rows.ptr, rows.rowCount, rows.colCount, digest, ...options, out.ptr);
    return out;
}

/** throws when the field's library lacks `symbol` of include/gstark_absorb.h (optional in the same way) */
function needAbsorb(field, symbol) {
    if (!field.lib.has || !field.lib.has(symbol)) {
        throw new Error(`the library of the field of ${field.modulus} elements has no ${symbol} entry point (include/gstark_absorb.h): records are not absorbed on this device library`);
    }
}

/** the rate of absorb / absorbMany (default: width - 1 up to a state of 3, width - 2 above) after the refusals that need no input */
function absorbRate(width, digest, rate) {
    if (rate === undefined || rate === null) rate = width <= 3 ? width - 1 : width - 2;
    if (!(Number.isInteger(rate) && rate >= 1 && rate < width)) throw new Error(`absorb: a rate of ${rate} does not leave a capacity in a state of ${width} (1 .. ${width - 1})`);
    if (!((digest === 1 || digest === 2) && digest <= rate)) throw new Error(`absorb: a digest of 1 or 2 elements and at most the rate (${rate}), not ${digest}`);
    return rate;
}

const ABSORB_MAX_LENGTH = 1 << 16;

/** absorb on BigInts (include/gstark_absorb.h): state = zeros with state[rate] = the length; per block of `rate` inputs the block is
 *  ADDED to state[0 .. rate) and the state permuted; the first `digest` elements of the last state */
function absorbHost(field, width, permute, inputs, digest, rate) {
    rate = absorbRate(width, digest, rate);
    if (!(inputs.length >= 1 && inputs.length <= ABSORB_MAX_LENGTH)) throw new Error(`absorb: a record of ${inputs.length} elements (1 .. ${ABSORB_MAX_LENGTH})`);
    let state = new Array(width).fill(0n);
    state[rate] = field.mod(BigInt(inputs.length));
    for (let at = 0; at < inputs.length; at += rate) {
        for (let j = 0; j < rate && at + j < inputs.length; j++) state[j] = field.mod(state[j] + BigInt(inputs[at + j]));
        state = permute(state);
    }
    return state.slice(0, digest);
}

/** absorb for every row of a device Matrix of count x L (or of rows of BigInts) in one launch — with `columns`, for every column of the
 *  register-major L x count Matrix: a Matrix of count x digest, like hashMany; options: what `symbol` takes between `digest` and `out` */
function absorbMany(field, symbol, handle, width, rows, digest, rate, columns, ...options) {
    needAbsorb(field, symbol);
    rate = absorbRate(width, digest, rate);
    if (!(rows instanceof Matrix)) {
        if (rows.some(r => r.length !== rows[0].length)) throw new Error(`absorb: every ${columns ? 'column' : 'row'} has the same number of elements`);
        rows = field.newMatrixFrom(rows);
    }
    field._own(rows);
    const count = columns ? rows.colCount : rows.rowCount, length = columns ? rows.rowCount : rows.colCount;
    if (!(length >= 1 && length <= ABSORB_MAX_LENGTH)) throw new Error(`absorb: a record of ${length} elements (1 .. ${ABSORB_MAX_LENGTH})`);
    const out = new Matrix(field, count, digest);
    if (count) field.lib.call(symbol, field.ctx, handle(), rows.ptr, count, length, columns ? 1 : length, columns ? count : 1, rate, digest, ...options, out.ptr);
    return out;
}

/** the tree over the device leaves `src` (the caller has checked that they are the field's: field._own), built by buildCall(handle, src, n, deviceNodes); newNodes(count): an array of the kind deviceNodes is;
 *  update: { symbol, call(handle, deviceNodes, n, indexes, leaves, count, before, roots) } — the family's entry of include/gstark_tree_update.h */
class DeviceTree {
    constructor(field, handle, digest, src, newNodes, buildCall, update) {
        const n = src instanceof Vector ? src.length : src.rowCount;
        this.field = field; this.digest = digest; this.leafCount = n;
        this.depth = Math.round(Math.log2(n));
        this._newNodes = newNodes; this._handle = handle; this._update = update;
        this.deviceNodes = newNodes(2 * n);
        buildCall(handle, src, n, this.deviceNodes);
    }
    _shape(row) { return this.digest === 1 ? row[0] : row; }      // a node as the reference's classes hold it: a pair, or one value
    _values(array) { return array instanceof Vector ? array.toValues() : array.toValues().map(r => this._shape(r)); }
    get nodes() { const values = this._values(this.deviceNodes); values[0] = undefined; return values; }
    get root() { return this.deviceNodes instanceof Vector ? this.deviceNodes.getValue(1) : this._shape(this.deviceNodes.row(1).toValues()); }
    prove(index) { return this.proveMany([index])[0]; }
    /** prove(index) for every index (repeats allowed): one launch, one read-back */
    proveMany(indexes) {
        if (!indexes.length) return [];
        const per = this.depth + 1, out = this._newNodes(indexes.length * per);
        this.field.lib.call('gs_hades_merkle_paths', this.field.ctx, this.deviceNodes.ptr, this.leafCount, this.digest, indexes, indexes.length, out.ptr);
        const values = this._values(out);
        return indexes.map((_, k) => values.slice(k * per, (k + 1) * per));
    }
    update(index, leaf) { return this.updateMany([index], [leaf])[0]; }
    /** sets leaf indexes[j] to leaves[j], j = 0, 1, .. in that order (repeats allowed); per update { before, root }: prove(indexes[j]) as it
     *  stood just before update j, and the root just after it (the witness of ComputeMerkleUpdate).  One upload, one launch sequence, one read-back. */
    updateMany(indexes, leaves) {
        needUpdate(this.field, this._update.symbol);
        const count = indexes.length, single = this.deviceNodes instanceof Vector;
        let src = leaves;
        if (Array.isArray(leaves)) {
            if (leaves.length !== count) throw new Error(`${count} indexes and ${leaves.length} leaves: an update is one of each`);
            if (!count) return [];
            src = single ? this.field.newVectorFrom(leaves) : this.field.newMatrixFrom(this.digest === 1 ? leaves.map(v => [v]) : leaves);
        }
        this.field._own(src);
        if ((src instanceof Vector ? src.length : src.rowCount) !== count) throw new Error(`${count} indexes and ${src instanceof Vector ? src.length : src.rowCount} leaves: an update is one of each`);
        if ((src instanceof Vector ? 1 : src.colCount) !== this.digest) throw new Error(`the leaves have ${this.digest} element${this.digest > 1 ? 's' : ''} each`);
        if (!count) return [];
        const per = this.depth + 1, before = this._newNodes(count * per), roots = this._newNodes(count);
        this._update.call(this._handle, this.deviceNodes, this.leafCount, indexes, src, count, before, roots);
        const values = this._values(before), after = this._values(roots);
        return indexes.map((_, j) => ({ before: values.slice(j * per, (j + 1) * per), root: after[j] }));
    }
}

/** throws when the field's library lacks `symbol` of include/gstark_sparse_tree.h (optional in the same way) */
function needSparse(field, symbol) {
    if (!field.lib.has || !field.lib.has(symbol)) {
        throw new Error(`the library of the field of ${field.modulus} elements has no ${symbol} entry point (include/gstark_sparse_tree.h): sparse trees are not kept on this device library`);
    }
}

const sparseRegistry = destroyRegistry('gs_sparse_destroy');

/** The sparse tree of 2^depth leaves (depth 1 .. 36) that all hold `empty` (default: zeros) until set: root, paths and update records are
 *  those of the dense tree over [empty] * 2^depth.  Only nodes with something set below them are stored on the device (each stored leaf
 *  costs up to `depth` stored nodes and host index entries; the store doubles from slotsHint slots, never past 2^31; nothing is pruned).
 *  Indexes are Numbers or BigInts below 2^depth; at most 2^20 updates or paths per call.  A path of an index never set starts with
 *  `empty`.  There is no `stored` member: gs_sparse_stored returns a count, not a status, and the addon's call() delivers statuses only
 *  (Python has it).  family: { symbol, create(handle, depth, emptyBytes, slotsHint, out) } — the family's create entry.  There is no host
 *  fallback: a missing entry throws an Error that names it. */
class SparseDeviceTree {
    constructor(field, hash, depth, digest, empty, slotsHint, family) {
        for (const symbol of [family.symbol, 'gs_sparse_update', 'gs_sparse_paths', 'gs_sparse_root', 'gs_sparse_empties', 'gs_sparse_destroy']) needSparse(field, symbol);
        if (!(Number.isInteger(depth) && depth >= 1 && depth <= 36)) throw new Error(`a depth of 1 .. 36, not ${depth}`);
        if (!(Number.isInteger(slotsHint) && slotsHint >= 1 && slotsHint <= 2 ** 31)) throw new Error(`slotsHint is 1 .. 2^31, not ${slotsHint}`);
        let row = new Array(digest).fill(0n);
        if (empty !== undefined && empty !== null) row = digest === 1 && !Array.isArray(empty) ? [empty] : empty;
        if (!Array.isArray(row) || row.length !== digest || row.some(v => typeof v !== 'bigint')) throw new Error(`the empty leaf has ${digest} element${digest > 1 ? 's' : ''} (BigInts)`);
        this.field = field; this.hash = hash; this.depth = depth; this.digest = digest; this.leafCount = 2 ** depth;
        const out = Buffer.alloc(8);
        family.create(hash.handle(), depth, field.packLe(row.map(v => field.mod(v))), slotsHint, out);
        this._tree = out.readBigUInt64LE(0);
        if (sparseRegistry) sparseRegistry.register(this, { lib: field.lib, ctx: field.ctx, handle: this._tree });
        this._empties = null;
    }
    _shape(row) { return this.digest === 1 ? row[0] : row; }
    _nodes(row) { const out = []; for (let l = 0; l * this.digest < row.length; l++) out.push(this._shape(row.slice(l * this.digest, (l + 1) * this.digest))); return out; }
    /** indexes as BigInts (anything above 2^32 survives the trip to the library) */
    _indexes(indexes, what) {
        if (indexes.length > 2 ** 20) throw new Error(`at most 2^20 ${what} per call, not ${indexes.length}`);
        return indexes.map(i => {
            const ok = typeof i === 'bigint' || Number.isSafeInteger(i), v = ok ? BigInt(i) : -1n;
            if (v < 0n || v >> BigInt(this.depth)) throw new Error(`index ${i} is outside of the 2^${this.depth} leaves`);
            return v;
        });
    }
    get root() {
        const out = new Matrix(this.field, 1, this.digest);
        this.field.lib.call('gs_sparse_root', this.field.ctx, this._tree, out.ptr);
        return this._shape(out.toValues()[0]);
    }
    /** empties[0 .. depth]: the node of every level above nothing but empty leaves */
    get empties() {
        if (this._empties === null) {
            const out = new Matrix(this.field, this.depth + 1, this.digest);
            this.field.lib.call('gs_sparse_empties', this.field.ctx, this._tree, out.ptr);
            this._empties = out.toValues().map(r => this._shape(r));
        }
        return this._empties.slice();
    }
    get(index) { return this.prove(index)[0]; }
    prove(index) { return this.proveMany([index])[0]; }
    /** prove(index) for every index, set or not: one launch, one read-back; device = true: the Matrix of one row per path, which the static
     *  pathRoots / verifyMany take without a read-back */
    proveMany(indexes, device = false) {
        const idx = this._indexes(indexes, 'paths'), out = new Matrix(this.field, idx.length, (this.depth + 1) * this.digest);
        if (idx.length) this.field.lib.call('gs_sparse_paths', this.field.ctx, this._tree, idx, idx.length, out.ptr);
        if (device) return out;
        return idx.length ? out.toValues().map(r => this._nodes(r)) : [];
    }
    update(index, leaf) { return this.updateMany([index], [leaf])[0]; }
    /** sets leaf indexes[j] to leaves[j], j = 0, 1, .. in that order (repeats allowed); per update { before, root } as DeviceTree.updateMany */
    updateMany(indexes, leaves) {
        const idx = this._indexes(indexes, 'updates'), count = idx.length;
        let src = leaves;
        if (Array.isArray(leaves)) {
            if (leaves.length !== count) throw new Error(`${count} indexes and ${leaves.length} leaves: an update is one of each`);
            if (!count) return [];
            if (leaves.some(v => (Array.isArray(v) ? v.length : 1) !== this.digest || (this.digest > 1) !== Array.isArray(v))) throw new Error(`the leaves have ${this.digest} element${this.digest > 1 ? 's' : ''} each`);
            src = this.field.newMatrixFrom(this.digest === 1 ? leaves.map(v => [v]) : leaves);
        }
        this.field._own(src);
        if ((src instanceof Vector ? src.length : src.rowCount) !== count) throw new Error(`${count} indexes and ${src instanceof Vector ? src.length : src.rowCount} leaves: an update is one of each`);
        if ((src instanceof Vector ? 1 : src.colCount) !== this.digest) throw new Error(`the leaves have ${this.digest} element${this.digest > 1 ? 's' : ''} each`);
        if (!count) return [];
        const before = new Matrix(this.field, count, (this.depth + 1) * this.digest), roots = new Matrix(this.field, count, this.digest);
        this.field.lib.call('gs_sparse_update', this.field.ctx, this._tree, idx, src.ptr, count, before.ptr, roots.ptr);
        const values = before.toValues(), after = roots.toValues();
        return idx.map((_, j) => ({ before: this._nodes(values[j]), root: this._shape(after[j]) }));
    }
}

/** a path (the leaf, then its siblings bottom-up) against a root: node(left, right) level by level, sides by the index bits */
function verifyPath(root, index, proof, node, same = (a, b) => a === b) {
    let v = proof[0];
    for (let level = 1; level < proof.length; level++) {
        v = Math.floor(index / 2 ** (level - 1)) % 2 === 1 ? node(proof[level], v) : node(v, proof[level]);
    }
    return same(root, v);
}

/** The static members pathRoots / verifyMany / verifyUpdates of a tree class (include/gstark_tree_verify.h): a verifier holds a root and
 *  the hash object, not a tree.  family: { digest, symbol, call(field, handle, paths, depth, indexes, leaves, count, roots) }.
 *  proofs: paths as prove returns them (the leaf, then its siblings bottom-up), or a device Matrix of one row of (depth + 1) * digest
 *  elements per path; leaves (optional; an array, or a device array): path k starts from leaves[k] instead of its own leaf. */
function installVerify(cls, family) {
    const { digest, symbol } = family;
    const shape = row => (digest === 1 ? row[0] : row);
    const same = digest === 1 ? (a, b) => a === b : (a, b) => a.length === b.length && a.every((x, i) => x === b[i]);
    const count = array => (array instanceof Vector ? array.length : array.rowCount);
    /** the root each path implies, in the shape `root` has: ONE launch walks every level of every path */
    cls.pathRoots = function (hash, indexes, proofs, leaves) {
        const field = hash && hash.field;
        if (!field || !hash.handle) throw new Error('the hash object must come from js/hades.js or js/rescue.js');
        needVerify(field, symbol);
        let paths = proofs;
        if (Array.isArray(proofs)) {
            if (proofs.length !== indexes.length) throw new Error(`${indexes.length} indexes and ${proofs.length} paths: a path is checked at one index`);
            if (!proofs.length) return [];
            if (proofs.some(path => path.length !== proofs[0].length)) throw new Error('the paths have unequal lengths: one call checks paths of one depth');
            if (proofs[0].length < 2) throw new Error('a path is a leaf and at least one sibling');
            if (proofs.some(path => path.some(node => (Array.isArray(node) ? node.length : 1) !== digest || (digest > 1) !== Array.isArray(node)))) throw new Error(`every node of a path has ${digest} element${digest > 1 ? 's' : ''}`);
            paths = field.newMatrixFrom(digest === 1 ? proofs : proofs.map(path => [].concat(...path)));
        } else {
            if (!(proofs instanceof Matrix)) throw new Error('the paths are an array of paths or a device Matrix of one row per path');
            field._own(paths);
            if (paths.rowCount !== indexes.length) throw new Error(`${indexes.length} indexes and ${paths.rowCount} paths: a path is checked at one index`);
            if (paths.colCount % digest || paths.colCount < 2 * digest) throw new Error(`a row of ${paths.colCount} elements is no leaf of ${digest} with at least one sibling`);
            if (!paths.rowCount) return [];
        }
        const depth = paths.colCount / digest - 1, n = indexes.length;
        for (const i of indexes) {
            if (!(Number.isInteger(i) && i >= 0 && i < 2 ** depth)) throw new Error(`index ${i} is outside of the ${2 ** depth} leaves of a path of ${depth} siblings`);
        }
        let src = null;
        if (leaves !== undefined && leaves !== null) {
            src = leaves;
            if (Array.isArray(leaves)) src = leaves.length ? (digest === 1 ? field.newVectorFrom(leaves) : field.newMatrixFrom(leaves)) : new Vector(field, 0);
            field._own(src);
            if (count(src) !== n) throw new Error(`${n} paths and ${count(src)} leaves: a path starts from one leaf`);
            if ((src instanceof Vector ? 1 : src.colCount) !== digest) throw new Error(`the leaves have ${digest} element${digest > 1 ? 's' : ''} each`);
        }
        const roots = new Matrix(field, n, digest);
        family.call(field, hash.handle(), paths, depth, indexes, src ? src.ptr : 0n, n, roots);
        return roots.toValues().map(shape);
    };
    /** verify(root, indexes[k], proofs[k], ..) for every k: one boolean per path */
    cls.verifyMany = function (root, indexes, proofs, hash) {
        return cls.pathRoots(hash, indexes, proofs).map(r => same(r, root));
    };
    /** one boolean per record of updateMany(indexes, leaves) on a tree whose root was oldRoot: records[j].before at indexes[j] implies the
     *  root before it (oldRoot, then records[j - 1].root as claimed) and the same siblings under leaves[j] imply records[j].root.  Two launches. */
    cls.verifyUpdates = function (oldRoot, indexes, leaves, records, hash) {
        const field = hash && hash.field;
        if (!field || !hash.handle) throw new Error('the hash object must come from js/hades.js or js/rescue.js');
        needVerify(field, symbol);
        if (records.length !== indexes.length) throw new Error(`${indexes.length} indexes and ${records.length} records: an update is one of each`);
        if (!records.length) { cls.pathRoots(hash, indexes, [], leaves); return []; }
        if (records.some(r => r.before.length !== records[0].before.length)) throw new Error('the paths have unequal lengths: one call checks paths of one depth');
        if (records[0].before.length < 2) throw new Error('a path is a leaf and at least one sibling');
        const paths = field.newMatrixFrom(records.map(r => (digest === 1 ? r.before : [].concat(...r.before))));      // one upload serves both launches
        const before = cls.pathRoots(hash, indexes, paths), after = cls.pathRoots(hash, indexes, paths, leaves);
        return records.map((r, j) => same(before[j], j ? records[j - 1].root : oldRoot) && same(after[j], r.root));
    };
}

module.exports = { destroyRegistry, needDevice, needUpdate, needVerify, needSparse, lazyHandle, hashMany, absorbHost, absorbMany, DeviceTree, SparseDeviceTree, verifyPath, installVerify };
