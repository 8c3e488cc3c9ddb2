'use strict';
// js/field_tree.js — what js/hades.js and js/rescue.js share above the addon's table: a device handle made on first use and destroyed
// when its owner is collected, one permutation per row of a device Matrix, and the heap-layout Merkle tree of nodes of `digest` field
// elements with its paths (the gather is the family-neutral gs_hades_merkle_paths: it reads nothing but the node array).
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

/** the tree over the device leaves `src` (the caller has checked that they are the field's: field._own), built by buildCall(handle, src, n, deviceNodes); newNodes(count): an array of the kind deviceNodes is */
class DeviceTree {
    constructor(field, handle, digest, src, newNodes, buildCall) {
        const n = src instanceof Vector ? src.length : src.rowCount;
        this.field = field; this.digest = digest; this.leafCount = n;
        this.depth = Math.round(Math.log2(n));
        this._newNodes = newNodes;
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
}

/** a path (the leaf, then its siblings bottom-up) against a root: node(left, right) level by level, sides by the index bits */
function verifyPath(root, index, proof, node, same = (a, b) => a === b) {
    let v = proof[0];
    for (let level = 1; level < proof.length; level++) {
        v = Math.floor(index / 2 ** (level - 1)) % 2 === 1 ? node(proof[level], v) : node(v, proof[level]);
    }
    return same(root, v);
}

module.exports = { destroyRegistry, needDevice, lazyHandle, hashMany, DeviceTree, verifyPath };
