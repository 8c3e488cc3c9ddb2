'use strict';
// js/hades.js — the Poseidon helpers of the reference's examples/poseidon/utils.ts with the bulk work on the device
// (include/gstark_hades.h through the addon's table): createHash(field, exp, rf, rp, stateWidth, rc?) returns the example's hash function
// (BigInt arithmetic on the host, as upstream) which also carries .hashMany(matrix, digest) — one permutation per row in one launch —,
// and MerkleTree / MerkleTree2 have the example's members (nodes, root, prove, static verify) plus proveMany(indexes): the tree is built
// by the device, the paths of any number of leaves come back in one read-back.  `field` is a PrimeField of js/galois.js.  A field whose
// library lacks the entry points (they are optional on an implementation of the ABI) makes the device members throw an Error saying so.
const crypto = require('crypto');
const { Matrix, Vector } = require('./galois.js');

function constants(field, seed, count) {      // utils.ts:115-122
    const out = new Array(count);
    for (let i = 0; i < count; i++) out[i] = field.mod(BigInt('0x' + crypto.createHash('sha256').update(`${seed}${i}`).digest('hex')));
    return out;
}
function getRoundConstants(field, width, rounds) {      // utils.ts:51-62
    const flat = constants(field, 'Hades', width * rounds), out = [];
    for (let i = 0; i < rounds; i++) out.push(flat.slice(i * width, (i + 1) * width));
    return out;
}
function getMdsMatrix(field, width) {      // utils.ts:64-79
    const xs = constants(field, 'HadesMDSx', width), ys = constants(field, 'HadesMDSy', width);
    if (new Set([...xs, ...ys]).size !== width * 2) throw new Error('MDS values are not all different');
    return xs.map(x => ys.map(y => field.inv(field.sub(x, y))));
}

const registry = (typeof FinalizationRegistry !== 'undefined')
    ? new FinalizationRegistry(({ lib, ctx, handle }) => { try { lib.call('gs_hades_destroy', ctx, handle); } catch (e) { /* context gone */ } })
    : null;

function needDevice(field) {
    if (!field.lib.has || !field.lib.has('gs_hades_hash')) {
        throw new Error(`the library of the field of ${field.modulus} elements has no gs_hades_* entry points (include/gstark_hades.h): Poseidon hashes and trees are not computed on this device library`);
    }
}

/** createHash of utils.ts:19 (`mds`: a matrix other than the derived one, e.g. the DATA of assembly/lib128.aa) */
function createHash(field, exp, rf, rp, stateWidth, rc, mds) {
    const m = stateWidth, alpha = BigInt(exp);
    if (!(m >= 2 && m <= 8)) throw new Error(`createHash: a state of ${m} elements is outside 2 .. 8`);
    if (rf < 2 || rf % 2 || rp < 0) throw new Error(`createHash: ${rf} full rounds (even, at least 2) and ${rp} partial rounds`);
    if (alpha < 2n || alpha >> 64n) throw new Error(`createHash: the exponent ${alpha} is outside 2 .. 2^64 - 1`);
    const ark = (rc || getRoundConstants(field, m, rf + rp)).map(row => row.map(v => field.mod(BigInt(v))));
    const matrix = (mds || getMdsMatrix(field, m)).map(row => row.map(v => field.mod(BigInt(v))));
    if (ark.length !== rf + rp || ark.some(row => row.length !== m)) throw new Error(`createHash: ${rf + rp} rows of ${m} round constants are needed`);
    if (matrix.length !== m || matrix.some(row => row.length !== m)) throw new Error(`createHash: the matrix has ${m} rows of ${m} values`);
    const p = field.modulus;

    const hash = function (inputs) {
        if (!(inputs.length > 0 && inputs.length < m)) throw new Error(`hash: ${inputs.length} inputs do not fit a state of ${m}`);
        let state = inputs.map(v => field.mod(BigInt(v)));
        while (state.length < m) state.push(0n);
        for (let i = 0; i < rf + rp; i++) {
            state = state.map((s, j) => (s + ark[i][j]) % p);
            if (i < rf / 2 || i >= rf / 2 + rp) state = state.map(s => field.exp(s, alpha));
            else state[m - 1] = field.exp(state[m - 1], alpha);
            state = matrix.map(row => row.reduce((acc, a, j) => (acc + a * state[j]) % p, 0n));
        }
        return state.slice(0, 2);
    };
    let handle = null;
    hash.field = field;
    hash.stateWidth = m;
    /** the gs_hades of this parameter set on the field's context (a BigInt): constants uploaded once, on first use */
    hash.handle = function () {
        if (handle === null) {
            needDevice(field);
            const out = Buffer.alloc(8);
            field.lib.call('gs_hades_create', field.ctx, m, rf, rp, alpha, field.packLe([].concat(...ark)), field.packLe([].concat(...matrix)), out);
            handle = out.readBigUInt64LE(0);
            if (registry) registry.register(hash, { lib: field.lib, ctx: field.ctx, handle });
        }
        return handle;
    };
    /** one permutation per row of a device Matrix (or of rows of BigInts): a Matrix of rowCount x digest */
    hash.hashMany = function (rows, digest = 2) {
        needDevice(field);
        if (!(rows instanceof Matrix)) rows = field.newMatrixFrom(rows);
        field._own(rows);
        const out = new Matrix(field, rows.rowCount, digest);
        field.lib.call('gs_hades_hash', field.ctx, hash.handle(), rows.ptr, rows.rowCount, rows.colCount, digest, out.ptr);
        return out;
    };
    return hash;
}

class DeviceTree {
    constructor(values, hash, digest) {
        const field = hash.field;
        if (!field || !hash.handle) throw new Error('the hash function must come from createHash of js/hades.js');
        needDevice(field);
        let src = values;
        if (Array.isArray(values)) src = field.newMatrixFrom(digest === 1 ? values.map(v => [v]) : values);
        field._own(src);
        const n = src instanceof Vector ? src.length : src.rowCount;
        if ((src instanceof Vector ? 1 : src.colCount) !== digest) throw new Error(`the leaves have ${digest} element${digest > 1 ? 's' : ''} each`);
        this.field = field; this.hash = hash; this.digest = digest; this.leafCount = n;
        this.depth = Math.round(Math.log2(n));
        this.deviceNodes = new Matrix(field, 2 * n, digest);
        field.lib.call('gs_hades_merkle', field.ctx, hash.handle(), src.ptr, n, digest, this.deviceNodes.ptr);
    }
    _shape(row) { return this.digest === 1 ? row[0] : row; }
    get nodes() { const rows = this.deviceNodes.toValues().map(r => this._shape(r)); rows[0] = undefined; return rows; }
    get root() { return this._shape(this.deviceNodes.row(1).toValues()); }
    prove(index) { return this.proveMany([index])[0]; }
    /** prove(index) for every index (repeats allowed): one launch, one read-back */
    proveMany(indexes) {
        if (!indexes.length) return [];
        const per = this.depth + 1, out = new Matrix(this.field, indexes.length * per, this.digest);
        this.field.lib.call('gs_hades_merkle_paths', this.field.ctx, this.deviceNodes.ptr, this.leafCount, this.digest, indexes, indexes.length, out.ptr);
        const rows = out.toValues().map(r => this._shape(r));
        return indexes.map((_, k) => rows.slice(k * per, (k + 1) * per));
    }
}

// a path against a root, for nodes of `digest` elements: level by level, the running value on the side the index bit says
function verifyPath(root, index, proof, hash, digest) {
    const listed = v => (digest === 1 ? [v] : v);
    let v = listed(proof[0]);
    for (let level = 1; level < proof.length; level++) {
        const sibling = listed(proof[level]), onRight = Math.floor(index / 2 ** (level - 1)) % 2 === 1;
        v = hash(onRight ? sibling.concat(v) : v.concat(sibling)).slice(0, digest);
    }
    const want = listed(root);
    return v.every((x, i) => x === want[i]);
}

class MerkleTree extends DeviceTree {      // utils.ts:126-167: nodes of two elements
    constructor(values, hash) { super(values, hash, 2); }
    static verify(root, index, proof, hash) { return verifyPath(root, index, proof, hash, 2); }
}

class MerkleTree2 extends DeviceTree {     // utils.ts:169-210: nodes of one element
    constructor(values, hash) { super(values, hash, 1); }
    static verify(root, index, proof, hash) { return verifyPath(root, index, proof, hash, 1); }
}

module.exports = { createHash, getRoundConstants, getMdsMatrix, MerkleTree, MerkleTree2 };
