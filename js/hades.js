'use strict';
// js/hades.js — the Poseidon helpers of the reference's examples/poseidon/utils.ts with the bulk work on the device
// (include/gstark_hades.h through the addon's table): createHash(field, exp, rf, rp, stateWidth, rc?) returns the example's hash function
// (BigInt arithmetic on the host, as upstream) which also carries .hashMany(matrix, digest) — one permutation per row in one launch —,
// .absorb(inputs, digest, rate) — a record of any length, on the host — and .absorbMany(rows, digest, rate, columns) — one record per
// row, or per column, in one launch (include/gstark_absorb.h) —,
// and MerkleTree / MerkleTree2 have the example's members (nodes, root, prove, static verify) plus proveMany(indexes) and update /
// updateMany(indexes, leaves): the tree is built and updated by the device, the paths of any number of leaves and the witnesses of any
// number of updates come back in one read-back; static pathRoots / verifyMany / verifyUpdates (include/gstark_tree_verify.h) check batches
// of paths and of update records on the device, one launch for all levels.  `field` is a PrimeField of js/galois.js.  A field whose
// library lacks the entry points (they are optional on an implementation of the ABI) makes the device members throw an Error saying so.
const crypto = require('crypto');
const { Matrix, Vector } = require('./galois.js');
const { destroyRegistry, needDevice: needDeviceOf, lazyHandle, hashMany, absorbHost, absorbMany, DeviceTree, SparseDeviceTree, verifyPath, installVerify } = require('./field_tree.js');

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

const registry = destroyRegistry('gs_hades_destroy');
const needDevice = field => needDeviceOf(field, 'hades', 'Poseidon');

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

    const permute = function (state) {
        for (let i = 0; i < rf + rp; i++) {
            state = state.map((s, j) => (s + ark[i][j]) % p);
            if (i < rf / 2 || i >= rf / 2 + rp) state = state.map(s => field.exp(s, alpha));
            else state[m - 1] = field.exp(state[m - 1], alpha);
            state = matrix.map(row => row.reduce((acc, a, j) => (acc + a * state[j]) % p, 0n));
        }
        return state;
    };
    const hash = function (inputs) {
        if (!(inputs.length > 0 && inputs.length < m)) throw new Error(`hash: ${inputs.length} inputs do not fit a state of ${m}`);
        const state = inputs.map(v => field.mod(BigInt(v)));
        while (state.length < m) state.push(0n);
        return permute(state).slice(0, 2);
    };
    hash.field = field;
    hash.stateWidth = m;
    /** the gs_hades of this parameter set on the field's context (a BigInt): constants uploaded once, on first use */
    hash.handle = lazyHandle(field, needDevice, registry, () => hash, out =>
        field.lib.call('gs_hades_create', field.ctx, m, rf, rp, alpha, field.packLe([].concat(...ark)), field.packLe([].concat(...matrix)), out));
    /** one permutation per row of a device Matrix (or of rows of BigInts): a Matrix of rowCount x digest */
    hash.hashMany = function (rows, digest = 2) {
        needDevice(field);
        return hashMany(field, 'gs_hades_hash', hash.handle(), rows, digest);
    };
    /** the digest of a record of any length (BigInts, on the host): the length in the first capacity element, `rate` inputs ADDED per
     *  permutation (include/gstark_absorb.h).  On purpose NOT hash(inputs) for short inputs: [a] and [a, 0] have different digests */
    hash.absorb = (inputs, digest = 2, rate) => absorbHost(field, m, permute, inputs, digest, rate);
    /** absorb for every row of a device Matrix of count x L (or of rows of BigInts), one launch; columns: every column of an L x count Matrix */
    hash.absorbMany = (rows, digest = 2, rate, columns = false) => absorbMany(field, 'gs_hades_absorb', hash.handle, m, rows, digest, rate, columns);
    return hash;
}

class HadesTree extends DeviceTree {
    constructor(values, hash, digest) {
        const field = hash.field;
        if (!field || !hash.handle) throw new Error('the hash function must come from createHash of js/hades.js');
        needDevice(field);
        let src = values;
        if (Array.isArray(values)) src = field.newMatrixFrom(digest === 1 ? values.map(v => [v]) : values);
        field._own(src);
        if ((src instanceof Vector ? 1 : src.colCount) !== digest) throw new Error(`the leaves have ${digest} element${digest > 1 ? 's' : ''} each`);
        super(field, hash.handle(), digest, src, count => new Matrix(field, count, digest),
            (handle, leaves, n, nodes) => field.lib.call('gs_hades_merkle', field.ctx, handle, leaves.ptr, n, digest, nodes.ptr),
            { symbol: 'gs_hades_merkle_update', call: (handle, nodes, n, indexes, leaves, count, before, roots) =>
                field.lib.call('gs_hades_merkle_update', field.ctx, handle, nodes.ptr, n, digest, indexes, leaves.ptr, count, before.ptr, roots.ptr) });
        this.hash = hash;
    }
}

class MerkleTree extends HadesTree {      // utils.ts:126-167: nodes of two elements
    constructor(values, hash) { super(values, hash, 2); }
    static verify(root, index, proof, hash) {
        return verifyPath(root, index, proof, (left, right) => hash(left.concat(right)).slice(0, 2), (a, b) => a.every((x, i) => x === b[i]));
    }
}

class MerkleTree2 extends HadesTree {     // utils.ts:169-210: nodes of one element
    constructor(values, hash) { super(values, hash, 1); }
    static verify(root, index, proof, hash) { return verifyPath(root, index, proof, (left, right) => hash([left, right])[0]); }
}

/** the sparse tree of 2^depth leaves (depth 1 .. 36) over the same node function (include/gstark_sparse_tree.h; js/field_tree.js) */
class HadesSparseTree extends SparseDeviceTree {
    constructor(depth, hash, digest, empty, slotsHint = 1024) {
        const field = hash && hash.field;
        if (!field || !hash.handle) throw new Error('the hash function must come from createHash of js/hades.js');
        if (2 * digest >= hash.stateWidth) throw new Error(`nodes of ${digest} elements: two of them do not fit a state of ${hash.stateWidth} beside its capacity`);
        super(field, hash, depth, digest, empty, slotsHint, { symbol: 'gs_hades_sparse_create', create: (handle, d, emptyBytes, hint, out) =>
            field.lib.call('gs_hades_sparse_create', field.ctx, handle, d, digest, emptyBytes, hint, out) });
    }
}

class SparseMerkleTree extends HadesSparseTree {      // the shape of MerkleTree: nodes of two elements
    constructor(depth, hash, empty, slotsHint) { super(depth, hash, 2, empty, slotsHint); }
    static verify(root, index, proof, hash) { return MerkleTree.verify(root, index, proof, hash); }
}

class SparseMerkleTree2 extends HadesSparseTree {     // the shape of MerkleTree2: nodes of one element
    constructor(depth, hash, empty, slotsHint) { super(depth, hash, 1, empty, slotsHint); }
    static verify(root, index, proof, hash) { return MerkleTree2.verify(root, index, proof, hash); }
}

// static pathRoots(hash, indexes, proofs, leaves?), verifyMany(root, indexes, proofs, hash), verifyUpdates(oldRoot, indexes, leaves, records, hash)
for (const [cls, digest] of [[MerkleTree, 2], [MerkleTree2, 1], [SparseMerkleTree, 2], [SparseMerkleTree2, 1]]) {
    installVerify(cls, { digest, symbol: 'gs_hades_merkle_path_roots', call: (field, handle, paths, depth, indexes, leaves, count, roots) =>
        field.lib.call('gs_hades_merkle_path_roots', field.ctx, handle, paths.ptr, depth, digest, indexes, leaves, count, roots.ptr) });
}

module.exports = { createHash, getRoundConstants, getMdsMatrix, MerkleTree, MerkleTree2, SparseMerkleTree, SparseMerkleTree2 };
