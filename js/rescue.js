'use strict';
// js/rescue.js — the Rescue helpers of the reference's examples/rescue/utils.ts with the bulk work on the device
// (include/gstark_rescue.h through the addon's table): createRescue(field, alpha, invAlpha, registers, rounds, mds, constants) has the
// members of the example's Rescue class (unrollConstants, groupConstants, sponge, modifiedSponge: BigInt arithmetic on the host, as
// upstream) and .hash2(v1, v2) = makeHashFunction, plus .hashMany(matrix, digest, modified, form) — one permutation per row in one
// launch —, .absorb(inputs, digest, rate, modified) and .absorbMany(rows, digest, rate, columns, modified) — records of any length, one
// per row or per column (include/gstark_absorb.h) — and .merkleTree(values): the example's MerkleTree (nodes, root, prove, static verify) built by the device, with
// proveMany(indexes) in one read-back and static pathRoots / verifyMany / verifyUpdates over the rescue object (include/gstark_tree_verify.h:
// batches of paths and of update records checked on the device).  `field` is a PrimeField of js/galois.js.  A field whose library lacks the entry points (they
// are optional on an implementation of the ABI) makes the device members throw an Error saying so.
const { Vector } = require('./galois.js');
const { destroyRegistry, needDevice: needDeviceOf, lazyHandle, hashMany, absorbHost, absorbMany, DeviceTree, SparseDeviceTree, verifyPath, installVerify } = require('./field_tree.js');

const registry = destroyRegistry('gs_rescue_destroy');
const needDevice = field => needDeviceOf(field, 'rescue', 'Rescue');

/** new Rescue(...) of utils.ts:33; invAlpha may be negative, as in the examples */
function createRescue(field, alpha, invAlpha, registers, rounds, mds, constants) {
    const m = registers, p = field.modulus;
    alpha = BigInt(alpha); invAlpha = BigInt(invAlpha);
    if (!(m >= 2 && m <= 8)) throw new Error(`createRescue: a state of ${m} elements is outside 2 .. 8`);
    if (!(rounds >= 1)) throw new Error(`createRescue: ${rounds} rounds (at least 1)`);
    if (alpha < 2n || alpha >> 64n) throw new Error(`createRescue: alpha ${alpha} is outside 2 .. 2^64 - 1`);
    const invExponent = invAlpha > 0n ? invAlpha : p - 1n + invAlpha;          // (1/x)^|invAlpha| for every x, 0 -> 0
    if (invExponent < 1n || invExponent >= p - 1n) throw new Error('createRescue: the inverse exponent is outside 1 .. p - 2');
    const matrix = mds.map(row => row.map(v => field.mod(BigInt(v)))), c = constants.map(v => field.mod(BigInt(v)));
    if (matrix.length !== m || matrix.some(row => row.length !== m)) throw new Error(`createRescue: the matrix has ${m} rows of ${m} values`);
    if (c.length !== m * (m + 2)) throw new Error(`createRescue: ${m * (m + 2)} key constants are needed`);
    const iConstants = c.slice(0, m), cConstants = c.slice(m + m * m), cMatrix = [];
    for (let i = 0; i < m; i++) cMatrix.push(c.slice(m + i * m, m + (i + 1) * m));
    const vadd = (a, b) => a.map((x, i) => (x + b[i]) % p);
    const mmul = (a, v) => a.map(row => row.reduce((acc, x, j) => (acc + x * v[j]) % p, 0n));
    const half = (state, e, key) => vadd(mmul(matrix, state.map(x => field.exp(x, e))), key);
    const padded = inputs => {
        if (!(inputs.length > 0 && inputs.length <= m)) throw new Error(`${inputs.length} inputs do not fit a state of ${m}`);
        const state = inputs.map(v => field.mod(BigInt(v)));
        while (state.length < m) state.push(0n);
        return state;
    };
    let keys = null;

    const rescue = {
        field, alpha, invAlpha, invExponent, registers: m, rounds, mds: matrix,
        unrollConstants() {      // utils.ts:128-159
            let state = iConstants.slice(), injection = iConstants;
            const result = [state.slice()];
            for (let r = 0; r <= rounds; r++) {
                for (const e of [invExponent, alpha]) {
                    injection = vadd(mmul(cMatrix, injection), cConstants);
                    state = half(state, e, injection);
                    result.push(state.slice());
                }
            }
            return result;
        },
        get keys() { if (keys === null) keys = rescue.unrollConstants(); return keys; },
        groupConstants(k = rescue.keys) {      // utils.ts:161-180
            const roundConstants = [];
            for (let j = 0; j < 2 * m; j++) roundConstants.push(new Array(rounds));
            for (let i = 0; i < rounds; i++) {
                for (let j = 0; j < m; j++) { roundConstants[j][i] = k[2 + 2 * i][j]; roundConstants[m + j][i] = k[3 + 2 * i][j]; }
            }
            return { initialConstants: [...k[0], ...k[1]], roundConstants };
        },
        sponge(inputs, k = rescue.keys) {      // utils.ts:49-88
            let state = padded(inputs);
            const trace = [state.slice()];
            state = vadd(state, k[0]);
            trace.push(state.slice());
            for (let r = 0; r < rounds; r++) {
                state = half(state, invExponent, k[2 * r + 1]); trace.push(state.slice());
                state = half(state, alpha, k[2 * r + 2]); trace.push(state.slice());
            }
            return { hash: state.slice(0, inputs.length), trace };
        },
        modifiedSponge(inputs, k = rescue.keys) {      // utils.ts:90-124
            let state = padded(inputs);
            const trace = [state.slice()];
            for (let r = 0; r < rounds - 1; r++) {
                state = half(state, alpha, k[2 * r + 2]); trace.push(state.slice());
                state = half(state, invExponent, k[2 * r + 3]); trace.push(state.slice());
            }
            return { hash: state.slice(0, inputs.length), trace };
        },
        /** makeHashFunction (utils.ts:11-15) */
        hash2(v1, v2) {
            const inputs = [v1, v2];
            while (inputs.length < m) inputs.push(0n);
            return rescue.modifiedSponge(inputs).hash[0];
        },
        /** the gs_rescue of this parameter set on the field's context (a BigInt): constants uploaded once, on first use */
        handle: lazyHandle(field, needDevice, registry, () => rescue, out =>
            field.lib.call('gs_rescue_create', field.ctx, m, rounds, alpha, field.packLe([invExponent]), field.packLe([].concat(...matrix)),
                field.packLe([].concat(...rescue.keys)), out)),
        /** one permutation per row of a device Matrix (or of rows of BigInts): a Matrix of rowCount x digest */
        hashMany(rows, digest = 1, modified = true, form = 0) {
            needDevice(field);
            return hashMany(field, 'gs_rescue_hash', rescue.handle(), rows, digest, modified ? 1 : 0, form);
        },
        /** the digest of a record of any length (BigInts, on the host): the length in the first capacity element, `rate` inputs ADDED per
         *  permutation — the whole last state of modifiedSponge, or of sponge (include/gstark_absorb.h).  On purpose NOT the sponge of
         *  short inputs: [a] and [a, 0] have different digests */
        absorb(inputs, digest = 1, rate, modified = true) {
            const permute = state => { const t = (modified ? rescue.modifiedSponge(state) : rescue.sponge(state)).trace; return t[t.length - 1]; };
            return absorbHost(field, m, permute, inputs, digest, rate);
        },
        /** absorb for every row of a device Matrix of count x L (or of rows of BigInts), one launch; columns: every column of an L x count Matrix */
        absorbMany(rows, digest = 1, rate, columns = false, modified = true) {
            return absorbMany(field, 'gs_rescue_absorb', rescue.handle, m, rows, digest, rate, columns, modified ? 1 : 0);
        },
        merkleTree(values) { return new MerkleTree(values, rescue); },
        /** the sparse tree of 2^depth leaves (depth 1 .. 36) that all hold `empty` until set (include/gstark_sparse_tree.h) */
        sparseMerkleTree(depth, empty, slotsHint) { return new SparseMerkleTree(depth, rescue, empty, slotsHint); },
    };
    return rescue;
}

class MerkleTree extends DeviceTree {      // utils.ts:232-273, built by the device
    constructor(values, rescue) {
        const field = rescue.field;
        if (!field || !rescue.handle) throw new Error('the hash must come from createRescue of js/rescue.js');
        needDevice(field);
        const src = Array.isArray(values) ? field.newVectorFrom(values) : values;
        if (!(src instanceof Vector)) throw new Error('the leaves are an array of BigInts or a Vector');
        field._own(src);
        super(field, rescue.handle(), 1, src, count => new Vector(field, count),
            (handle, leaves, n, nodes) => field.lib.call('gs_rescue_merkle', field.ctx, handle, leaves.ptr, n, nodes.ptr),
            { symbol: 'gs_rescue_merkle_update', call: (handle, nodes, n, indexes, leaves, count, before, roots) =>
                field.lib.call('gs_rescue_merkle_update', field.ctx, handle, nodes.ptr, n, indexes, leaves.ptr, count, before.ptr, roots.ptr) });
        this.rescue = rescue;
    }
    /** hash: a function of two values (rescue.hash2) */
    static verify(root, index, proof, hash) { return verifyPath(root, index, proof, hash); }
}

class SparseMerkleTree extends SparseDeviceTree {      // the sparse form of MerkleTree: nodes of one element
    constructor(depth, rescue, empty, slotsHint = 1024) {
        const field = rescue && rescue.field;
        if (!field || !rescue.handle) throw new Error('the hash must come from createRescue of js/rescue.js');
        if (rescue.registers < 3) throw new Error(`two nodes do not fit a state of ${rescue.registers} beside its capacity (3 .. 8 registers)`);
        super(field, rescue, depth, 1, empty, slotsHint, { symbol: 'gs_rescue_sparse_create', create: (handle, d, emptyBytes, hint, out) =>
            field.lib.call('gs_rescue_sparse_create', field.ctx, handle, d, emptyBytes, hint, out) });
        this.rescue = rescue;
    }
    static verify(root, index, proof, hash) { return verifyPath(root, index, proof, hash); }
}

// static pathRoots(rescue, indexes, proofs, leaves?), verifyMany(root, indexes, proofs, rescue), verifyUpdates(oldRoot, indexes, leaves, records, rescue)
for (const cls of [MerkleTree, SparseMerkleTree]) installVerify(cls, { digest: 1, symbol: 'gs_rescue_merkle_path_roots', call: (field, handle, paths, depth, indexes, leaves, count, roots) =>
    field.lib.call('gs_rescue_merkle_path_roots', field.ctx, handle, paths.ptr, depth, indexes, leaves, count, roots.ptr) });

module.exports = { createRescue, MerkleTree, SparseMerkleTree };
