'use strict';
// js/merkle.js — drop-in for the `@guildofweavers/merkle` surface genSTARK uses: createHash(algorithm, useWasm) ->
// Hash {digest, merge, mergeVectorRows, digestValues, digestSize, isOptimized}; MerkleTree {create, root, proveBatch,
// verifyBatch}.  Call sites: lib/Stark.ts:50,115,118,150,206; lib/components/LowDegreeProver.ts:45-53,163-164,201-217.
const { Vector } = require('./galois');
const { defaultField } = require('./context');

const ALGS = { sha256: 0, blake2s256: 1 };
const DIGEST = 32;

class Hash {
    /** field: the field whose library hashes (its vectors, its device context).  Without one, the hash follows the field of the vectors it
     *  is given, and hashes bytes in the default field's library (the upstream createHash(algorithm) knows no field) */
    constructor(algorithm, field) {
        if (!(algorithm in ALGS)) throw new TypeError(`Hash algorithm ${algorithm} is not supported`);
        this.algorithm = algorithm; this.alg = ALGS[algorithm]; this.field = field;
        this.digestSize = DIGEST; this.isOptimized = true;
    }
    /** the field an operation on `x` (a Vector / Matrix, or nothing) runs in */
    _fieldFor(x) {
        const of = x && x.field;
        if (this.field) {
            if (of && of.lib !== this.field.lib) throw new TypeError(`a vector of the field of ${of.modulus} elements was passed to a hash of the field of ${this.field.modulus} elements`);
            return this.field;
        }
        return of || defaultField();
    }
    digest(value) { const f = this._fieldFor(), out = Buffer.alloc(DIGEST); f.lib.call('gs_hash_digest', f.ctx, this.alg, value, value.length, out); return out; }
    merge(a, b) { return this.digest(Buffer.concat([a, b])); }
    mergeVectorRows(vectors) {
        const f = this._fieldFor(vectors[0]);
        for (const v of vectors) if (v.field && v.field.lib !== f.lib) throw new TypeError(`vectors of the fields of ${v.field.modulus} and ${f.modulus} elements were hashed together`);
        const n = vectors[0].length, out = new Vector(f, n, undefined, 0n, DIGEST);
        f.lib.call('gs_hash_merge_rows', f.ctx, this.alg, vectors.map(v => v.ptr), vectors.length, n, out.ptr);
        return out;
    }
    digestValues(values, valueSize) {
        const f = this._fieldFor(Buffer.isBuffer(values) ? undefined : values);
        let src = values, bytes;
        if (Buffer.isBuffer(values)) {
            src = new Vector(f, values.length, undefined, 0n, 1);
            f.lib.call('gs_upload', f.ctx, src.ptr, values, values.length);
            bytes = values.length;
        } else bytes = values.rowCount !== undefined ? values.rowCount * values.colCount * values.elementSize : values.byteLength;
        const count = bytes / valueSize, out = new Vector(f, count, undefined, 0n, DIGEST);
        f.lib.call('gs_hash_digest_values', f.ctx, this.alg, src.ptr, valueSize, count, out.ptr);
        return out;
    }
}
// upstream signature is createHash(algorithm, useWasm); the field object carries the library and the device context here (none: the
// field of the vectors hashed, the default field for bytes)
function createHash(algorithm, field) { return new Hash(algorithm, field); }

function normalize(indexes) {
    const out = new Set();
    for (const ix of indexes.slice().sort((a, b) => a - b)) out.add(ix - (ix & 1));
    return Array.from(out);
}

class MerkleTree {
    constructor(values, nodes, hash) { this.values = values; this.nodes = nodes; this.hash = hash; this.depth = Math.log2(values.length); }
    static create(leaves, hash) {
        const f = hash._fieldFor(leaves);
        const nodes = new Vector(f, leaves.length, undefined, 0n, DIGEST);
        f.lib.call('gs_merkle_build', f.ctx, hash.alg, leaves.ptr, leaves.length, nodes.ptr);
        return new MerkleTree(leaves, nodes, hash);
    }
    get root() { if (!this._root) this._root = this.nodes.toBuffer(1, 1); return this._root; }
    proveBatch(indexes) {
        const f = this.nodes.field;
        const r = f.lib.merkleProveBatch(f.ctx, this.values.ptr, this.nodes.ptr, this.values.length, indexes);
        const values = indexes.map((_, i) => r.values.slice(i * DIGEST, (i + 1) * DIGEST));
        const nodes = []; let o = 0;
        for (const k of r.colLens) { const col = []; for (let t = 0; t < k; t++, o++) col.push(r.nodes.slice(o * DIGEST, (o + 1) * DIGEST)); nodes.push(col); }
        return { values, nodes, depth: this.depth };
    }
    static verifyBatch(root, indexes, proof, hash) {
        const offset = 2 ** proof.depth, indexMap = new Map();
        indexes.forEach((ix, i) => indexMap.set(ix, i));
        if (indexMap.size !== indexes.length) return false;
        const norm = normalize(indexes);
        if (norm.length !== proof.nodes.length) return false;
        const v = new Map(), ptr = new Array(norm.length).fill(0);
        let next = [];
        for (let i = 0; i < norm.length; i++) {
            const ix = norm[i], i1 = indexMap.get(ix), i2 = indexMap.get(ix + 1);
            let v1, v2;
            if (i1 !== undefined && i2 !== undefined) { v1 = proof.values[i1]; v2 = proof.values[i2]; }
            else if (i1 !== undefined) { v1 = proof.values[i1]; v2 = proof.nodes[i][0]; ptr[i] = 1; }
            else { v1 = proof.nodes[i][0]; v2 = proof.values[i2]; ptr[i] = 1; }
            if (!v1 || !v2) return false;
            const parent = (offset + ix) >> 1;
            v.set(parent, hash.merge(v1, v2)); next.push(parent);
        }
        for (let d = proof.depth - 1; d > 0; d--) {
            const cur = next; next = [];
            for (let i = 0; i < cur.length; i++) {
                const node = cur[i], sib = node ^ 1;
                let s;
                if (i + 1 < cur.length && cur[i + 1] === sib) { s = v.get(sib); i++; }
                else { s = proof.nodes[i][ptr[i]]; ptr[i]++; }
                const me = v.get(node);
                if (!me || !s) return false;
                v.set(node >> 1, (node & 1) ? hash.merge(s, me) : hash.merge(me, s));
                next.push(node >> 1);
            }
        }
        return Buffer.compare(v.get(1), root) === 0;
    }
}

module.exports = { createHash, Hash, MerkleTree };
