'use strict';
// js/galois.js — drop-in for the `@guildofweavers/galois` surface genSTARK uses (SURVEY.md section 8b):
// createPrimeField(modulus) -> FiniteField whose Vector / Matrix objects live in MI355X HBM and whose vector,
// matrix and polynomial members each forward to one entry point of include/gstark.h through the N-API shim
// (napi/gstark_napi.node -> libgstark_hip.so).  Scalar bigint members stay JS BigInt arithmetic, as upstream.
const crypto = require('crypto');
const path = require('path');

const MODULUS = 2n ** 128n - 9n * 2n ** 32n + 1n;
// one build flavour of the library per field (genstark_amd/csrc/build.sh).  A process may work in several fields: each modulus resolves
// to its library, which is opened once (the addon's open(): a library object with its own contexts and driver bindings) and shared by
// every PrimeField of that modulus
const LIBRARIES = new Map([
    [MODULUS, 'libgstark_hip.so'],
    [2n ** 64n - 21n * 2n ** 30n + 1n, 'libgstark_hip_q64.so'], [2n ** 32n - 3n * 2n ** 25n + 1n, 'libgstark_hip_q32.so'], [96769n, 'libgstark_hip_q17.so'],
    [2n ** 256n - 351n * 2n ** 32n + 1n, 'libgstark_hip_p256.so'], [2n ** 224n - 2n ** 96n + 1n, 'libgstark_hip_p224.so'],
]);
const RUNTIME_LIBRARY = 'libgstark_hip_rt.so';

// deterministic Miller-Rabin (the first 24 primes as bases: a proof of primality below 3.3e24, a strong probable-prime test above)
const MR_BASES = [2n, 3n, 5n, 7n, 11n, 13n, 17n, 19n, 23n, 29n, 31n, 37n, 41n, 43n, 47n, 53n, 59n, 61n, 67n, 71n, 73n, 79n, 83n, 89n];
function powMod(b, e, m) { let r = 1n; b %= m; while (e > 0n) { if (e & 1n) r = r * b % m; b = b * b % m; e >>= 1n; } return r; }
function isProbablePrime(n) {
    if (n < 2n) return false;
    for (const p of MR_BASES) { if (n === p) return true; if (n % p === 0n) return false; }
    let d = n - 1n, s = 0;
    while (!(d & 1n)) { d >>= 1n; s++; }
    for (const a of MR_BASES) {
        let x = powMod(a, d, n);
        if (x === 1n || x === n - 1n) continue;
        let i = 1;
        for (; i < s; i++) { x = x * x % n; if (x === n - 1n) break; }
        if (i === s) return false;
    }
    return true;
}

let addonModule = null;
function addon() {      // GSTARK_ADDON: an instrumented build (tools/build_sanitized.sh)
    if (!addonModule) addonModule = require(process.env.GSTARK_ADDON || path.join(__dirname, '..', 'napi', 'gstark_napi.node'));
    return addonModule;
}
const OPENED = new Map();        // library path -> { lib, modulus, elementSize }
const BY_MODULUS = new Map();    // modulus -> the same record
let runtimeModulus = null;       // the runtime-modulus library's field (its constants are per process: one such modulus per process)
let firstLib = null;             // the default field's library: the first one opened

function openLibrary(file, setModulus, wanted) {
    let rec = OPENED.get(file);
    if (!rec) {
        const lib = addon().open(file);
        if (lib.backend !== 'hip-gfx950' && process.env.GSTARK_ALLOW_TEST_DOUBLE !== '1') {
            throw new Error(`refusing backend ${lib.backend}: the product path runs on hip-gfx950 only (no CPU fallback)`);
        }
        if (setModulus) {
            const bytes = Buffer.alloc(32);
            let x = wanted;
            for (let i = 0; i < 32; i++) { bytes[i] = Number(x & 0xFFn); x >>= 8n; }
            lib.call('gs_set_modulus', bytes, 32);
        }
        const info = lib.fieldInfo();
        rec = { lib, elementSize: info.elementSize, modulus: fromLe(info.modulus, 0, info.elementSize) };
        OPENED.set(file, rec);
        if (!firstLib) firstLib = rec;
    }
    return rec;
}

/** modulus -> { lib, modulus, elementSize }: the library computing in that field, opened on first use */
function libraryFor(modulus) {
    const wanted = modulus === undefined ? (firstLib ? firstLib.modulus : MODULUS) : BigInt(modulus);
    const known = BY_MODULUS.get(wanted);
    if (known) return known;
    let rec;
    if (process.env.GSTARK_LIB) {
        // one library named for every field (an instrumented or test build): it computes in one field, a second modulus is refused
        // (GSTARK_SET_MODULUS=1: GSTARK_LIB names a runtime-modulus library — the tests' double)
        const setModulus = process.env.GSTARK_SET_MODULUS === '1';
        if (setModulus && !OPENED.has(process.env.GSTARK_LIB)) checkRuntimeModulus(wanted);
        rec = openLibrary(process.env.GSTARK_LIB, setModulus, wanted);
        if (wanted !== rec.modulus) throw new TypeError(`the loaded library computes in the field of ${rec.modulus} elements, not ${wanted} (one field per process)`);
    } else {
        // a modulus none of the fixed builds knows: the runtime-modulus build (gs_set_modulus: any odd prime below 2^256, once per process)
        const runtime = !LIBRARIES.has(wanted);
        if (runtime) {
            checkRuntimeModulus(wanted);
            if (runtimeModulus !== null && runtimeModulus !== wanted) {
                throw new TypeError(`the runtime-modulus library already computes in the field of ${runtimeModulus} elements; it cannot also take ${wanted} (one runtime modulus per process)`);
            }
        }
        const name = runtime ? RUNTIME_LIBRARY : LIBRARIES.get(wanted);
        // GSTARK_LIB_DIR (tests): every flavour from one directory under the CPU oracle's file names (oracle/Makefile: liboracle*.so)
        const file = process.env.GSTARK_LIB_DIR ? path.join(process.env.GSTARK_LIB_DIR, name.replace('libgstark_hip', 'liboracle'))
                                               : path.join(__dirname, '..', 'genstark_amd', 'csrc', name);
        rec = openLibrary(file, runtime, wanted);
        if (runtime) runtimeModulus = wanted;
        if (wanted !== rec.modulus) throw new TypeError(`the library ${file} computes in the field of ${rec.modulus} elements, not ${wanted}`);
    }
    BY_MODULUS.set(wanted, rec);
    return rec;
}
function checkRuntimeModulus(q) {
    if (q < 3n || q % 2n === 0n || q >> 256n) throw new TypeError(`no build of the library for the field of ${q} elements`);
    if (!isProbablePrime(q)) throw new TypeError(`${q} is not prime: no field of ${q} elements`);
}

/** the library object of a field (the default field's when no modulus is given): its members are the addon's, on that library */
function native(modulus) { return libraryFor(modulus).lib; }

// bigint <-> little-endian bytes (lib/utils/serialization.ts:140-146 layout), a 64-bit word at a time: a column of an input register is
// 10^4..10^5 of these per proof, and a byte at a time they cost more than the proof (element sizes are 16 or 32 bytes).  The module-level
// helpers take the element size of a field given as their last argument, else of the default field; PrimeField has the same members.
const M64 = (1n << 64n) - 1n;
const sizeOf = field => (field && typeof field === 'object' && field.elementSize) ? field.elementSize : (firstLib ? firstLib.elementSize : 16);
function putLe(b, off, v, size) {
    let x = BigInt(v);
    for (let i = 0; i < size; i += 8) { b.writeBigUInt64LE(x & M64, off + i); x >>= 64n; }
}
function le(v, field) {  // bigint -> elementSize-byte little-endian Buffer
    const size = sizeOf(field);
    const b = Buffer.allocUnsafe(size);
    putLe(b, 0, v, size);
    return b;
}
/** values (BigInt, already reduced; or anything BigInt() takes when `mod` is given) -> ONE Buffer of their little-endian elements */
function packLe(values, mod, field) {
    const size = sizeOf(field);
    if (mod) { const reduced = new Array(values.length); for (let i = 0; i < values.length; i++) reduced[i] = mod(BigInt(values[i])); values = reduced; }
    // the addon copies the BigInts' words (napi_get_value_bigint_words: ~30 ns per element); without it — or for the handful of values
    // most calls carry — the loop below
    if (values.length >= 64 && addonModule && addonModule.packElements) return addonModule.packElements(values, size);
    const b = Buffer.allocUnsafe(values.length * size);
    for (let i = 0; i < values.length; i++) putLe(b, i * size, values[i], size);
    return b;
}
/** a Buffer of little-endian elements -> BigInt[] */
function unpackLe(raw, size) {
    if (size === undefined) size = sizeOf();
    const n = raw.length / size;
    if (n >= 64 && (size === 16 || size === 32) && addonModule && addonModule.unpackElements) return addonModule.unpackElements(raw, size);
    const out = new Array(n);
    for (let i = 0; i < n; i++) out[i] = fromLe(raw, i * size, size);
    return out;
}
function fromLe(buf, off = 0, size) {
    if (size === undefined) size = sizeOf();
    let v = 0n;
    if (size % 8 === 0) { for (let i = size - 8; i >= 0; i -= 8) v = (v << 64n) | buf.readBigUInt64LE(off + i); return v; }
    for (let i = size - 1; i >= 0; i--) v = (v << 8n) | BigInt(buf[off + i]);
    return v;
}
function sha256(value) {  // same helper as lib/components/QueryIndexGenerator.ts:61-67
    const buffer = (typeof value === 'bigint') ? Buffer.from(value.toString(16), 'hex') : value;
    return BigInt('0x' + crypto.createHash('sha256').update(buffer).digest().toString('hex'));
}

const registry = (typeof FinalizationRegistry !== 'undefined')
    ? new FinalizationRegistry(({ lib, ctx, ptr }) => { try { lib.call('gs_free', ctx, ptr); } catch (e) { /* context gone */ } })
    : null;

class DeviceBuffer {
    constructor(field, bytes) {
        this.field = field;
        this.ptr = field.lib.alloc(field.ctx, bytes > 16 ? bytes : 16);
        if (registry) registry.register(this, { lib: field.lib, ctx: field.ctx, ptr: this.ptr });
    }
}

class Vector {
    constructor(field, length, owner, offset = 0n, elementSize) {
        if (elementSize === undefined) elementSize = field.elementSize;
        this.field = field; this.length = length; this.elementSize = elementSize;
        this.owner = owner || new DeviceBuffer(field, length * elementSize);
        this.offset = offset;
        this.seriesBase = undefined;
    }
    get ptr() { return this.owner.ptr + this.offset; }
    get byteLength() { return this.length * this.elementSize; }
    toBuffer(start = 0, count) {
        count = (count === undefined) ? this.length - start : count;
        const out = Buffer.alloc(count * this.elementSize);
        if (count) this.field.lib.call('gs_download', this.field.ctx, out, this.ptr + BigInt(start * this.elementSize), out.length);
        return out;
    }
    getValue(index) { return fromLe(this.toBuffer(index, 1), 0, this.elementSize); }
    toValues() { return unpackLe(this.toBuffer(), this.elementSize); }
    copyValue(index, destination, offset) {  // lib/Stark.ts:290
        this.toBuffer(index, 1).copy(destination, offset);
        return this.elementSize;
    }
    valuesAt(indexes) {
        const out = Buffer.alloc(indexes.length * this.elementSize);
        if (indexes.length) this.field.lib.call('gs_gather', this.field.ctx, this.ptr, this.elementSize, indexes, indexes.length, out);
        return indexes.map((_, i) => out.slice(i * this.elementSize, (i + 1) * this.elementSize));
    }
}

class Matrix {
    constructor(field, rowCount, colCount, owner, offset = 0n) {
        const es = field.elementSize;
        this.field = field; this.rowCount = rowCount; this.colCount = colCount; this.elementSize = es;
        this.owner = owner || new DeviceBuffer(field, rowCount * colCount * es);
        this.offset = offset;
        this.quarticDomain = undefined;
    }
    get ptr() { return this.owner.ptr + this.offset; }
    toBuffer() {
        const out = Buffer.alloc(this.rowCount * this.colCount * this.elementSize);
        if (out.length) this.field.lib.call('gs_download', this.field.ctx, out, this.ptr, out.length);
        return out;
    }
    getValue(row, col) {
        const es = this.elementSize, out = Buffer.alloc(es);
        this.field.lib.call('gs_download', this.field.ctx, out, this.ptr + BigInt((row * this.colCount + col) * es), es);
        return fromLe(out, 0, es);
    }
    toValues() {
        const flat = unpackLe(this.toBuffer(), this.elementSize), out = [];
        for (let r = 0; r < this.rowCount; r++) out.push(flat.slice(r * this.colCount, (r + 1) * this.colCount));
        return out;
    }
    rowsToBuffers(indexes) {  // lib/components/LowDegreeProver.ts:53,214,217
        const rec = this.colCount * this.elementSize;
        const out = Buffer.alloc(indexes.length * rec);
        if (indexes.length) this.field.lib.call('gs_gather', this.field.ctx, this.ptr, rec, indexes, indexes.length, out);
        return indexes.map((_, i) => out.slice(i * rec, (i + 1) * rec));
    }
    row(r) { return new Vector(this.field, this.colCount, this.owner, this.offset + BigInt(r * this.colCount * this.elementSize)); }
}

const TREE_EVAL_FROM = 2 ** 15;     // evalPolyAtPoints(method undefined): the tree from this many coefficients and points (profiles/poly.md)

class PrimeField {
    constructor(modulus, options) {
        const rec = libraryFor(modulus);
        this.lib = rec.lib; this.modulus = rec.modulus; this.elementSize = rec.elementSize; this.isOptimized = true;
        this.zero = 0n; this.one = 1n;
        this.ctx = (options && options.ctx) || this.lib.ctxCreate((options && options.device) || 0);
    }
    // ---- this field's element bytes (the module-level le / packLe / unpackLe / fromLe with this field's element size)
    le(v) { return le(v, this); }
    packLe(values, mod) { return packLe(values, mod, this); }
    unpackLe(raw) { return unpackLe(raw, this.elementSize); }
    fromLe(buf, off = 0) { return fromLe(buf, off, this.elementSize); }
    /** every Vector / Matrix an operation takes must live in this field's library: a gs_ctx or a pointer of another never reaches it */
    _own(...xs) {
        for (const x of xs) {
            if (x && x.field && x.field.lib !== this.lib) throw new TypeError(`a vector or matrix of the field of ${x.field.modulus} elements was passed to the field of ${this.modulus} elements`);
        }
    }
    // ---- scalars
    mod(v) { return v >= 0n ? v % this.modulus : ((v % this.modulus) + this.modulus) % this.modulus; }
    add(a, b) { return this.mod(a + b); }
    sub(a, b) { return this.mod(a - b); }
    mul(a, b) { return this.mod(a * b); }
    neg(a) { return this.mod(-a); }
    exp(b, e) {
        if (e < 0n) { b = this.inv(b); e = -e; }
        let r = 1n; b = this.mod(b);
        while (e > 0n) { if (e & 1n) r = (r * b) % this.modulus; b = (b * b) % this.modulus; e >>= 1n; }
        return r;
    }
    inv(a) { return this.mod(a) === 0n ? 0n : this.exp(a, this.modulus - 2n); }
    div(a, b) { return this.mul(a, this.inv(b)); }
    prng(seed, length) {  // UNVERIFIED restatement (SURVEY appendix A.1)
        if (length === undefined) return this.mod(sha256(seed));
        const out = new Array(length); let state = sha256(seed);
        for (let i = 0; i < length; i++) { out[i] = this.mod(state); state = sha256(state); }
        return this.newVectorFrom(out);
    }
    getRootOfUnity(order) {  // UNVERIFIED restatement (SURVEY appendix A.3)
        const o = BigInt(order);
        if (o < 1n || (this.modulus - 1n) % o !== 0n) throw new Error(`the field of ${this.modulus} elements has no root of unity of order ${order}: it does not divide p - 1`);
        for (let i = 2n; i < 65536n; i++) {
            const g = this.exp(i, (this.modulus - 1n) / o);
            if (this.exp(g, o) === 1n && (o === 1n || this.exp(g, o / 2n) !== 1n)) return g;
        }
        throw new Error(`Root of unity for order ${order} was not found`);
    }
    // ---- construction
    newVector(length) { return new Vector(this, length); }
    newVectorFrom(values) {
        const v = new Vector(this, values.length);
        if (values.length) this.lib.call('gs_upload', this.ctx, v.ptr, this.packLe(values, x => this.mod(x)), values.length * this.elementSize);
        return v;
    }
    newMatrix(rows, cols) { return new Matrix(this, rows, cols); }
    newMatrixFrom(values) {
        const rows = values.length, cols = rows ? values[0].length : 0;
        const m = new Matrix(this, rows, cols);
        if (rows * cols) {
            const flat = new Array(rows * cols);
            for (let r = 0; r < rows; r++) for (let c = 0; c < cols; c++) flat[r * cols + c] = values[r][c];
            this.lib.call('gs_upload', this.ctx, m.ptr, this.packLe(flat, x => this.mod(x)), rows * cols * this.elementSize);
        }
        return m;
    }
    newMatrixFromVectors(vectors) {
        this._own(...vectors);
        // shorter rows are zero-extended (polynomials of different degrees: BoundaryConstraints.ts:84-85)
        const cols = Math.max(...vectors.map(v => v.length)); const m = new Matrix(this, vectors.length, cols);
        vectors.forEach((v, r) => {
            this.lib.call('gs_copy', this.ctx, m.ptr + BigInt(r * cols * this.elementSize), v.ptr, v.length * this.elementSize);
            if (v.length < cols) this.lib.call('gs_upload', this.ctx, m.ptr + BigInt((r * cols + v.length) * this.elementSize), Buffer.alloc((cols - v.length) * this.elementSize), (cols - v.length) * this.elementSize);
        });
        return m;
    }
    matrixRowsToVectors(m) { this._own(m); const out = []; for (let r = 0; r < m.rowCount; r++) out.push(m.row(r)); return out; }
    // ---- vector ops
    _binary(fnVec, fnScalar, a, b) {
        this._own(a, b);
        const out = new Vector(this, a.length);
        if (typeof b === 'bigint') this.lib.call(fnScalar, this.ctx, a.ptr, this.le(this.mod(b)), a.length, out.ptr);
        else {
            if (a.length !== b.length) throw new Error('Cannot combine vector elements: vectors have different lengths');
            this.lib.call(fnVec, this.ctx, a.ptr, b.ptr, a.length, out.ptr);
        }
        return out;
    }
    addVectorElements(a, b) { return this._binary('gs_vec_add', 'gs_vec_add_scalar', a, b); }
    subVectorElements(a, b) { return this._binary('gs_vec_sub', 'gs_vec_sub_scalar', a, b); }
    mulVectorElements(a, b) { return this._binary('gs_vec_mul', 'gs_vec_mul_scalar', a, b); }
    divVectorElements(a, b) {
        this._own(a, b);
        if (typeof b === 'bigint') return this.mulVectorElements(a, this.inv(b));
        const out = new Vector(this, a.length);
        this.lib.call('gs_vec_div', this.ctx, a.ptr, b.ptr, a.length, out.ptr);
        return out;
    }
    invVectorElements(a) { this._own(a); const out = new Vector(this, a.length); this.lib.call('gs_vec_inv', this.ctx, a.ptr, a.length, out.ptr); return out; }
    expVectorElements(a, e) {
        this._own(a);
        if (e < 0n) { a = this.invVectorElements(a); e = -e; }
        const out = new Vector(this, a.length); this.lib.call('gs_vec_exp', this.ctx, a.ptr, this.le(e), a.length, out.ptr); return out;
    }
    combineVectors(a, b) { this._own(a, b); const out = Buffer.alloc(this.elementSize); this.lib.call('gs_combine', this.ctx, a.ptr, b.ptr, a.length, out); return this.fromLe(out); }
    mulMatrixByVector(m, v) { // examples/poseidon/utils.ts:45
        this._own(m, v);
        const out = [];
        for (let r = 0; r < m.rowCount; r++) out.push(this.combineVectors(new Vector(this, m.colCount, m.owner, m.offset + BigInt(r * m.colCount * this.elementSize)), v));
        return this.newVectorFrom(out);
    }
    combineManyVectors(vectors, coefficients) {
        this._own(...vectors, coefficients);
        const ks = Array.isArray(coefficients) ? coefficients : coefficients.toValues();
        const out = new Vector(this, vectors[0].length);
        this.lib.call('gs_combine_many', this.ctx, vectors.map(v => v.ptr), this.packLe(ks), vectors.length, vectors[0].length, out.ptr);
        return out;
    }
    getPowerSeries(base, length) {
        const out = new Vector(this, length);
        this.lib.call('gs_power_series', this.ctx, this.le(this.mod(base)), length, out.ptr);
        out.seriesBase = this.mod(base);
        return out;
    }
    pluckVector(v, skip, times) { this._own(v); const out = new Vector(this, times); this.lib.call('gs_pluck', this.ctx, v.ptr, v.length, skip, times, out.ptr); return out; }
    transposeVector(v, columns, step = 1) {
        this._own(v);
        const rows = v.length / (columns * step);
        const m = new Matrix(this, rows, columns);
        this.lib.call('gs_transpose_vector', this.ctx, v.ptr, v.length, columns, step, m.ptr);
        if (columns === 4 && v.seriesBase !== undefined) m.quarticDomain = { omega: v.seriesBase, n: v.length, step };
        return m;
    }
    // ---- matrix ops
    transposeMatrix(m) { this._own(m); const out = new Matrix(this, m.colCount, m.rowCount); this.lib.call('gs_transpose_matrix', this.ctx, m.ptr, m.rowCount, m.colCount, out.ptr); return out; }
    joinMatrixRows(m) { this._own(m); return new Vector(this, m.rowCount * m.colCount, m.owner, m.offset); }
    subMatrixElementsFromVectors(vectors, m) {
        this._own(...vectors, m);
        const out = new Matrix(this, m.rowCount, m.colCount);
        this.lib.call('gs_sub_matrix_from_vectors', this.ctx, vectors.map(v => v.ptr), m.ptr, m.rowCount, m.colCount, out.ptr);
        return out;
    }
    divMatrixElements(a, b) { this._own(a, b); const out = new Matrix(this, a.rowCount, a.colCount); this.lib.call('gs_vec_div', this.ctx, a.ptr, b.ptr, a.rowCount * a.colCount, out.ptr); return out; }
    // ---- polynomials
    _omegaOf(roots) { return roots.seriesBase !== undefined ? roots.seriesBase : (roots.length > 1 ? roots.getValue(1) : 1n); }
    evalPolyAtRoots(poly, roots) {
        this._own(poly, roots);
        const out = new Vector(this, roots.length);
        this.lib.call('gs_eval_polys_at_roots', this.ctx, poly.ptr, 1, poly.length, this.le(this._omegaOf(roots)), roots.length, out.ptr);
        return out;
    }
    evalPolysAtRoots(polys, roots) {
        this._own(polys, roots);
        const out = new Matrix(this, polys.rowCount, roots.length);
        this.lib.call('gs_eval_polys_at_roots', this.ctx, polys.ptr, polys.rowCount, polys.colCount, this.le(this._omegaOf(roots)), roots.length, out.ptr);
        return out;
    }
    interpolateRoots(roots, ys) {
        this._own(roots, ys);
        const n = roots.length, isM = ys instanceof Matrix;
        const out = isM ? new Matrix(this, ys.rowCount, n) : new Vector(this, n);
        this.lib.call('gs_interpolate_roots', this.ctx, ys.ptr, isM ? ys.rowCount : 1, this.le(this._omegaOf(roots)), n, out.ptr);
        return out;
    }
    evalPolyAt(poly, x) { this._own(poly); const out = Buffer.alloc(this.elementSize); this.lib.call('gs_eval_poly_at', this.ctx, poly.ptr, poly.length, this.le(this.mod(x)), out); return this.fromLe(out); }
    mulPolys(a, b) {
        this._own(a, b);
        // tiny operands (BoundaryConstraints.ts:30) on the host; larger ones through the device NTT
        const la = a.length, lb = b.length;
        if (la * lb <= 4096) {
            const av = a.toValues(), bv = b.toValues(), out = new Array(la + lb - 1).fill(0n);
            for (let i = 0; i < la; i++) for (let j = 0; j < lb; j++) out[i + j] = this.mod(out[i + j] + av[i] * bv[j]);
            return this.newVectorFrom(out);
        }
        let n = 1; while (n < la + lb - 1) n <<= 1;
        const roots = this.getPowerSeries(this.getRootOfUnity(n), n);
        const full = this.interpolateRoots(roots, this.mulVectorElements(this.evalPolyAtRoots(a, roots), this.evalPolyAtRoots(b, roots)));
        return new Vector(this, la + lb - 1, full.owner, full.offset);
    }
    padPoly(v, length) {
        this._own(v);
        if (v.length === length) return v;
        const out = new Vector(this, length);
        this.lib.call('gs_copy', this.ctx, out.ptr, v.ptr, v.length * this.elementSize);
        const zeros = Buffer.alloc((length - v.length) * this.elementSize);
        this.lib.call('gs_upload', this.ctx, out.ptr + BigInt(v.length * this.elementSize), zeros, zeros.length);
        return out;
    }
    addPolys(a, b) { const n = Math.max(a.length, b.length); return this.addVectorElements(this.padPoly(a, n), this.padPoly(b, n)); }
    subPolys(a, b) { const n = Math.max(a.length, b.length); return this.subVectorElements(this.padPoly(a, n), this.padPoly(b, n)); }
    mulPolyByConstant(a, c) { return this.mulVectorElements(a, this.mod(c)); }
    // ---- square roots (include/gstark_sqrt.h, csrc/sqrt.hip).  sqrt is host BigInt arithmetic (Tonelli-Shanks); the vector members are one
    // launch each and throw on a library without the entry points (the tests' double)
    _sqrtNeed(symbol) {
        if (!this.lib.has || !this.lib.has(symbol)) {
            throw new Error(`the library of the field of ${this.modulus} elements has no ${symbol} entry point (include/gstark_sqrt.h): square roots are not taken on this device library`);
        }
    }
    /** the even square root of a (the other one is p - root), or null for a non-residue */
    sqrt(a) {
        const p = this.modulus;
        a = this.mod(BigInt(a));
        if (a === 0n) return 0n;
        if (this.exp(a, (p - 1n) / 2n) !== 1n) return null;
        if (!this._sqrtSplit) {
            let s = 0n, t = p - 1n, z = 2n;
            while (t % 2n === 0n) { t /= 2n; s++; }
            while (z < 1000n && this.exp(z, (p - 1n) / 2n) !== p - 1n) z++;
            if (z === 1000n) throw new Error(`sqrt: modulus is not prime (${p})`);
            this._sqrtSplit = [s, t, this.exp(z, t)];
        }
        let [m, t, c] = this._sqrtSplit;
        let r = this.exp(a, (t + 1n) / 2n), b = this.exp(a, t);
        while (b !== 1n) {
            let i = 0n, sq = b;
            while (sq !== 1n) { sq = sq * sq % p; i++; if (i === m) throw new Error(`sqrt: modulus is not prime (${p})`); }
            const f = this.exp(c, 1n << (m - i - 1n));
            r = r * f % p; c = f * f % p; b = b * c % p; m = i;
        }
        return r % 2n === 0n ? r : p - r;
    }
    _sqrtOperand(v, what) {
        if (!(v instanceof Vector)) {
            const vals = Array.from(v, x => BigInt(x));
            if (vals.some(x => x < 0n || x >= this.modulus)) throw new Error(`${what}: a value is not a canonical element`);
            v = this.newVectorFrom(vals);
        }
        this._own(v);
        if (v.elementSize !== this.elementSize) throw new Error(`${what}: a vector of field elements, not of ${v.elementSize}-byte entries`);
        if (v.length > 2 ** 20) throw new Error(`${what}: at most 2^20 elements per call, not ${v.length}`);
        return v;
    }
    /** { roots: Vector of the even roots (0 where there is none), flags: Vector of bytes (1 = a square, 0 included) }, nothing read back */
    sqrtVectorElements(v) {
        this._sqrtNeed('gs_field_sqrt');
        v = this._sqrtOperand(v, 'sqrtVectorElements');
        const roots = new Vector(this, v.length), flags = new Vector(this, v.length, undefined, 0n, 1);
        if (v.length) this.lib.call('gs_field_sqrt', this.ctx, v.ptr, v.length, roots.ptr, flags.ptr);
        return { roots, flags };
    }
    /** the flags alone: Euler's criterion */
    isSquareVectorElements(v) {
        this._sqrtNeed('gs_field_sqrt');
        v = this._sqrtOperand(v, 'isSquareVectorElements');
        const flags = new Vector(this, v.length, undefined, 0n, 1);
        if (v.length) this.lib.call('gs_field_sqrt', this.ctx, v.ptr, v.length, 0n, flags.ptr);
        return flags;
    }
    // ---- running sums, running products and linear recurrences (include/gstark_scan.h, csrc/scan.hip; DESIGN 3.19).  Operands are Vectors /
    // Matrices or arrays of BigInts, results stay on the device.  A library without the entry points (the tests' double) has no host route
    // here: the members throw
    _scanNeed(symbol) {
        if (!this.lib.has || !this.lib.has(symbol)) {
            throw new Error(`the library of the field of ${this.modulus} elements has no ${symbol} entry point (include/gstark_scan.h): scans are not computed on this device library`);
        }
    }
    /** { tile, elementsPerThread, maxElements, launches } of the library's schedule (launches: what a call of n elements enqueues) */
    scanPlan(n = 0) {
        this._scanNeed('gs_scan_plan');
        const tile = Buffer.alloc(4), per = Buffer.alloc(4), most = Buffer.alloc(8), launches = Buffer.alloc(4);
        this.lib.call('gs_scan_plan', this.ctx, n, tile, per, most, launches);
        return { tile: tile.readUInt32LE(0), elementsPerThread: per.readUInt32LE(0), maxElements: Number(most.readBigUInt64LE(0)), launches: launches.readUInt32LE(0) };
    }
    _scanCanonical(values, what) {
        const vals = Array.from(values, x => BigInt(x));
        if (vals.some(x => x < 0n || x >= this.modulus)) throw new Error(`${what}: a value is not a canonical element`);
        return vals;
    }
    _scanCount(n, what) {
        if (n > 2 ** 24) throw new Error(`${what}: at most 2^24 elements per call, not ${n}`);
    }
    _scanOperand(v, what) {
        if (v instanceof Matrix) throw new Error(`${what}: a Vector or an array, not a Matrix (the MatrixRows members take one)`);
        if (!(v instanceof Vector)) { this._scanCount(v.length, what); v = this.newVectorFrom(this._scanCanonical(v, what)); }
        this._own(v);
        if (v.elementSize !== this.elementSize) throw new Error(`${what}: a vector of field elements, not of ${v.elementSize}-byte entries`);
        this._scanCount(v.length, what);
        return v;
    }
    _scanMatrix(m, what) {
        if (m instanceof Vector) throw new Error(`${what}: a Matrix or an array of rows, not a Vector`);
        if (!(m instanceof Matrix)) {
            const cols = m.length ? m[0].length : 0;
            if (m.some(r => r.length !== cols)) throw new Error(`${what}: the rows have different lengths`);
            this._scanCount(m.length * cols, what);
            m = this.newMatrixFrom(m.map(r => this._scanCanonical(r, what)));
        }
        this._own(m);
        if (m.rowCount && !m.colCount) throw new Error(`${what}: ${m.rowCount} rows of 0 columns`);
        this._scanCount(m.rowCount * m.colCount, what);
        return m;
    }
    /** heads as a Vector of bytes (heads[i] & 1 starts a segment at i), or undefined */
    _scanHeads(heads, n, what) {
        if (heads === undefined || heads === null) return undefined;
        if (!(heads instanceof Vector)) {
            const bytes = Array.from(heads, Number);
            if (bytes.some(h => !Number.isInteger(h) || h < 0 || h > 255)) throw new Error(`${what}: heads are bytes`);
            heads = new Vector(this, bytes.length, undefined, 0n, 1);
            if (bytes.length) this.lib.call('gs_upload', this.ctx, heads.ptr, Buffer.from(bytes), bytes.length);
        }
        this._own(heads);
        if (heads.elementSize !== 1) throw new Error(`${what}: heads is a vector of bytes, not of ${heads.elementSize}-byte entries`);
        if (heads.length !== n) throw new Error(`${what}: ${heads.length} heads and ${n} values`);
        return heads;
    }
    _scanScalar(x, name, what) {
        if (typeof x !== 'bigint') throw new Error(`${what}: ${name} is a BigInt`);
        if (x < 0n || x >= this.modulus) throw new Error(`${what}: ${name} is not a canonical element`);
        return x;
    }
    _scanVector(op, v, exclusive, heads, what) {
        this._scanNeed('gs_scan');
        v = this._scanOperand(v, what);
        heads = this._scanHeads(heads, v.length, what);
        const out = new Vector(this, v.length);
        if (v.length) this.lib.call('gs_scan', this.ctx, op, exclusive ? 1 : 0, v.ptr, heads ? heads.ptr : 0n, 1, v.length, out.ptr, 0n);
        return out;
    }
    /** out[i] = v[0] + ... + v[i] (exclusive: ... + v[i-1], out[0] = 0); heads: bytes whose low bit starts a new segment.  Nothing read back */
    prefixSumVectorElements(v, exclusive = false, heads) { return this._scanVector(0, v, exclusive, heads, 'prefixSumVectorElements'); }
    /** out[i] = v[0] * ... * v[i] (exclusive: out[0] = 1); a zero zeroes the rest of its own segment only */
    prefixProductVectorElements(v, exclusive = false, heads) { return this._scanVector(1, v, exclusive, heads, 'prefixProductVectorElements'); }
    _scanRows(op, m, exclusive, totals, what) {
        this._scanNeed('gs_scan');
        m = this._scanMatrix(m, what);
        const out = new Matrix(this, m.rowCount, m.colCount), tot = totals ? new Vector(this, m.rowCount) : undefined;
        if (m.rowCount * m.colCount) this.lib.call('gs_scan', this.ctx, op, exclusive ? 1 : 0, m.ptr, 0n, m.rowCount, m.colCount, out.ptr, tot ? tot.ptr : 0n);
        return totals ? { matrix: out, totals: tot } : out;
    }
    /** the running sums of every row on its own, as a Matrix; totals = true: { matrix, totals: Vector of the rows' sums } */
    prefixSumMatrixRows(m, exclusive = false, totals = false) { return this._scanRows(0, m, exclusive, totals, 'prefixSumMatrixRows'); }
    prefixProductMatrixRows(m, exclusive = false, totals = false) { return this._scanRows(1, m, exclusive, totals, 'prefixProductMatrixRows'); }
    _reduceRows(op, src, rows, cols) {
        this._scanNeed('gs_reduce');
        const tot = new Vector(this, rows);
        if (rows * cols) this.lib.call('gs_reduce', this.ctx, op, src.ptr, rows, cols, tot.ptr);
        return tot;
    }
    /** the sum / the product of a Vector or an array, as a BigInt: one element is read back */
    sumVectorElements(v) { this._scanNeed('gs_reduce'); v = this._scanOperand(v, 'sumVectorElements'); return v.length ? this._reduceRows(0, v, 1, v.length).getValue(0) : 0n; }
    prodVectorElements(v) { this._scanNeed('gs_reduce'); v = this._scanOperand(v, 'prodVectorElements'); return v.length ? this._reduceRows(1, v, 1, v.length).getValue(0) : 1n; }
    /** a Vector of the sums / the products of the rows; no running values are written */
    sumMatrixRows(m) { this._scanNeed('gs_reduce'); m = this._scanMatrix(m, 'sumMatrixRows'); return this._reduceRows(0, m, m.rowCount, m.colCount); }
    prodMatrixRows(m) { this._scanNeed('gs_reduce'); m = this._scanMatrix(m, 'prodMatrixRows'); return this._reduceRows(1, m, m.rowCount, m.colCount); }
    /** x[i] = a[i] * x[i-1] + b[i], x[-1] = x0: out[i] = x[i] (exclusive: x[i-1], out[0] = x0).  a: a Vector, an array, or ONE BigInt for every
     *  step; x0 starts every segment (a start per segment is folded into that segment's first b) */
    linearRecurrence(a, b, x0 = 0n, exclusive = false, heads) {
        const what = 'linearRecurrence';
        this._scanNeed('gs_scan_affine');
        b = this._scanOperand(b, what);
        const scalar = typeof a === 'bigint' ? this._scanScalar(a, 'a', what) : undefined;
        if (scalar === undefined) {
            a = this._scanOperand(a, what);
            if (a.length !== b.length) throw new Error(`${what}: ${a.length} factors and ${b.length} terms: the lengths differ`);
        }
        x0 = this._scanScalar(x0, 'x0', what);
        heads = this._scanHeads(heads, b.length, what);
        const out = new Vector(this, b.length);
        if (b.length) this.lib.call('gs_scan_affine', this.ctx, exclusive ? 1 : 0, scalar === undefined ? a.ptr : 0n, this.le(scalar === undefined ? 0n : scalar), b.ptr, this.le(x0), heads ? heads.ptr : 0n, 1, b.length, out.ptr);
        return out;
    }
    linearRecurrenceMatrixRows(a, b, x0 = 0n, exclusive = false) {
        const what = 'linearRecurrenceMatrixRows';
        this._scanNeed('gs_scan_affine');
        b = this._scanMatrix(b, what);
        const scalar = typeof a === 'bigint' ? this._scanScalar(a, 'a', what) : undefined;
        if (scalar === undefined) {
            a = this._scanMatrix(a, what);
            if (a.rowCount !== b.rowCount || a.colCount !== b.colCount) throw new Error(`${what}: a is ${a.rowCount} x ${a.colCount} and b is ${b.rowCount} x ${b.colCount}: the shapes differ`);
        }
        x0 = this._scanScalar(x0, 'x0', what);
        const out = new Matrix(this, b.rowCount, b.colCount);
        if (b.rowCount * b.colCount) this.lib.call('gs_scan_affine', this.ctx, exclusive ? 1 : 0, scalar === undefined ? a.ptr : 0n, this.le(scalar === undefined ? 0n : scalar), b.ptr, this.le(x0), 0n, b.rowCount, b.colCount, out.ptr);
        return out;
    }
    // ---- long polynomials at arbitrary points (include/gstark_poly.h, csrc/poly.hip; DESIGN 3.16).  Operands are Vectors or arrays of
    // BigInts, results stay on the device.  A library without the entry points (the tests' double) has no host route here: the members throw
    _polyNeed(symbol) {
        if (!this.lib.has || !this.lib.has(symbol)) {
            throw new Error(`the library of the field of ${this.modulus} elements has no ${symbol} entry point (include/gstark_poly.h): long polynomials are not computed on this device library`);
        }
    }
    /** [omega as bytes, log2 of its order]: a root of unity of the largest power-of-two order dividing p - 1, capped at 2^26; once per field */
    _polyOmega() {
        if (!this._polyRoot) {
            let log2 = 0;
            while (log2 < 26 && (this.modulus - 1n) % (1n << BigInt(log2 + 1)) === 0n) log2++;
            this._polyRoot = [this.le(this.getRootOfUnity(2 ** log2)), log2];
        }
        return this._polyRoot;
    }
    _polyOperand(v, what) {
        if (!(v instanceof Vector)) v = this.newVectorFrom(Array.from(v, x => BigInt(x)));
        this._own(v);
        if (v.length > 2 ** 20) throw new Error(`${what}: at most 2^20 elements per operand, not ${v.length}`);
        return v;
    }
    /** the xs.length + 1 coefficients of the product of (x - xs[i]), low-order first */
    polyFromRoots(xs) {
        this._polyNeed('gs_poly_from_roots');
        xs = this._polyOperand(xs, 'polyFromRoots');
        const [omega, log2] = this._polyOmega(), out = new Vector(this, xs.length + 1);
        this.lib.call('gs_poly_from_roots', this.ctx, omega, log2, xs.length ? xs.ptr : 0n, xs.length, out.ptr);
        return out;
    }
    /** [q, r] with a = q * b + r: q of a.length - b.length + 1 coefficients (one zero when a is shorter), r of b.length - 1 */
    divModPolys(a, b) {
        this._polyNeed('gs_poly_div');
        a = this._polyOperand(a, 'divModPolys'); b = this._polyOperand(b, 'divModPolys');
        if (!a.length || !b.length) throw new Error('divModPolys: both polynomials need at least one coefficient');
        const [omega, log2] = this._polyOmega();
        const q = new Vector(this, Math.max(a.length - b.length + 1, 1)), r = new Vector(this, b.length - 1);
        this.lib.call('gs_poly_div', this.ctx, omega, log2, a.ptr, a.length, b.ptr, b.length, q.ptr, r.ptr);
        return [q, r];
    }
    divPolys(a, b) { return this.divModPolys(a, b)[0]; }
    /** poly at every x of xs: method 'tree' (gs_poly_eval_points), 'horner' (gs_eval_polys_at_points) or undefined: the tree from 2^15
     *  coefficients and points on (profiles/poly.md: Horner is ahead at 2^14, the tree at 2^15), Horner below */
    evalPolyAtPoints(poly, xs, method) {
        if (method !== undefined && method !== 'tree' && method !== 'horner') throw new Error(`evalPolyAtPoints: method ${method} is not 'tree' or 'horner'`);
        poly = this._polyOperand(poly, 'evalPolyAtPoints');
        if (method === undefined) method = Math.min(poly.length, xs.length) >= TREE_EVAL_FROM ? 'tree' : 'horner';
        if (method !== 'tree') {
            const points = xs instanceof Vector ? xs.toValues() : Array.from(xs, x => this.mod(BigInt(x)));
            const out = new Vector(this, points.length);
            if (points.length) this.lib.call('gs_eval_polys_at_points', this.ctx, poly.ptr, 1, poly.length, [poly.length], this.packLe(points, x => x), points.length, out.ptr);
            return out;
        }
        this._polyNeed('gs_poly_eval_points');
        xs = this._polyOperand(xs, 'evalPolyAtPoints');
        const [omega, log2] = this._polyOmega(), out = new Vector(this, xs.length);
        this.lib.call('gs_poly_eval_points', this.ctx, omega, log2, poly.length ? poly.ptr : 0n, poly.length, xs.length ? xs.ptr : 0n, xs.length, xs.length ? out.ptr : 0n);
        return out;
    }
    /** the coefficients of the polynomial through (xs[i], ys[i]): any distinct points, up to 2^20 of them; equal points throw */
    interpolateAtPoints(xs, ys) {
        this._polyNeed('gs_poly_interpolate_points');
        xs = this._polyOperand(xs, 'interpolateAtPoints'); ys = this._polyOperand(ys, 'interpolateAtPoints');
        if (xs.length !== ys.length) throw new Error('Number of x coordinates must be the same as number of y coordinates');
        if (!xs.length) throw new Error('interpolateAtPoints: at least one point');
        const [omega, log2] = this._polyOmega(), out = new Vector(this, xs.length), flag = new Vector(this, 1, undefined, 0n, 1);
        this.lib.call('gs_poly_interpolate_points', this.ctx, omega, log2, xs.ptr, ys.ptr, xs.length, out.ptr, flag.ptr);
        if (flag.toBuffer()[0]) throw new Error('interpolateAtPoints: two of the x coordinates are equal');
        return out;
    }
    /** a square root of g (g of order `order`, a power of two): an element of order 2 * order, found in the field's 2-power subgroup bit by bit */
    _rootAbove(g, order) {
        const w = this.getRootOfUnity(2 * order), g0 = this.mul(w, w);
        let e = 0n, k = 0;
        while ((1 << k) < order) k++;
        for (let i = 0; i < k; i++) {
            const rest = this.mul(this.mod(g), this.inv(this.exp(g0, e)));
            if (this.exp(rest, BigInt(order) >> BigInt(i + 1)) !== 1n) e |= 1n << BigInt(i);
        }
        const s = this.exp(w, e);
        if (this.mul(s, s) !== this.mod(g)) throw new Error(`interpolateAtRoots: ${g} does not generate a domain of ${order} points`);
        return s;
    }
    /** The interpolant through (rootOfUnity^positions[i], ys[i]): points of the domain of `order` points (a power of two) that rootOfUnity
     *  generates, distinct positions — built on the device (gs_boundary_polys; DESIGN 3.7): any number of points up to `order`, a device
     *  vector of positions.length coefficients, the ones interpolate() gives for these points.  The field must have a root of unity of
     *  order 2 * order, the library the entry point (the HIP library has it; interpolate() remains for everything else). */
    interpolateAtRoots(rootOfUnity, order, positions, ys) {
        this._own(ys);
        const m = positions.length;
        if (m !== ys.length) throw new Error('Number of x coordinates must be the same as number of y coordinates');
        if (m < 1 || order < 1 || (order & (order - 1))) throw new Error('interpolateAtRoots: at least one point, on a domain of a power-of-two order');
        const omega = this._rootAbove(rootOfUnity, order);
        const out = new Vector(this, m), z = new Vector(this, m + 1);
        this.lib.call('gs_boundary_polys', this.ctx, this.le(omega), 2 * order, order, positions, ys.toBuffer(), [m], 1, m, out.ptr, z.ptr);
        return out;
    }
    interpolate(xs, ys) {
        this._own(xs, ys);
        // xs known to be a whole domain {g^i} of a power-of-two order (getPowerSeries of a root of unity) and a library with the device entry
        // point: the same coefficients without the host path's 4 096-point cap
        if (xs.seriesBase !== undefined && xs.length > 1 && !(xs.length & (xs.length - 1)) && xs.length === ys.length && this.lib.has && this.lib.has('gs_boundary_polys') &&
            this.exp(xs.seriesBase, BigInt(xs.length / 2)) === this.modulus - 1n && (this.modulus - 1n) % BigInt(2 * xs.length) === 0n)
            return this.interpolateAtRoots(xs.seriesBase, xs.length, Array.from({ length: xs.length }, (_, i) => i), ys);
        const n = xs.length, out = Buffer.alloc(this.elementSize * n);
        this.lib.call('gs_small_interpolate', xs.toBuffer(), ys.toBuffer(), n, out);
        const v = new Vector(this, n); this.lib.call('gs_upload', this.ctx, v.ptr, out, out.length); return v;
    }
    interpolateQuarticBatch(xs, ys) {
        this._own(xs, ys);
        const out = new Matrix(this, ys.rowCount, 4);
        if (xs.quarticDomain) this.lib.call('gs_interpolate_quartic_domain', this.ctx, this.le(xs.quarticDomain.omega), xs.quarticDomain.n, xs.quarticDomain.step, ys.ptr, ys.rowCount, out.ptr);
        else this.lib.call('gs_interpolate_quartic_batch', this.ctx, xs.ptr, ys.ptr, ys.rowCount, out.ptr);
        return out;
    }
    evalQuarticBatch(polys, x) { this._own(polys); const out = new Vector(this, polys.rowCount); this.lib.call('gs_eval_quartic_batch', this.ctx, polys.ptr, polys.rowCount, this.le(this.mod(x)), out.ptr); return out; }
}

function createPrimeField(modulus, options) { return new PrimeField(modulus, options); }

module.exports = { createPrimeField, PrimeField, Vector, Matrix, MODULUS, LIBRARIES, native, le, packLe, unpackLe, fromLe, sha256, isProbablePrime };
