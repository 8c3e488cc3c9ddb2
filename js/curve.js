'use strict';
// js/curve.js — scalar multiplications on short Weierstrass curves y^2 = x^3 + a*x + b over a PrimeField of js/galois.js, the batches on
// the device (include/gstark_curve.h through the addon's table): the products, public keys and nonce points that the reference's
// examples/elliptic/pointMul.ts and the Schnorr example of examples/assembly/lib224.ts assert.  A point is [x, y] (BigInts), the point at
// infinity is null.  createCurve(field, a, b) has the host members contains / neg / add / mul (BigInt arithmetic, the complete affine
// law) and the device members mulMany / containsMany: one launch for the whole batch, one thread per multiplication — and msm / sumMany
// (include/gstark_msm.h): the SUM of the products, or of the points, in one call.  A field whose library lacks the entry points (they
// are optional on an implementation of the ABI) makes the device members throw an Error saying so.  liftX / decompressMany /
// compressMany (include/gstark_sqrt.h) go between full points and x with a parity bit, one launch each.
const { Matrix, Vector } = require('./galois.js');

const MAX_COUNT = 1 << 20, SCALAR_BITS = 256, MAX_WINDOW = 16;
const MODULUS_224 = 2n ** 224n - 2n ** 96n + 1n;
// the point the reference's examples multiply (pointMul.ts:23-24, lib224.ts:163), b as it follows from it, and the order of the point
const G_224 = [19277929113566293071110308034699488026831934219452440156649784352033n, 19926808758034470970197974370888749184205991990603949537637343198772n];
const B_224 = 0xb4050a850c04b3abf54132565044b0b7d7bfd8ba270b39432355ffb4n;
const ORDER_224 = 0xffffffffffffffffffffffffffff16a2e0b8f03e13dd29455c5c2a3dn;

function needDevice(field) {
    for (const symbol of ['gs_curve_mul', 'gs_curve_contains']) {
        if (!field.lib.has || !field.lib.has(symbol)) {
            throw new Error(`the library of the field of ${field.modulus} elements has no ${symbol} entry point (include/gstark_curve.h): curve points are not multiplied on this device library`);
        }
    }
}

function needSums(field) {
    if (!field.lib.has || !field.lib.has('gs_curve_msm')) {
        throw new Error(`the library of the field of ${field.modulus} elements has no gs_curve_msm entry point (include/gstark_msm.h): curve points are not summed on this device library`);
    }
}

function needLifts(field) {
    for (const symbol of ['gs_curve_lift_x', 'gs_curve_compress']) {
        if (!field.lib.has || !field.lib.has(symbol)) {
            throw new Error(`the library of the field of ${field.modulus} elements has no ${symbol} entry point (include/gstark_sqrt.h): curve points are not lifted on this device library`);
        }
    }
}

function createCurve(field, a, b) {
    const p = field.modulus;
    a = field.mod(BigInt(a)); b = field.mod(BigInt(b));
    const curve = { field, a, b, G: null, order: null };

    // ---- host BigInts
    curve.contains = function (point) {
        if (point === null) return true;
        const [x, y] = point;
        return x >= 0n && x < p && y >= 0n && y < p && field.mod(y * y - (x * x + a) * x - b) === 0n;
    };
    curve.neg = point => (point === null ? null : [point[0], field.neg(point[1])]);
    /** the affine group law, complete: infinity, equal points, opposite points, points with y = 0 */
    curve.add = function (u, v) {
        if (u === null) return v;
        if (v === null) return u;
        let m;
        if (u[0] === v[0]) {
            if (field.add(u[1], v[1]) === 0n) return null;
            m = field.div(3n * u[0] * u[0] + a, 2n * u[1]);
        } else {
            m = field.div(field.sub(u[1], v[1]), field.sub(u[0], v[0]));
        }
        const x = field.mod(m * m - u[0] - v[0]);
        return [x, field.mod(m * (u[0] - x) - u[1])];
    };
    curve.mul = function (point, scalar) {
        let acc = null;
        const bits = BigInt(scalar).toString(2);
        for (const bit of bits) {
            acc = curve.add(acc, acc);
            if (bit === '1') acc = curve.add(acc, point);
        }
        return BigInt(scalar) === 0n ? null : acc;
    };

    // ---- device
    const pointMatrix = function (points, what) {
        if (points instanceof Matrix) {
            field._own(points);
            if (points.colCount !== 2) throw new Error(`a matrix of ${what} has 2 columns (x, y), not ${points.colCount}`);
            return points;
        }
        for (const pt of points) if (!curve.contains(pt) || pt === null) throw new Error(`${pt} is not a finite point of the curve`);
        return field.newMatrixFrom(points);
    };
    const bytesOnDevice = function (bytes) {
        const v = new Vector(field, bytes.length, undefined, 0n, 1);
        if (bytes.length) field.lib.call('gs_upload', field.ctx, v.ptr, bytes, bytes.length);
        return v;
    };

    /** one bool per row of a device Matrix of count x 2, or per [x, y] of an array */
    curve.containsMany = function (points) {
        needDevice(field);
        if (!(points instanceof Matrix)) points = field.newMatrixFrom(points);
        field._own(points);
        if (points.colCount !== 2) throw new Error(`a matrix of points has 2 columns (x, y), not ${points.colCount}`);
        const count = points.rowCount;
        if (count > MAX_COUNT) throw new Error(`at most 2^20 points per call, not ${count}`);
        if (!count) return [];
        const flags = new Vector(field, count, undefined, 0n, 1);
        field.lib.call('gs_curve_contains', field.ctx, field.le(a), field.le(b), points.ptr, count, flags.ptr);
        return Array.from(flags.toBuffer(), v => v !== 0);
    };

    /** addends[k] + (scalars[k] mod 2^bits) * points[k]: points an array of [x, y], ONE [x, y] for all (the fixed-base case) or a device
     *  Matrix of count x 2 or 1 x 2; scalars BigInts in 0 .. 2^256 - 1; options.addends an array of [x, y] / null (infinity);
     *  options.bits 1 .. 256; options.device: { points: Matrix of count x 2, infinity: Vector of count flag bytes }, nothing read back.
     *  Otherwise an array of [x, y] / null. */
    curve.mulMany = function (points, scalars, options = {}) {
        needDevice(field);
        const bits = options.bits === undefined ? SCALAR_BITS : options.bits;
        if (!(bits >= 1 && bits <= SCALAR_BITS)) throw new Error(`${bits} bits of a scalar are outside 1 .. ${SCALAR_BITS}`);
        scalars = scalars.map(k => BigInt(k));
        if (scalars.some(k => k < 0n || k >> 256n)) throw new Error(`a scalar is outside 0 .. 2^${SCALAR_BITS} - 1`);
        const count = scalars.length;
        if (count > MAX_COUNT) throw new Error(`at most 2^20 multiplications per call, not ${count}`);
        if (Array.isArray(points) && points.length === 2 && typeof points[0] === 'bigint') points = [points];
        const src = pointMatrix(points, 'points');
        if (src.rowCount !== count && src.rowCount !== 1) throw new Error(`${src.rowCount} points and ${count} scalars: one point for all, or one each`);
        let more = null, moreInf = null;
        if (options.addends) {
            if (options.addends.length !== count) throw new Error(`${options.addends.length} addends and ${count} scalars: one addend each`);
            for (const pt of options.addends) if (!curve.contains(pt)) throw new Error(`${pt} is not a point of the curve`);
            more = field.newMatrixFrom(options.addends.map(pt => (pt === null ? [0n, 0n] : pt)));
            moreInf = bytesOnDevice(Buffer.from(options.addends.map(pt => (pt === null ? 1 : 0))));
        }
        const out = new Matrix(field, count, 2), flags = new Vector(field, count, undefined, 0n, 1);
        if (count) {
            const ks = Buffer.alloc(32 * count);
            scalars.forEach((k, i) => { for (let w = 0; w < 4; w++) ks.writeBigUInt64LE((k >> BigInt(64 * w)) & 0xffffffffffffffffn, 32 * i + 8 * w); });
            const keys = bytesOnDevice(ks);
            field.lib.call('gs_curve_mul', field.ctx, field.le(a), src.ptr, src.rowCount, keys.ptr, bits, more ? more.ptr : 0n, moreInf ? moreInf.ptr : 0n, count, out.ptr, flags.ptr);
        }
        if (options.device) return { points: out, infinity: flags };
        const inf = flags.toBuffer();
        return out.toValues().map((row, k) => (inf[k] ? null : row));
    };

    /** the sum over k of (scalars[k] mod 2^bits) * points[k]: [x, y], or null for infinity.  points: an array of [x, y] / null (an
     *  infinite point contributes nothing: it is dropped with its scalar) or a device Matrix of count x 2 finite points; scalars: BigInts
     *  in 0 .. 2^256 - 1; bits 1 .. 256 (default 256); window 0 (the plan chooses, default) or 1 .. 16 (the bucket method with windows of
     *  that many bits). */
    curve.msm = function (points, scalars, bits = SCALAR_BITS, window = 0) {
        needSums(field);
        if (!(bits >= 1 && bits <= SCALAR_BITS)) throw new Error(`${bits} bits of a scalar are outside 1 .. ${SCALAR_BITS}`);
        if (!(window >= 0 && window <= MAX_WINDOW)) throw new Error(`a window of ${window} bits is outside 0 .. ${MAX_WINDOW}`);
        scalars = scalars.map(k => BigInt(k));
        if (scalars.some(k => k < 0n || k >> 256n)) throw new Error(`a scalar is outside 0 .. 2^${SCALAR_BITS} - 1`);
        const given = points instanceof Matrix ? points.rowCount : points.length;
        if (given !== scalars.length) throw new Error(`${given} points and ${scalars.length} scalars: a term is one of each`);
        if (!(points instanceof Matrix)) {
            scalars = scalars.filter((k, i) => points[i] !== null);
            points = points.filter(pt => pt !== null);
        }
        const count = scalars.length;
        if (count > MAX_COUNT) throw new Error(`at most 2^20 terms per sum, not ${count}`);
        const out = new Matrix(field, 1, 2), flag = new Vector(field, 1, undefined, 0n, 1);
        let src = 0n, keys = 0n;
        if (count) {
            src = pointMatrix(points, 'points').ptr;
            const ks = Buffer.alloc(32 * count);
            scalars.forEach((k, i) => { for (let w = 0; w < 4; w++) ks.writeBigUInt64LE((k >> BigInt(64 * w)) & 0xffffffffffffffffn, 32 * i + 8 * w); });
            keys = bytesOnDevice(ks).ptr;
        }
        field.lib.call('gs_curve_msm', field.ctx, field.le(a), src, keys, 32, bits, count, window, out.ptr, flag.ptr);
        return flag.toBuffer()[0] ? null : out.toValues()[0];
    };

    /** the sum of the points: msm with every scalar 1 and one bit */
    curve.sumMany = function (points) {
        const count = points instanceof Matrix ? points.rowCount : points.length;
        return curve.msm(points, new Array(count).fill(1n), 1, 0);
    };

    // ---- compressed points (include/gstark_sqrt.h): x and the parity y & 1
    /** [x, y] with y & 1 == parities[k] for every x of an array of BigInts or a device Vector, null where x^3 + a*x + b is not a square
     *  (y = 0 answers both parities).  parities: undefined (every y even), an array of 0 / 1, or a device Vector of bytes.
     *  options.device: { points: Matrix of count x 2 ((0, 0) where there is no point), flags: Vector of count bytes }, nothing read back. */
    curve.liftX = function (xs, parities, options = {}) {
        needLifts(field);
        if (!(xs instanceof Vector)) {
            xs = Array.from(xs, x => BigInt(x));
            if (xs.some(x => x < 0n || x >= p)) throw new Error('an x is not a canonical element');
            xs = field.newVectorFrom(xs);
        }
        field._own(xs);
        if (xs.elementSize !== field.elementSize) throw new Error(`xs are a vector of field elements, not of ${xs.elementSize}-byte entries`);
        const count = xs.length;
        if (parities !== undefined && parities !== null && !(parities instanceof Vector)) {
            parities = Array.from(parities, b => Number(b));
            if (parities.some(b => b !== 0 && b !== 1)) throw new Error('parities are 0 or 1');
            parities = bytesOnDevice(Buffer.from(parities));
        }
        if (parities) {
            field._own(parities);
            if (parities.elementSize !== 1) throw new Error(`parities are a vector of bytes, not of ${parities.elementSize}-byte entries`);
            if (parities.length !== count) throw new Error(`${parities.length} parities and ${count} xs: one parity each`);
        }
        if (count > MAX_COUNT) throw new Error(`at most 2^20 points per call, not ${count}`);
        const out = new Matrix(field, count, 2), flags = new Vector(field, count, undefined, 0n, 1);
        if (count) field.lib.call('gs_curve_lift_x', field.ctx, field.le(a), field.le(b), xs.ptr, parities ? parities.ptr : 0n, count, out.ptr, flags.ptr);
        if (options.device) return { points: out, flags };
        const ok = flags.toBuffer();
        return out.toValues().map((row, k) => (ok[k] ? row : null));
    };
    /** liftX with the parities required */
    curve.decompressMany = function (xs, parities, options = {}) {
        if (parities === undefined || parities === null) throw new Error('decompressMany needs the parities');
        return curve.liftX(xs, parities, options);
    };
    /** { xs, parities } of finite points (an array of [x, y] or a device Matrix of count x 2): an array of BigInts and an array of 0 / 1;
     *  options.device: a Vector of elements and a Vector of bytes, nothing read back */
    curve.compressMany = function (points, options = {}) {
        needLifts(field);
        const src = pointMatrix(points, 'points'), count = src.rowCount;
        if (count > MAX_COUNT) throw new Error(`at most 2^20 points per call, not ${count}`);
        const xs = new Vector(field, count), parities = new Vector(field, count, undefined, 0n, 1);
        if (count) field.lib.call('gs_curve_compress', field.ctx, src.ptr, count, xs.ptr, parities.ptr);
        if (options.device) return { xs, parities };
        return { xs: xs.toValues(), parities: Array.from(parities.toBuffer()) };
    };
    return curve;
}

/** the curve of examples/elliptic/pointmul.aa and assembly/lib224.aa (a = p - 3 over 2^224 - 2^96 + 1) with G and its order */
function curve224(field) {
    if (field.modulus !== MODULUS_224) throw new Error(`curve224: the curve lives over the field of 2^224 - 2^96 + 1 elements, not ${field.modulus}`);
    const curve = createCurve(field, -3n, B_224);
    curve.G = G_224.slice();
    curve.order = ORDER_224;
    return curve;
}

module.exports = { createCurve, curve224, MODULUS_224, G_224, B_224, ORDER_224 };
