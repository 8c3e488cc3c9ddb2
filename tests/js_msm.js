'use strict';
// tests/js_msm.js <hip|double> <expectations.json> — msm / sumMany of js/curve.js against values the Python host computed
// (tests/test_msm.py writes them): sums on the 224-bit curve (all terms, infinite points among them, 100 bits of every scalar, the
// points themselves, no term at all) and on the curve of 97 200 points over the 96 769 field under the plan's window and forced ones.
// Two fields in one process.
//   hip:    the sums, from arrays and from a device Matrix, and the refusals
//   double: a library without the optional entry point — msm and sumMany throw an Error that says what is missing
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const ROOT = path.resolve(__dirname, '..');
const galois = require(path.join(ROOT, 'js', 'galois.js'));
const curves = require(path.join(ROOT, 'js', 'curve.js'));

const mode = process.argv[2];
const want = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const big = x => (x === null ? null : Array.isArray(x) ? x.map(big) : BigInt(x));

const w224 = want.p224, w17 = want.q17;
const f224 = galois.createPrimeField(BigInt(w224.modulus)), f17 = galois.createPrimeField(BigInt(w17.modulus));
const c224 = curves.curve224(f224), small = curves.createCurve(f17, -3n, BigInt(w17.b));
const scalars = big(w224.scalars), points = big(w224.points), holes = big(w224.holes);
const smallPoints = big(w17.points), smallScalars = big(w17.scalars);

// the host law agrees with the recorded sums on a prefix (the whole lists are the device's business)
let acc = null;
for (let k = 0; k < 3; k++) acc = c224.add(acc, c224.mul(points[k], scalars[k]));
assert.deepStrictEqual(acc, c224.add(points[1], c224.mul(points[2], 2n)));

if (mode === 'double') {
    for (const f of [f224, f17]) assert.strictEqual(f.lib.has('gs_curve_msm'), false);
    for (const attempt of [() => c224.msm(points, scalars), () => c224.sumMany(points), () => small.msm(smallPoints, smallScalars, 256, 4)]) {
        assert.throws(attempt, e => e.constructor === Error && /no gs_curve_msm entry point \(include\/gstark_msm\.h\)/.test(e.message));
    }
} else {
    for (const f of [f224, f17]) assert.strictEqual(f.lib.has('gs_curve_msm'), true);
    assert.deepStrictEqual(c224.msm(points, scalars), big(w224.sum));
    assert.deepStrictEqual(c224.msm(f224.newMatrixFrom(points), scalars), big(w224.sum));
    assert.deepStrictEqual(c224.msm(points, scalars, 256, 9), big(w224.sum));
    assert.deepStrictEqual(c224.msm(holes, scalars), big(w224.sum_holes));
    assert.deepStrictEqual(c224.msm(points, scalars, 100), big(w224.sum_100_bits));
    assert.deepStrictEqual(c224.sumMany(points), big(w224.sum_points));
    assert.strictEqual(c224.msm([], []), null);
    assert.strictEqual(c224.msm([null], [3n]), null);
    assert.strictEqual(c224.msm([c224.G, c224.neg(c224.G)], [5n, 5n]), null);
    assert.strictEqual(c224.msm([c224.G], [c224.order]), null);
    for (const window of [0, 1, 5, 16]) assert.deepStrictEqual(small.msm(smallPoints, smallScalars, 256, window), big(w17.sum));
    assert.deepStrictEqual(small.sumMany(smallPoints), big(w17.sum_points));
    assert.deepStrictEqual(small.sumMany(f17.newMatrixFrom(smallPoints)), big(w17.sum_points));
    assert.throws(() => c224.msm([[c224.G[0], c224.G[1] ^ 1n]], [1n]), /not a finite point/);
    assert.throws(() => c224.msm([c224.G], [1n << 256n]), /scalar/);
    assert.throws(() => c224.msm([c224.G], [1n], 257), /bits/);
    assert.throws(() => c224.msm([c224.G], [1n], 256, 17), /window/);
    assert.throws(() => c224.msm(points.slice(0, 2), scalars.slice(0, 3)), /a term is one of each/);
    const m = f224.newMatrixFrom(points.slice(0, 3));
    assert.throws(() => f224.lib.call('gs_curve_msm', f224.ctx, f224.le(c224.a), m.ptr, m.ptr, 8, 64, 3, 0, m.ptr, m.ptr), /scalar_stride/);
}
console.log(`js msm (${mode}) OK`);
