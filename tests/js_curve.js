'use strict';
// tests/js_curve.js <hip|double> <expectations.json> — js/curve.js against values the Python host computed (tests/test_curve.py writes
// them): the 224-bit curve (fixed and variable base, addends with infinity among them, perturbed points) and the special cases of the
// curve of 97 200 points over the 96 769 field.  Two fields in one process.
//   hip:    the host members, mulMany (lists, a device Matrix, device results) and containsMany
//   double: a library without the optional entry points — the host members still equal the Python values, the device members throw an
//           Error that says what is missing
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
assert.strictEqual(c224.b, BigInt(w224.b));
assert.deepStrictEqual(c224.G, big(w224.G));
assert.strictEqual(c224.order, BigInt(w224.order));
assert.throws(() => curves.curve224(f17), /curve224/);

// host members
const scalars = big(w224.scalars), points = big(w224.points), addends = big(w224.addends), fixed = big(w224.fixed), variable = big(w224.variable);
for (const k of [0, 1, 2, 3, 4, 5, 7]) {
    assert.deepStrictEqual(c224.mul(c224.G, scalars[k]), fixed[k]);
    assert.deepStrictEqual(c224.add(addends[k], c224.mul(points[k], scalars[k])), variable[k]);
}
assert.strictEqual(c224.mul(c224.G, c224.order), null);
assert.deepStrictEqual(c224.mul(c224.G, c224.order - 1n), c224.neg(c224.G));
const smallPoints = big(w17.points), smallScalars = big(w17.scalars), products = big(w17.products);
smallPoints.forEach((pt, k) => assert.deepStrictEqual(small.mul(pt, smallScalars[k]), products[k]));
assert.strictEqual(c224.contains(c224.G) && c224.contains(null) && !c224.contains([c224.G[0], c224.G[1] ^ 1n]), true);

if (mode === 'double') {
    for (const f of [f224, f17]) assert.strictEqual(f.lib.has('gs_curve_mul'), false);
    for (const attempt of [() => c224.mulMany(c224.G, scalars), () => c224.containsMany(points), () => small.mulMany(smallPoints, smallScalars)]) {
        assert.throws(attempt, e => e.constructor === Error && /no gs_curve_mul entry point \(include\/gstark_curve\.h\)/.test(e.message));
    }
} else {
    for (const f of [f224, f17]) assert.strictEqual(f.lib.has('gs_curve_mul') && f.lib.has('gs_curve_contains'), true);
    assert.deepStrictEqual(c224.mulMany(c224.G, scalars), fixed);
    assert.deepStrictEqual(c224.mulMany(f224.newMatrixFrom([c224.G]), scalars), fixed);
    assert.deepStrictEqual(c224.mulMany(points, scalars, { addends }), variable);
    const onDevice = c224.mulMany(c224.G, scalars, { device: true });
    assert.deepStrictEqual(onDevice.points.toValues(), fixed.map(pt => (pt === null ? [0n, 0n] : pt)));
    assert.deepStrictEqual(Array.from(onDevice.infinity.toBuffer()), fixed.map(pt => (pt === null ? 1 : 0)));
    assert.deepStrictEqual(c224.mulMany(c224.G, scalars.slice(0, 9), { bits: 100 }), scalars.slice(0, 9).map(k => c224.mul(c224.G, k & ((1n << 100n) - 1n))));
    assert.deepStrictEqual(small.mulMany(smallPoints, smallScalars), products);
    assert.deepStrictEqual(c224.containsMany(big(w224.perturbed)), w224.contains);
    assert.deepStrictEqual(c224.containsMany(f224.newMatrixFrom(points)), points.map(() => true));
    assert.deepStrictEqual(c224.mulMany(c224.G, []), []);
    assert.throws(() => c224.mulMany([[c224.G[0], c224.G[1] ^ 1n]], [1n]), /not a finite point/);
    assert.throws(() => c224.mulMany(c224.G, [1n << 256n]), /scalar/);
    assert.throws(() => c224.mulMany(c224.G, [1n], { bits: 257 }), /bits/);
    assert.throws(() => c224.mulMany(points.slice(0, 2), scalars.slice(0, 3)), /one point for all/);
    assert.throws(() => f224.lib.call('gs_curve_mul', f224.ctx, f224.le(c224.a), onDevice.points.ptr, 2, onDevice.points.ptr, 256, 0n, 0n, 3, onDevice.points.ptr, onDevice.infinity.ptr), /one for all/);
}
console.log(`js curve (${mode}) OK`);
