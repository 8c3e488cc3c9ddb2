'use strict';
// tests/js_sqrt.js <hip|double> <expectations.json> — sqrt / sqrtVectorElements / isSquareVectorElements of js/galois.js and liftX /
// decompressMany / compressMany of js/curve.js against values the Python host computed (tests/test_sqrt.py writes them): 65 roots and
// 65 lifts in the 224-bit field.
//   hip:    the roots, the flags and the lifted points, from arrays and from device vectors, and the refusals
//   double: a library without the optional entry points — the host sqrt still answers, the device members throw an Error that says what
//           is missing
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const ROOT = path.resolve(__dirname, '..');
const galois = require(path.join(ROOT, 'js', 'galois.js'));
const curves = require(path.join(ROOT, 'js', 'curve.js'));

const mode = process.argv[2];
const want = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const big = x => (x === null ? null : Array.isArray(x) ? x.map(big) : BigInt(x));

const f224 = galois.createPrimeField(BigInt(want.modulus));
const c224 = curves.curve224(f224);
const values = big(want.values), roots = big(want.roots), xs = big(want.xs), lifted = big(want.lifted);
const parities = want.parities, flags = want.flags;
assert.strictEqual(values.length, 65);
assert.strictEqual(xs.length, 65);

// the host member agrees with the recorded roots
values.forEach((v, k) => assert.strictEqual(f224.sqrt(v), flags[k] ? roots[k] : null));

if (mode === 'double') {
    assert.strictEqual(f224.lib.has('gs_field_sqrt'), false);
    for (const attempt of [() => f224.sqrtVectorElements(values), () => f224.isSquareVectorElements(values)]) {
        assert.throws(attempt, e => e.constructor === Error && /no gs_field_sqrt entry point \(include\/gstark_sqrt\.h\)/.test(e.message));
    }
    for (const attempt of [() => c224.liftX(xs, parities), () => c224.decompressMany(xs, parities), () => c224.compressMany([c224.G])]) {
        assert.throws(attempt, e => e.constructor === Error && /no gs_curve_lift_x entry point \(include\/gstark_sqrt\.h\)/.test(e.message));
    }
} else {
    for (const symbol of ['gs_field_sqrt', 'gs_curve_lift_x', 'gs_curve_compress', 'gs_field_sqrt_plan']) assert.strictEqual(f224.lib.has(symbol), true);
    for (const operand of [values, f224.newVectorFrom(values)]) {
        const got = f224.sqrtVectorElements(operand);
        assert.deepStrictEqual(got.roots.toValues(), roots.map((r, k) => (flags[k] ? r : 0n)));
        assert.deepStrictEqual(Array.from(got.flags.toBuffer()), flags);
        assert.deepStrictEqual(Array.from(f224.isSquareVectorElements(operand).toBuffer()), flags);
    }
    assert.deepStrictEqual(c224.liftX(xs, parities), lifted);
    assert.deepStrictEqual(c224.decompressMany(f224.newVectorFrom(xs), parities), lifted);
    assert.deepStrictEqual(c224.liftX(xs), lifted.map(pt => (pt === null ? null : [pt[0], pt[1] % 2n === 0n ? pt[1] : f224.neg(pt[1])])));
    const there = lifted.filter(pt => pt !== null);
    const packed = c224.compressMany(there);
    assert.deepStrictEqual(packed.xs, there.map(pt => pt[0]));
    assert.deepStrictEqual(packed.parities, there.map(pt => Number(pt[1] & 1n)));
    const onDevice = c224.compressMany(f224.newMatrixFrom(there), { device: true });
    assert.deepStrictEqual(c224.decompressMany(onDevice.xs, onDevice.parities), there);
    const dev = c224.liftX(xs, parities, { device: true });
    assert.deepStrictEqual(Array.from(dev.flags.toBuffer()), lifted.map(pt => (pt === null ? 0 : 1)));
    assert.deepStrictEqual(c224.containsMany(dev.points), lifted.map(pt => pt !== null));     // (0, 0), where there is no point, is not on this curve
    assert.deepStrictEqual(f224.sqrtVectorElements([]).roots.toValues(), []);
    assert.deepStrictEqual(c224.liftX([]), []);
    const plan = [0, 1, 2, 3].map(() => Buffer.alloc(4));
    f224.lib.call('gs_field_sqrt_plan', f224.ctx, ...plan);
    assert.deepStrictEqual(plan.slice(0, 3).map(b => b.readUInt32LE(0)), [96, 8, 12]);
    assert.throws(() => f224.sqrtVectorElements([f224.modulus]), /canonical/);
    assert.throws(() => c224.liftX([1n, 2n], [0]), /one parity each/);
    assert.throws(() => c224.liftX([1n], [2]), /parities are 0 or 1/);
    assert.throws(() => c224.decompressMany([1n]), /needs the parities/);
    assert.throws(() => c224.compressMany([[c224.G[0], c224.G[1] ^ 1n]]), /not a finite point/);
    const v = f224.newVectorFrom(values);
    assert.throws(() => f224.lib.call('gs_field_sqrt', f224.ctx, v.ptr, 2 ** 20 + 1, v.ptr, v.ptr), /at most 2\^20/);
}
console.log(`js sqrt (${mode}) OK`);
