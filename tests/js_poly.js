'use strict';
// tests/js_poly.js <hip|double> <expectations.json> — polyFromRoots / divPolys / divModPolys / evalPolyAtPoints / interpolateAtPoints of
// js/galois.js against values the Python host computed by the schoolbook definitions (tests/test_poly.py writes them): 257 points and
// (600, 299) coefficients in the 128-bit field, where the tree has levels on both sides of its switch-over.
//   hip:    the members, from arrays of BigInts and from device Vectors, and the refusals
//   double: a library without the optional entry points — has() is false, the members throw an Error that says what is missing, and
//           interpolate() is what it was
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const ROOT = path.resolve(__dirname, '..');
const galois = require(path.join(ROOT, 'js', 'galois.js'));

const mode = process.argv[2];
const want = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const big = x => x.map(BigInt);
const f = galois.createPrimeField(BigInt(want.modulus));
const xs = big(want.xs), ys = big(want.ys), poly = big(want.poly), a = big(want.a), b = big(want.b);
const ENTRIES = ['gs_poly_from_roots', 'gs_poly_div', 'gs_poly_eval_points', 'gs_poly_interpolate_points'];

// the host route of interpolate() is untouched on either library
assert.deepStrictEqual(f.interpolate(f.newVectorFrom(xs.slice(0, 12)), f.newVectorFrom(ys.slice(0, 12))).toValues(), big(want.few));

if (mode === 'double') {
    for (const name of ENTRIES) assert.strictEqual(f.lib.has(name), false);
    const missing = name => e => e.constructor === Error && e.message.includes(`no ${name} entry point (include/gstark_poly.h)`);
    assert.throws(() => f.polyFromRoots(xs), missing('gs_poly_from_roots'));
    assert.throws(() => f.divModPolys(a, b), missing('gs_poly_div'));
    assert.throws(() => f.divPolys(a, b), missing('gs_poly_div'));
    assert.throws(() => f.evalPolyAtPoints(poly, xs, 'tree'), missing('gs_poly_eval_points'));
    assert.throws(() => f.interpolateAtPoints(xs, ys), missing('gs_poly_interpolate_points'));
} else {
    for (const name of ENTRIES) assert.strictEqual(f.lib.has(name), true);
    assert.deepStrictEqual(f.polyFromRoots(xs).toValues(), big(want.from_roots));
    assert.deepStrictEqual(f.polyFromRoots(f.newVectorFrom(xs)).toValues(), big(want.from_roots));
    assert.deepStrictEqual(f.polyFromRoots([]).toValues(), [1n]);
    const [q, r] = f.divModPolys(a, b);
    assert.deepStrictEqual(q.toValues(), big(want.q));
    assert.deepStrictEqual(r.toValues(), big(want.r));
    assert.deepStrictEqual(f.divPolys(f.newVectorFrom(a), f.newVectorFrom(b)).toValues(), big(want.q));
    const values = f.evalPolyAtPoints(poly, xs, 'tree');
    assert.deepStrictEqual(values.toValues(), big(want.values));
    assert.deepStrictEqual(f.evalPolyAtPoints(poly, xs, 'horner').toValues(), big(want.values));
    assert.deepStrictEqual(f.evalPolyAtPoints(f.newVectorFrom(poly), f.newVectorFrom(xs)).toValues(), big(want.values));
    assert.deepStrictEqual(f.interpolateAtPoints(xs.slice(0, 12), ys.slice(0, 12)).toValues(), big(want.few));
    const through = f.interpolateAtPoints(f.newVectorFrom(xs), ys);
    assert.strictEqual(through.length, 257);
    assert.deepStrictEqual(f.evalPolyAtPoints(through, xs, 'tree').toValues(), ys);
    assert.deepStrictEqual(f.evalPolyAtPoints(through, xs, 'horner').toValues(), ys);
    assert.throws(() => f.interpolateAtPoints([1n, 2n, 1n], [3n, 4n, 5n]), /two of the x coordinates are equal/);
    assert.throws(() => f.interpolateAtPoints([1n, 2n], [3n]), /same as number of y/);
    assert.throws(() => f.divModPolys([1n, 2n, 3n], [5n, 0n]), /leading coefficient/);
    assert.throws(() => f.divModPolys([], [1n]), /at least one coefficient/);
    assert.throws(() => f.evalPolyAtPoints(poly, xs, 'fast'), /method/);
}
console.log(`js poly (${mode}) OK`);
