'use strict';
// tests/js_scan.js <hip|double> <expectations.json> — the scan members of js/galois.js (prefixSum* / prefixProduct* / sum* / prod* /
// linearRecurrence* / scanPlan) against values the Python host computed (tests/test_scan.py writes them): the three ops, inclusive and
// exclusive, one vector, uniform and flagged segments, at T + 1 and 2T + 1 elements of the 128-bit field.
//   hip:    the same values as the definitions give (and so the same bytes as the Python members), from arrays and from device objects,
//           and the refusals
//   double: a library without the optional entry points — every member throws an Error that says what is missing
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const ROOT = path.resolve(__dirname, '..');
const galois = require(path.join(ROOT, 'js', 'galois.js'));

const mode = process.argv[2];
const want = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const big = x => (Array.isArray(x) ? x.map(big) : BigInt(x));
const f = galois.createPrimeField(BigInt(want.modulus));
const nested = (flat, cols) => { const out = []; for (let r = 0; r * cols < flat.length; r++) out.push(flat.slice(r * cols, (r + 1) * cols)); return out; };
const flatten = m => [].concat(...m.toValues());

if (mode === 'double') {
    assert.strictEqual(f.lib.has('gs_scan'), false);
    const tries = {
        gs_scan: [() => f.prefixSumVectorElements([1n]), () => f.prefixProductVectorElements([1n]), () => f.prefixSumMatrixRows([[1n]]), () => f.prefixProductMatrixRows([[1n]])],
        gs_reduce: [() => f.sumVectorElements([1n]), () => f.prodVectorElements([1n]), () => f.sumMatrixRows([[1n]]), () => f.prodMatrixRows([[1n]])],
        gs_scan_affine: [() => f.linearRecurrence(1n, [1n]), () => f.linearRecurrenceMatrixRows(1n, [[1n]])],
        gs_scan_plan: [() => f.scanPlan()],
    };
    for (const symbol of Object.keys(tries)) {
        for (const attempt of tries[symbol]) {
            assert.throws(attempt, e => e.constructor === Error && new RegExp(`no ${symbol} entry point \\(include/gstark_scan\\.h\\)`).test(e.message));
        }
    }
} else {
    for (const symbol of ['gs_scan', 'gs_scan_affine', 'gs_reduce', 'gs_scan_plan']) assert.strictEqual(f.lib.has(symbol), true);
    const plan = f.scanPlan();
    assert.deepStrictEqual(plan, { tile: want.tile, elementsPerThread: want.tile / 256, maxElements: 2 ** 24, launches: 0 });
    assert.deepStrictEqual([1, want.tile, want.tile + 1, 2 ** 24, 2 ** 24 + 1].map(n => f.scanPlan(n).launches), [1, 1, 3, 3, 0]);
    assert.deepStrictEqual(want.cases.map(c => c.n), [want.tile + 1, 2 * want.tile + 1]);
    for (const c of want.cases) {
        const values = big(c.values), factors = big(c.factors), x0 = BigInt(c.x0), n = c.n, rows = n / c.cols;
        const vec = f.newVectorFrom(values), avec = f.newVectorFrom(factors), heads = new galois.Vector(f, n, undefined, 0n, 1);
        f.lib.call('gs_upload', f.ctx, heads.ptr, Buffer.from(c.heads), n);
        const mat = f.newMatrixFrom(nested(values, c.cols)), amat = f.newMatrixFrom(nested(factors, c.cols));
        for (const exclusive of [false, true]) {
            const form = exclusive ? 'exclusive' : 'inclusive';
            const get = key => big(c.want[`${key}/${form}`]);
            // one vector: from device vectors and from arrays
            assert.deepStrictEqual(f.prefixSumVectorElements(vec, exclusive).toValues(), get('sum/vector'));
            assert.deepStrictEqual(f.prefixSumVectorElements(values, exclusive).toValues(), get('sum/vector'));
            assert.deepStrictEqual(f.prefixProductVectorElements(vec, exclusive).toValues(), get('product/vector'));
            assert.deepStrictEqual(f.linearRecurrence(avec, vec, x0, exclusive).toValues(), get('affine/vector'));
            assert.deepStrictEqual(f.linearRecurrence(factors, values, x0, exclusive).toValues(), get('affine/vector'));
            assert.deepStrictEqual(f.linearRecurrence(factors[0], vec, x0, exclusive).toValues(), get('scalar/vector'));
            // flagged segments: a device vector of bytes and an array
            assert.deepStrictEqual(f.prefixSumVectorElements(vec, exclusive, heads).toValues(), get('sum/flagged'));
            assert.deepStrictEqual(f.prefixProductVectorElements(vec, exclusive, c.heads).toValues(), get('product/flagged'));
            assert.deepStrictEqual(f.linearRecurrence(avec, vec, x0, exclusive, heads).toValues(), get('affine/flagged'));
            assert.deepStrictEqual(f.linearRecurrence(factors[0], vec, x0, exclusive, c.heads).toValues(), get('scalar/flagged'));
            // uniform segments
            assert.deepStrictEqual(flatten(f.prefixSumMatrixRows(mat, exclusive)), get('sum/uniform'));
            const both = f.prefixProductMatrixRows(mat, exclusive, true);
            assert.deepStrictEqual(flatten(both.matrix), get('product/uniform'));
            assert.deepStrictEqual(both.totals.toValues(), big(c.totals.product));
            assert.deepStrictEqual(flatten(f.linearRecurrenceMatrixRows(amat, mat, x0, exclusive)), get('affine/uniform'));
            assert.deepStrictEqual(flatten(f.linearRecurrenceMatrixRows(factors[0], mat, x0, exclusive)), get('scalar/uniform'));
        }
        assert.deepStrictEqual(f.sumMatrixRows(mat).toValues(), big(c.totals.sum));
        assert.deepStrictEqual(f.prodMatrixRows(mat).toValues(), big(c.totals.product));
        assert.strictEqual(f.sumMatrixRows(mat).length, rows);
        const sums = big(c.want['sum/vector/inclusive']), products = big(c.want['product/vector/inclusive']);
        assert.strictEqual(f.sumVectorElements(vec), sums[n - 1]);
        assert.strictEqual(f.prodVectorElements(values), products[n - 1]);
        assert.deepStrictEqual(vec.toValues(), values);
    }
    assert.deepStrictEqual(f.prefixSumVectorElements([]).toValues(), []);
    assert.strictEqual(f.sumVectorElements([]), 0n);
    assert.strictEqual(f.prodVectorElements([]), 1n);
    assert.throws(() => f.prefixSumVectorElements([f.modulus]), /canonical/);
    assert.throws(() => f.linearRecurrence([1n, 2n], [1n]), /lengths differ/);
    assert.throws(() => f.linearRecurrence(f.modulus, [1n]), /canonical/);
    assert.throws(() => f.linearRecurrence(1n, [1n], 5), /x0 is a BigInt/);
    assert.throws(() => f.prefixSumVectorElements([1n, 2n], false, [1]), /1 heads and 2 values/);
    assert.throws(() => f.prefixSumVectorElements([1n, 2n], false, f.newVectorFrom([1n, 0n])), /vector of bytes/);
    assert.throws(() => f.prefixSumMatrixRows([[1n, 2n], [3n]]), /different lengths/);
    assert.throws(() => f.linearRecurrenceMatrixRows([[1n, 2n]], [[1n], [2n]]), /shapes differ/);
    const v = f.newVectorFrom([1n, 2n, 3n]);
    assert.throws(() => f.lib.call('gs_scan', f.ctx, 0, 0, v.ptr, 0n, 1, 2 ** 24 + 1, v.ptr, 0n), /at most 2\^24/);
    assert.throws(() => f.lib.call('gs_scan', f.ctx, 2, 0, v.ptr, 0n, 1, 3, v.ptr, 0n), /op is GS_SCAN_SUM or GS_SCAN_PRODUCT/);
    assert.throws(() => f.lib.call('gs_scan', f.ctx, 0, 0, v.ptr, 0n, 3, 0, v.ptr, 0n), /cols is 0/);
    assert.deepStrictEqual(f.prefixSumVectorElements(v).toValues(), [1n, 3n, 6n]);      // the context is as usable as before
}
console.log(`js scan (${mode}) OK`);
