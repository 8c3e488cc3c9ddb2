'use strict';
// tests/js_absorb.js <hip|double> <expectations.json> — absorb / absorbMany of js/hades.js and js/rescue.js (include/gstark_absorb.h) against
// values the Python host computed (tests/test_absorb.py writes them): per field a width-6 Poseidon hash (x^5, 8 + 55 rounds) and a width-4
// Rescue of random constants (3 rounds) over records of 1, 4, 5 and 11 elements.  Two fields in one process.
//   hip:    the host members, absorbMany by rows and by columns, from BigInts and from device matrices, the refusals
//   double: a library without the optional entry points — the host members still equal the Python values, the device members throw an
//           Error that names the missing entry
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const ROOT = path.resolve(__dirname, '..');
const galois = require(path.join(ROOT, 'js', 'galois.js'));
const hades = require(path.join(ROOT, 'js', 'hades.js'));
const rescue = require(path.join(ROOT, 'js', 'rescue.js'));

const mode = process.argv[2];
const want = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const big = x => (Array.isArray(x) ? x.map(big) : BigInt(x));
const transposed = rows => rows[0].map((_, i) => rows.map(r => r[i]));

assert.strictEqual(want.length, 2);
for (const rec of want) {
    const f = galois.createPrimeField(BigInt(rec.modulus));
    const h = hades.createHash(f, 5n, 8, 55, 6);
    const r = rescue.createRescue(f, 3n, BigInt(rec.invAlpha), 4, 3, big(rec.mds), big(rec.constants));
    for (const c of rec.cases) {
        const rows = big(c.rows);
        // the host members: defaults (Poseidon: two elements at rate 4; Rescue: one element at rate 2, modifiedSponge) and explicit arguments
        rows.slice(0, 4).forEach((row, k) => {
            assert.deepStrictEqual(h.absorb(row), big(c.hades[k]));
            assert.deepStrictEqual(h.absorb(row, 1, 1), big(c.hadesRate1[k]));
            assert.deepStrictEqual(r.absorb(row), big(c.rescue[k]));
            assert.deepStrictEqual(r.absorb(row, 2, 3, false), big(c.rescueSponge[k]));
        });
        if (mode === 'double') {
            assert.strictEqual(f.lib.has('gs_hades_absorb'), false);
            assert.strictEqual(f.lib.has('gs_rescue_absorb'), false);
            assert.throws(() => h.absorbMany(rows), e => e.constructor === Error && /no gs_hades_absorb entry point \(include\/gstark_absorb\.h\)/.test(e.message));
            assert.throws(() => r.absorbMany(rows), e => e.constructor === Error && /no gs_rescue_absorb entry point \(include\/gstark_absorb\.h\)/.test(e.message));
            continue;
        }
        assert.strictEqual(f.lib.has('gs_hades_absorb'), true);
        assert.strictEqual(f.lib.has('gs_rescue_absorb'), true);
        const columns = transposed(rows);
        assert.deepStrictEqual(h.absorbMany(rows).toValues(), big(c.hades));
        assert.deepStrictEqual(h.absorbMany(f.newMatrixFrom(rows), 1, 1).toValues(), big(c.hadesRate1));
        assert.deepStrictEqual(h.absorbMany(columns, 2, undefined, true).toValues(), big(c.hades));
        assert.deepStrictEqual(h.absorbMany(f.newMatrixFrom(columns), 1, 1, true).toValues(), big(c.hadesRate1));
        assert.deepStrictEqual(r.absorbMany(rows).toValues(), big(c.rescue));
        assert.deepStrictEqual(r.absorbMany(f.newMatrixFrom(rows), 2, 3, false, false).toValues(), big(c.rescueSponge));
        assert.deepStrictEqual(r.absorbMany(columns, 1, undefined, true).toValues(), big(c.rescue));
        assert.deepStrictEqual(r.absorbMany(f.newMatrixFrom(columns), 2, 3, true, false).toValues(), big(c.rescueSponge));
    }
    // the length separates what zero padding does not, and the refusals of the host members
    assert.deepStrictEqual(h([7n]), h([7n, 0n]));
    assert.notDeepStrictEqual(h.absorb([7n]), h.absorb([7n, 0n]));
    assert.notDeepStrictEqual(r.absorb([7n]), r.absorb([7n, 0n]));
    assert.notDeepStrictEqual(h.absorb([7n, 8n]), h([7n, 8n]));
    for (const attempt of [() => h.absorb([1n], 2, 0), () => h.absorb([1n], 2, 6), () => h.absorb([1n], 2, 1), () => h.absorb([1n], 3), () => h.absorb([]),
                           () => r.absorb([1n], 1, 4), () => r.absorb([1n], 2, 1), () => r.absorb([])]) {
        assert.throws(attempt, /^Error: absorb: /);
    }
    if (mode === 'hip') {
        assert.throws(() => h.absorbMany([[1n, 2n], [1n]]), /absorb: every row has the same number/);
        assert.throws(() => h.absorbMany([[1n, 2n]], 2, 6), /absorb: a rate of 6/);
    }
}
console.log(`js absorb (${mode}) OK`);
