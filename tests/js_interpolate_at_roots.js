'use strict';
// tests/js_interpolate_at_roots.js <hip|double> — galois.interpolateAtRoots (js/galois.js; gs_boundary_polys through the addon's table).
//   hip:    against interpolate() coefficient by coefficient up to 4 096 points (a generator of the domain that is NOT getRootOfUnity's
//           among them), beyond 4 096 points against the definition (Horner at sampled points) where interpolate() refuses, and
//           interpolate() itself routed to the device for a whole power series of 8 192 points.
//   double: a library without the optional entry point: has() says so, interpolateAtRoots throws, interpolate() behaves as before
//           (its 4 096 cap and error included).
const path = require('path');
const assert = require('assert');
const ROOT = path.resolve(__dirname, '..');
const galois = require(path.join(ROOT, 'js', 'galois.js'));

const mode = process.argv[2];
const P = 2n ** 128n - 9n * 2n ** 32n + 1n;
const f = galois.createPrimeField(P);
let seed = 12345n;
const rnd = () => { seed = (seed * 6364136223846793005n + 1442695040888963407n) % (1n << 64n); return seed; };
const sample = (n, m) => { const all = Array.from({ length: n }, (_, i) => i); for (let i = 0; i < m; i++) { const j = i + Number(rnd() % BigInt(n - i)); [all[i], all[j]] = [all[j], all[i]]; } return all.slice(0, m); };
const horner = (coef, x) => { let acc = 0n; for (let k = coef.length - 1; k >= 0; k--) acc = (acc * x + coef[k]) % P; return acc; };

if (mode === 'double') {
    assert.strictEqual(f.lib.has('gs_boundary_polys'), false);
    assert.strictEqual(f.lib.has('gs_small_interpolate'), true);
    const ys = f.newVectorFrom([1n, 2n, 3n]);
    assert.throws(() => f.interpolateAtRoots(f.getRootOfUnity(8), 8, [0, 3, 5], ys), /symbol not found|gs_boundary_polys/);
    const xs = f.getPowerSeries(f.getRootOfUnity(8), 8), y8 = f.newVectorFrom([5n, 4n, 3n, 2n, 1n, 9n, 8n, 7n]);
    const coef = f.interpolate(xs, y8).toValues();          // the host path, as before
    const g = f.getRootOfUnity(8);
    for (let i = 0; i < 8; i++) assert.strictEqual(horner(coef, f.exp(g, BigInt(i))), y8.toValues()[i]);
    const big = f.getPowerSeries(f.getRootOfUnity(8192), 8192);
    assert.throws(() => f.interpolate(big, big), /gs_small_interpolate failed/);
    console.log('js interpolateAtRoots (double) OK');
} else {
    assert.strictEqual(f.lib.has('gs_boundary_polys'), true);
    for (const [order, m, odd] of [[256, 5, 1n], [4096, 1000, 1n], [4096, 4096, 1n], [1024, 300, 77n], [1 << 14, 6000, 1n], [1 << 14, 1 << 14, 5n]]) {
        const g = f.exp(f.getRootOfUnity(order), odd);       // odd power: another generator of the same domain
        const pos = sample(order, m), yv = pos.map(() => rnd() * rnd() % P);
        const got = f.interpolateAtRoots(g, order, pos, f.newVectorFrom(yv));
        assert.strictEqual(got.length, m);
        const coef = got.toValues();
        const xv = pos.map(s => f.exp(g, BigInt(s)));
        if (m <= 4096) assert.deepStrictEqual(coef, f.interpolate(f.newVectorFrom(xv), f.newVectorFrom(yv)).toValues(), `order ${order}, m ${m}`);
        else assert.throws(() => f.interpolate(f.newVectorFrom(xv), f.newVectorFrom(yv)), /gs_small_interpolate failed/);
        for (const i of sample(m, Math.min(m, 12))) assert.strictEqual(horner(coef, xv[i]), yv[i], `order ${order}, m ${m}, point ${i}`);
    }
    // interpolate() of a whole power series: routed to the device, the same polynomial as interpolateRoots
    const n = 8192, xs = f.getPowerSeries(f.getRootOfUnity(n), n), ys = f.newVectorFrom(Array.from({ length: n }, () => rnd() * rnd() % P));
    assert.deepStrictEqual(f.interpolate(xs, ys).toValues(), f.interpolateRoots(xs, ys).toValues());
    assert.throws(() => f.interpolateAtRoots(f.getRootOfUnity(8), 8, [1, 1, 2], f.newVectorFrom([1n, 2n, 3n])), /asserted twice/);
    console.log('js interpolateAtRoots (hip) OK');
}
