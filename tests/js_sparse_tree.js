'use strict';
// tests/js_sparse_tree.js <hip|double> <expectations.json> — the sparse trees of js/hades.js and js/rescue.js against values the Python
// host computed (tests/test_sparse_tree.py writes them): per field, at depth 3 and 36, a tree of pairs, a tree of single elements and a
// Rescue tree with one batch each — repeats, a sibling pair, indexes above 2^32, a leaf set back to `empty` — and paths of set and
// absent indexes.  Two fields in one process.
//   hip:    every record's `before` and `root`, empties, root, the paths (non-membership ones included) as values and through the static
//           verifyMany on the device Matrix, indexes as Numbers and as BigInts, update() = updateMany of one, the refusals
//   double: a library without the optional entry points — the constructors throw an Error that names what is missing
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

assert.strictEqual(want.length, 2);
for (const rec of want) {
    const f = galois.createPrimeField(BigInt(rec.modulus));
    const h6 = hades.createHash(f, 5n, 8, 55, 6), h3 = hades.createHash(f, 3n, 8, 5, 3);
    const r = rec.rescue, hr = rescue.createRescue(f, BigInt(r.alpha), BigInt(r.invAlpha), 4, r.rounds, big(r.mds), big(r.constants));
    const build = { pairs: (depth, empty) => new hades.SparseMerkleTree(depth, h6, empty, 1), singles: (depth, empty) => new hades.SparseMerkleTree2(depth, h3, empty, 1),
        rescued: (depth, empty) => hr.sparseMerkleTree(depth, empty, 1) };
    if (mode === 'double') {
        for (const [key, symbol] of [['pairs', 'gs_hades_sparse_create'], ['singles', 'gs_hades_sparse_create'], ['rescued', 'gs_rescue_sparse_create']]) {
            assert.strictEqual(f.lib.has(symbol), false);
            assert.throws(() => build[key](3, null), e => e.constructor === Error && new RegExp(`no ${symbol} entry point \\(include/gstark_sparse_tree.h\\)`).test(e.message));
        }
        continue;
    }
    assert.strictEqual(rec.trees.length, 6);
    for (const w of rec.trees) {
        const key = w.kind, depth = w.depth, empty = w.empty === null ? null : big(w.empty);
        const indexes = w.indexes.map(Number), fresh = big(w.new), before = big(w.before), roots = big(w.roots), probe = w.probe.map(Number), paths = big(w.paths);
        if (depth === 36) assert.ok(indexes.some(i => i > 2 ** 32) && probe.some(i => i > 2 ** 32));
        const tree = build[key](depth, empty), verifier = key === 'pairs' ? hades.SparseMerkleTree : (key === 'singles' ? hades.SparseMerkleTree2 : rescue.SparseMerkleTree);
        const hash = key === 'pairs' ? h6 : (key === 'singles' ? h3 : hr);
        assert.deepStrictEqual(tree.empties, big(w.empties), key);
        assert.deepStrictEqual(tree.root, tree.empties[depth]);
        assert.deepStrictEqual(tree.prove(indexes[3])[0], tree.empties[0]);
        const records = tree.updateMany(indexes, fresh);
        assert.deepStrictEqual(records.map(x => x.before), before, key);
        assert.deepStrictEqual(records.map(x => x.root), roots, key);
        assert.deepStrictEqual(tree.root, roots[roots.length - 1]);
        assert.deepStrictEqual(tree.proveMany(probe), paths, key);                         // set and absent indexes
        assert.deepStrictEqual(tree.proveMany(probe.map(BigInt)), paths, key);             // ... given as BigInts
        assert.deepStrictEqual(tree.get(indexes[3]), fresh[3]);
        assert.deepStrictEqual(verifier.verifyMany(tree.root, probe, tree.proveMany(probe, true), hash), probe.map(() => true), key);
        assert.deepStrictEqual(verifier.verifyUpdates(tree.empties[depth], indexes, fresh, records, hash), indexes.map(() => true), key);
        // one at a time on a second tree, indexes as BigInts: the same records
        const again = build[key](depth, empty);
        indexes.forEach((index, j) => assert.deepStrictEqual(again.update(BigInt(index), fresh[j]), records[j], key));
        assert.deepStrictEqual(again.root, tree.root);
        // refusals, and an empty batch
        const root = tree.root;
        assert.deepStrictEqual(tree.updateMany([], []), []);
        assert.deepStrictEqual(tree.proveMany([]), []);
        assert.throws(() => tree.updateMany([0, 1], [fresh[0]]), /2 indexes and 1 leaves/);
        assert.throws(() => tree.updateMany([2 ** depth], [fresh[0]]), /outside of the 2\^/);
        assert.throws(() => tree.proveMany([-1]), /outside/);
        assert.throws(() => tree.proveMany([1n << BigInt(depth)]), /outside/);
        assert.throws(() => tree.proveMany([0.5]), /outside/);
        assert.throws(() => tree.proveMany(new Array(2 ** 20 + 1).fill(0)), /at most 2\^20 paths/);
        assert.throws(() => tree.updateMany([0], [key === 'pairs' ? 1n : [1n, 2n]]), /each/);
        assert.throws(() => build[key](37, empty), /depth of 1 .. 36/);
        assert.throws(() => build[key](0, empty), /depth of 1 .. 36/);
        assert.deepStrictEqual(tree.root, root);
    }
}
console.log(`js sparse_tree (${mode}) OK`);
