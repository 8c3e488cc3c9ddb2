'use strict';
// tests/js_tree_update.js <hip|double> <expectations.json> — update / updateMany of the device trees of js/hades.js and js/rescue.js
// against values the Python host computed (tests/test_tree_update.py writes them): per field a tree of pairs, a tree of single
// elements and a Rescue tree of 16 leaves each, and one batch with a repeated index, a sibling pair back to back and an update that
// changes nothing.  Two fields in one process.
//   hip:    every record's `before` and `root`, the nodes afterwards, prove after the update, update() = updateMany of one, the
//           refusals (lengths, a leaf of the wrong shape, an index outside the leaves), an empty batch
//   double: a library without the optional entry points — the members throw an Error that names what is missing
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const ROOT = path.resolve(__dirname, '..');
const galois = require(path.join(ROOT, 'js', 'galois.js'));
const hades = require(path.join(ROOT, 'js', 'hades.js'));
const rescue = require(path.join(ROOT, 'js', 'rescue.js'));
const { DeviceTree } = require(path.join(ROOT, 'js', 'field_tree.js'));

const mode = process.argv[2];
const want = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const big = x => (Array.isArray(x) ? x.map(big) : BigInt(x));

assert.strictEqual(want.length, 2);
for (const rec of want) {
    const f = galois.createPrimeField(BigInt(rec.modulus));
    const indexes = rec.indexes;
    if (mode === 'double') {
        // no tree can be built on this library; the members are asked on a stand-in that holds what they look at first
        for (const symbol of ['gs_hades_merkle_update', 'gs_rescue_merkle_update']) {
            assert.strictEqual(f.lib.has(symbol), false);
            const standIn = Object.assign(Object.create(DeviceTree.prototype), { field: f, _update: { symbol } });
            for (const attempt of [() => standIn.updateMany([0], [1n]), () => standIn.update(0, 1n), () => standIn.updateMany([], [])]) {
                assert.throws(attempt, e => e.constructor === Error && new RegExp(`no ${symbol} entry point`).test(e.message));
            }
        }
        continue;
    }
    const h6 = hades.createHash(f, 5n, 8, 55, 6), h3 = hades.createHash(f, 3n, 8, 5, 3);
    const r = rec.rescue, hr = rescue.createRescue(f, BigInt(r.alpha), BigInt(r.invAlpha), 4, r.rounds, big(r.mds), big(r.constants));
    const cases = [['pairs', leaves => new hades.MerkleTree(leaves, h6)], ['singles', leaves => new hades.MerkleTree2(leaves, h3)], ['rescued', leaves => hr.merkleTree(leaves)]];
    for (const [key, build] of cases) {
        const w = rec[key], leaves = big(w.leaves), fresh = big(w.new), before = big(w.before), roots = big(w.roots), nodes = big(w.nodes);
        const tree = build(leaves), n = tree.leafCount;
        assert.strictEqual(f.lib.has(tree._update.symbol), true);
        const records = tree.updateMany(indexes, fresh);
        assert.deepStrictEqual(records.map(x => x.before), before, key);
        assert.deepStrictEqual(records.map(x => x.root), roots, key);
        assert.deepStrictEqual(tree.nodes.slice(1), nodes, key);
        assert.deepStrictEqual(tree.root, roots[roots.length - 1]);
        assert.deepStrictEqual(tree.prove(indexes[0])[0], nodes[n + indexes[0] - 1]);
        // one at a time on a second tree: the same records; then the leaf a position holds: nothing changes
        const again = build(leaves);
        indexes.forEach((index, j) => assert.deepStrictEqual(again.update(index, fresh[j]), records[j], key));
        assert.deepStrictEqual(again.nodes, tree.nodes);
        const held = again.prove(3), root = again.root;
        assert.deepStrictEqual(again.update(3, held[0]), { before: held, root });
        assert.deepStrictEqual(again.nodes, tree.nodes);
        // leaves already on the device
        const third = build(leaves);
        const src = key === 'pairs' ? f.newMatrixFrom(fresh) : (key === 'singles' ? f.newMatrixFrom(fresh.map(v => [v])) : f.newVectorFrom(fresh));
        assert.deepStrictEqual(third.updateMany(indexes, src), records, key);
        // refusals, and an empty batch
        assert.deepStrictEqual(tree.updateMany([], []), []);
        assert.throws(() => tree.updateMany([0, 1], [fresh[0]]), /2 indexes and 1 leaves/);
        assert.throws(() => tree.updateMany([n], [fresh[0]]), /outside/);
        if (key === 'pairs') assert.throws(() => tree.updateMany([0], f.newMatrixFrom([[1n]])), /2 elements each/);
        assert.deepStrictEqual(tree.nodes.slice(1), nodes, key);
    }
}
console.log(`js tree_update (${mode}) OK`);
