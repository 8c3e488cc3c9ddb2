'use strict';
// tests/js_rescue.js <hip|double> <expectations.json> — js/rescue.js against values the Python host computed (tests/test_rescue_hash.py
// writes them): per field a width-4 Rescue of random constants (3 rounds) with both sponges over rows of two inputs, hash2 and a tree of
// 16 leaves; for the 128-bit field also key rows of the example's parameter set.  Two fields in one process.
//   hip:    the host members, hashMany in both forms, merkleTree (nodes, root, prove, proveMany, verify)
//   double: a library without the optional entry points — the host members still equal the Python values, the device members throw an
//           Error that says what is missing
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const ROOT = path.resolve(__dirname, '..');
const galois = require(path.join(ROOT, 'js', 'galois.js'));
const rescue = require(path.join(ROOT, 'js', 'rescue.js'));

const mode = process.argv[2];
const want = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const big = x => (Array.isArray(x) ? x.map(big) : BigInt(x));

assert.strictEqual(want.length, 2);
for (const rec of want) {
    const f = galois.createPrimeField(BigInt(rec.modulus));
    const rows = big(rec.rows), modified = big(rec.modified), sponge = big(rec.sponge), leaves = big(rec.leaves), nodes = big(rec.nodes);
    const h = rescue.createRescue(f, BigInt(rec.alpha), BigInt(rec.invAlpha), 4, rec.rounds, big(rec.mds), big(rec.constants));
    assert.deepStrictEqual(h.unrollConstants(), big(rec.keys));
    const grouped = h.groupConstants(h.unrollConstants());
    assert.strictEqual(grouped.roundConstants.length, 8);
    assert.deepStrictEqual(grouped.roundConstants[5][1], big(rec.keys)[5][1]);
    assert.deepStrictEqual(h.sponge(rows[2]).trace, big(rec.trace));
    for (let i = 0; i < 5; i++) {
        assert.deepStrictEqual(h.modifiedSponge(rows[i]).hash, modified[i]);
        assert.deepStrictEqual(h.sponge(rows[i]).hash, sponge[i]);
    }
    assert.strictEqual(h.hash2(leaves[0], leaves[1]), nodes[7]);                          // node 8 = hash2(leaf 0, leaf 1); nodes[] starts at node 1
    assert.throws(() => rescue.createRescue(f, 3n, BigInt(rec.invAlpha), 9, 3, big(rec.mds), big(rec.constants)), /outside 2 \.\. 8/);
    assert.throws(() => rescue.createRescue(f, 3n, BigInt(rec.invAlpha), 4, 3, big(rec.mds), big(rec.constants).slice(1)), /key constants/);
    if (rec.exampleKeys) {
        const P = rec.example;
        const ex = rescue.createRescue(f, 3n, -BigInt(P.invAlpha), 4, 32, big(P.mds), big(P.constants));
        const keys = ex.unrollConstants();
        assert.strictEqual(keys.length, 67);
        assert.deepStrictEqual(keys.slice(0, 3).concat(keys.slice(-1)), big(rec.exampleKeys));
    }
    if (mode === 'double') {
        assert.strictEqual(f.lib.has('gs_rescue_hash'), false);
        for (const attempt of [() => h.hashMany(rows), () => h.merkleTree(leaves), () => new rescue.MerkleTree(f.newVectorFrom(leaves), h)]) {
            assert.throws(attempt, e => e.constructor === Error && /no gs_rescue_\* entry points/.test(e.message));
        }
        continue;
    }
    assert.strictEqual(f.lib.has('gs_rescue_hash'), true);
    for (const form of [0, 1, 2]) {
        assert.deepStrictEqual(h.hashMany(rows, 2, true, form).toValues(), modified);
        assert.deepStrictEqual(h.hashMany(f.newMatrixFrom(rows), 1, false, form).toValues(), sponge.map(d => d.slice(0, 1)));
    }
    assert.deepStrictEqual(h.hashMany(rows).toValues(), modified.map(d => d.slice(0, 1)));

    const tree = h.merkleTree(f.newVectorFrom(leaves));
    assert.deepStrictEqual(tree.nodes.slice(1), nodes);
    assert.strictEqual(tree.nodes[0], undefined);
    assert.strictEqual(tree.root, nodes[0]);
    assert.deepStrictEqual(new rescue.MerkleTree(leaves, h).nodes.slice(1), nodes);
    const n = tree.leafCount, indexes = [0, n - 1, 3, 3, 5];
    const paths = tree.proveMany(indexes);
    indexes.forEach((index, k) => {
        const expect = [nodes[n + index - 1]];
        for (let at = n + index; at > 1; at >>= 1) expect.push(nodes[(at ^ 1) - 1]);
        assert.deepStrictEqual(paths[k], expect);
        assert.deepStrictEqual(tree.prove(index), expect);
        assert.strictEqual(rescue.MerkleTree.verify(tree.root, index, paths[k], h.hash2), true);
        const bad = paths[k].slice();
        bad[1] ^= 1n;
        assert.strictEqual(rescue.MerkleTree.verify(tree.root, index, bad, h.hash2), false);
    });
    assert.throws(() => tree.proveMany([n]), /outside/);
    assert.throws(() => h.merkleTree(leaves.slice(0, 3)), /power of two/);
    assert.throws(() => h.hashMany(rows, 3), /digest/);
}
console.log(`js rescue (${mode}) OK`);
