'use strict';
// tests/js_hades.js <hip|double> <expectations.json> — js/hades.js against values the Python host computed (tests/test_hades.py writes
// them): per field a width-6 Poseidon hash (x^5, 8 + 55 rounds) over rows of four inputs with its tree of pairs, and a width-3 hash
// (x^3, 8 + 5 rounds) with its tree of single elements.  Two fields in one process.
//   hip:    createHash's host function, hashMany, MerkleTree, MerkleTree2 (nodes, root, prove, proveMany, verify)
//   double: a library without the optional entry points — the host function still equals the Python values, the device members throw an
//           Error that says what is missing
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const ROOT = path.resolve(__dirname, '..');
const galois = require(path.join(ROOT, 'js', 'galois.js'));
const hades = require(path.join(ROOT, 'js', 'hades.js'));

const mode = process.argv[2];
const want = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const big = x => (Array.isArray(x) ? x.map(big) : BigInt(x));

assert.strictEqual(want.length, 2);
for (const rec of want) {
    const f = galois.createPrimeField(BigInt(rec.modulus));
    const rows = big(rec.rows), digests = big(rec.digests), pairs = big(rec.pairs), singles = big(rec.singles);
    const h6 = hades.createHash(f, 5n, 8, 55, 6), h3 = hades.createHash(f, 3n, 8, 5, 3);
    for (let i = 0; i < 5; i++) assert.deepStrictEqual(h6(rows[i]), digests[i]);
    if (mode === 'double') {
        assert.strictEqual(f.lib.has('gs_hades_hash'), false);
        for (const attempt of [() => h6.hashMany(rows), () => new hades.MerkleTree(pairs, h6), () => new hades.MerkleTree2(singles, h3)]) {
            assert.throws(attempt, e => e.constructor === Error && /no gs_hades_\* entry points/.test(e.message));
        }
        continue;
    }
    assert.strictEqual(f.lib.has('gs_hades_hash'), true);
    assert.deepStrictEqual(h6.hashMany(rows).toValues(), digests);
    assert.deepStrictEqual(h6.hashMany(f.newMatrixFrom(rows), 1).toValues(), digests.map(d => d.slice(0, 1)));

    const t2 = new hades.MerkleTree(pairs, h6), pairNodes = big(rec.pairNodes);            // nodes 1 .. 2n - 1
    assert.deepStrictEqual(t2.nodes.slice(1), pairNodes);
    assert.strictEqual(t2.nodes[0], undefined);
    assert.deepStrictEqual(t2.root, pairNodes[0]);
    const t1 = new hades.MerkleTree2(f.newVectorFrom(singles), h3), singleNodes = big(rec.singleNodes);
    assert.deepStrictEqual(t1.nodes.slice(1), singleNodes);
    assert.strictEqual(t1.root, singleNodes[0]);
    for (const [tree, nodes, cls, h] of [[t2, pairNodes, hades.MerkleTree, h6], [t1, singleNodes, hades.MerkleTree2, h3]]) {
        const n = tree.leafCount, indexes = [0, n - 1, 3, 3, 5];
        const paths = tree.proveMany(indexes);
        indexes.forEach((index, k) => {
            const expect = [nodes[n + index - 1]];
            for (let at = n + index; at > 1; at >>= 1) expect.push(nodes[(at ^ 1) - 1]);
            assert.deepStrictEqual(paths[k], expect);
            assert.deepStrictEqual(tree.prove(index), expect);
            assert.strictEqual(cls.verify(tree.root, index, paths[k], h), true);
            const bad = paths[k].slice();
            bad[1] = Array.isArray(bad[1]) ? [bad[1][0], bad[1][1] ^ 1n] : bad[1] ^ 1n;
            assert.strictEqual(cls.verify(tree.root, index, bad, h), false);
        });
        assert.throws(() => tree.proveMany([n]), /outside/);
    }
    assert.throws(() => new hades.MerkleTree(pairs.slice(0, 3), h6), /power of two/);
    assert.throws(() => new hades.MerkleTree(pairs, h3), /do not fit/);
}
console.log(`js hades (${mode}) OK`);
