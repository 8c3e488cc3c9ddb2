'use strict';
// tests/js_tree_verify.js <hip|double> <expectations.json> — the static members pathRoots / verifyMany / verifyUpdates of the tree classes of
// js/hades.js (MerkleTree, MerkleTree2) and js/rescue.js (MerkleTree) against values the Python host computed (tests/test_tree_verify.py
// writes them): per field a tree of pairs, a tree of single elements and a Rescue tree of 16 leaves each, some of their paths, the roots
// the same paths imply under other leaves, and the records of one batch of updates.  Two fields in one process.
//   hip:    the three members on host arrays and on device arrays, one negative of each kind (a sibling, an index bit, the leaf, the
//           root, a record's root, a record's sibling), the refusals, empty input
//   double: a library without the optional entry points — the members throw an Error that names the entry and the header
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
const bump = (node, p) => (Array.isArray(node) ? [node[0], (node[1] + 1n) % p] : (node + 1n) % p);      // (of a pair: only the second element)

assert.strictEqual(want.length, 2);
for (const rec of want) {
    const p = BigInt(rec.modulus), f = galois.createPrimeField(p);
    const indexes = rec.indexes, updates = rec.updates;
    const h6 = hades.createHash(f, 5n, 8, 55, 6), h3 = hades.createHash(f, 3n, 8, 5, 3);
    const r = rec.rescue, hr = rescue.createRescue(f, BigInt(r.alpha), BigInt(r.invAlpha), 4, r.rounds, big(r.mds), big(r.constants));
    const cases = [['pairs', hades.MerkleTree, h6, 'gs_hades_merkle_path_roots'], ['singles', hades.MerkleTree2, h3, 'gs_hades_merkle_path_roots'],
        ['rescued', rescue.MerkleTree, hr, 'gs_rescue_merkle_path_roots']];
    for (const [key, cls, hash, symbol] of cases) {
        const w = rec[key], root = big(w.root), paths = big(w.paths), other = big(w.other), swapped = big(w.swapped);
        const fresh = big(w.new), records = big(w.before).map((before, j) => ({ before, root: big(w.roots)[j] }));
        if (mode === 'double') {
            assert.strictEqual(f.lib.has(symbol), false);
            for (const attempt of [() => cls.pathRoots(hash, indexes, paths), () => cls.verifyMany(root, indexes, paths, hash), () => cls.pathRoots(hash, [], []),
                () => cls.verifyUpdates(root, updates, fresh, records, hash)]) {
                assert.throws(attempt, e => e.constructor === Error && new RegExp(`no ${symbol} entry point \\(include/gstark_tree_verify.h\\)`).test(e.message));
            }
            continue;
        }
        assert.strictEqual(f.lib.has(symbol), true);
        const all = n => new Array(n).fill(true), only = (n, ...bad) => all(n).map((_, k) => !bad.includes(k));
        // paths on the host and on the device, from a tree built here
        const tree = new cls(big(w.leaves), hash);
        assert.deepStrictEqual(tree.root, root, key);
        assert.deepStrictEqual(tree.proveMany(indexes), paths, key);
        assert.deepStrictEqual(cls.pathRoots(hash, indexes, paths), indexes.map(() => root), key);
        assert.deepStrictEqual(cls.verifyMany(root, indexes, paths, hash), all(indexes.length), key);
        const flat = f.newMatrixFrom(paths.map(q => (key === 'pairs' ? [].concat(...q) : q)));
        assert.deepStrictEqual(cls.pathRoots(hash, indexes, flat), indexes.map(() => root), key);
        assert.deepStrictEqual(cls.verifyMany(root, indexes, paths, hash), indexes.map((i, k) => cls.verify(root, i, paths[k], key === 'rescued' ? hr.hash2 : hash)), key);
        // the leaves argument, from the host and from the device
        assert.deepStrictEqual(cls.pathRoots(hash, indexes, paths, other), swapped, key);
        assert.deepStrictEqual(cls.pathRoots(hash, indexes, flat, key === 'pairs' ? f.newMatrixFrom(other) : f.newVectorFrom(other)), swapped, key);
        // one negative of each kind
        const edit = (k, level, node) => paths.map((q, j) => (j === k ? q.map((v, l) => (l === level ? node : v)) : q));
        assert.deepStrictEqual(cls.verifyMany(root, indexes, edit(1, 2, bump(paths[1][2], p)), hash), only(5, 1), key);
        assert.deepStrictEqual(cls.verifyMany(root, indexes, edit(3, 0, bump(paths[3][0], p)), hash), only(5, 3), key);
        assert.deepStrictEqual(cls.verifyMany(root, indexes.map((i, k) => (k === 2 ? i ^ 4 : i)), paths, hash), only(5, 2), key);
        assert.deepStrictEqual(cls.verifyMany(bump(root, p), indexes, paths, hash), only(5, 0, 1, 2, 3, 4), key);
        // the records of a batch of updates
        assert.deepStrictEqual(tree.updateMany(updates, fresh), records, key);
        assert.deepStrictEqual(cls.verifyUpdates(root, updates, fresh, records, hash), all(updates.length), key);
        assert.deepStrictEqual(cls.pathRoots(hash, updates, records.map(x => x.before), fresh), records.map(x => x.root), key);
        const claimed = records.map((x, j) => (j === 1 ? { before: x.before, root: bump(x.root, p) } : x));
        assert.deepStrictEqual(cls.verifyUpdates(root, updates, fresh, claimed, hash), only(4, 1, 2), key);
        const witness = records.map((x, j) => (j === 2 ? { before: x.before.map((v, l) => (l === 3 ? bump(v, p) : v)), root: x.root } : x));
        assert.deepStrictEqual(cls.verifyUpdates(root, updates, fresh, witness, hash), only(4, 2), key);
        // refusals, and empty input
        assert.deepStrictEqual(cls.pathRoots(hash, [], []), []);
        assert.deepStrictEqual(cls.verifyMany(root, [], [], hash), []);
        assert.deepStrictEqual(cls.verifyUpdates(root, [], [], [], hash), []);
        assert.throws(() => cls.pathRoots(hash, [0], paths), /1 indexes and 5 paths/);
        assert.throws(() => cls.pathRoots(hash, indexes, [paths[0], ...paths.slice(1).map(q => q.slice(0, 3))]), /unequal lengths/);
        assert.throws(() => cls.pathRoots(hash, [0, 16], paths.slice(0, 2)), /index 16 is outside of the 16 leaves/);
        assert.throws(() => cls.pathRoots(hash, [0], [paths[0].slice(0, 1)]), /a leaf and at least one sibling/);
        assert.throws(() => cls.pathRoots(hash, indexes, paths, other.slice(1)), /5 paths and 4 leaves/);
        assert.throws(() => cls.pathRoots({}, indexes, paths), /must come from/);
    }
}
console.log(`js tree_verify (${mode}) OK`);
