'use strict';
// tests/js_multi_field.js <tier> <runtimePrimeSeed> <out.json> [statement] — several prime fields in ONE node process: MiMC-128, the
// ledger module (tests/golden/aa/ledger.aa) over the 128-bit field, and an x^3 + k AirAssembly chain over 2^64 - 21*2^30 + 1,
// 2^32 - 3*2^25 + 1, 2^224 - 2^96 + 1 and a runtime-modulus prime k*2^32 + 1 (k from the seed).  Without [statement]: every statement,
// interleaved (A B C D E F A B ...), member by member (trace, constraints, extension, Merkle commitment: each stage over all fields before
// the next) and through the one-call entries (js/prover.js), every proof verified by the native verifier; then the refusals (a vector of
// one field in another's member, a second runtime modulus, a composite one, a context handed to another field's library).  With
// [statement]: that statement alone, in a process that uses its field only.  Writes { statement: { proofHex, members } }; the caller
// (tests/test_multi_field.py) compares the two.  tier: 'small' (CPU oracle) or 'anchored' (the sizes of tests/golden/config_digests.json).
const fs = require('fs');
const path = require('path');
const crypto = require('crypto');
const assert = require('assert');
const ROOT = path.resolve(__dirname, '..');
const galois = require(path.join(ROOT, 'js', 'galois.js'));
const { createHash, MerkleTree } = require(path.join(ROOT, 'js', 'merkle.js'));
const { MimcAir } = require(path.join(ROOT, 'js', 'air_mimc.js'));
const { compile, AssemblyAir } = require(path.join(ROOT, 'js', 'air_assembly.js'));
const { defaultField } = require(path.join(ROOT, 'js', 'context.js'));
const prover = require(path.join(ROOT, 'js', 'prover.js'));

const [tier, rtSeed, outPath, only] = process.argv.slice(2);
const anchored = tier === 'anchored';
const sha = b => crypto.createHash('sha256').update(b).digest('hex');

const P128 = 2n ** 128n - 9n * 2n ** 32n + 1n, Q64 = 2n ** 64n - 21n * 2n ** 30n + 1n, Q32 = 2n ** 32n - 3n * 2n ** 25n + 1n, P224 = 2n ** 224n - 2n ** 96n + 1n;
// the runtime-modulus field: the first prime k * 2^32 + 1 from a k the seed picks (no fixed build knows it)
function ntPrime(seed) {
    let k = BigInt('0x' + sha(Buffer.from(`runtime prime ${seed}`)).slice(0, 15)) | 1n;
    for (;; k += 2n) { const q = (k << 32n) + 1n; if (!galois.LIBRARIES.has(q) && galois.isProbablePrime(q)) return q; }
}
const QRT = ntPrime(rtSeed);

// x <- x^3 + k, k cycling 1 2 3 4: one register, one constraint of degree 3
const KEYS = [1n, 2n, 3n, 4n];
const chainSource = (p, steps) => `
(module
    (field prime ${p})
    (const $three scalar 3)
    (function $step
        (result vector 1)
        (param $x vector 1) (param $key scalar)
        (add (exp (load.param $x) (load.const $three)) (load.param $key)))
    (export chain
        (registers 1) (constraints 1) (steps ${steps})
        (static (cycle 1 2 3 4))
        (init (param $start vector 1) (load.param $start))
        (transition (call $step (load.trace 0) (get (load.static 0) 0)))
        (evaluation (sub (load.trace 1) (call $step (load.trace 0) (get (load.static 0) 0))))))`;

function ledgerLast(f, balances, factors, deposits) {       // the ledger's register 2 at its last step (tests/test_airassembly.py: ledger_model)
    const p = f.modulus, third = f.inv(3n);
    let step = -1, r;
    for (let i = 0; i < balances.length; i++) {
        r = [balances[i] % p, factors[i] % p, 0n];
        const deps = deposits[i];
        for (let t = 0; t < 2 * deps.length; t++) {
            step++;
            if (t === 2 * deps.length - 1 && i === balances.length - 1) return r[2];
            const dep = deps[Math.min((t + 1) >> 1, deps.length - 1)];
            const n0 = (r[0] + dep * BigInt([1, 2, 3, 4][step % 4])) % p;
            const n1 = (r[1] * factors[i] + (1n << BigInt(step % 8))) % p;
            const s = (n0 + 2n * n1) % p;
            r = [n0, n1, s * s % p * third % p];
        }
    }
    return r[2];
}

// the statements: build() -> { air, field, options, assertions, prove(), verify(proof), context() }
const STATEMENTS = {
    mimc128() {
        const steps = anchored ? 1 << 13 : 256, f = defaultField(P128);
        const options = { hashAlgorithm: 'blake2s256', extensionFactor: 8, exeQueryCount: 48, friQueryCount: 24 };          // C2_E8 when anchored
        const air = new MimcAir(steps, 8, f);
        let x = 3n;
        for (let i = 0; i < steps - 1; i++) x = (x * x % P128 * x + air.roundConstants[i % air.roundConstants.length]) % P128;
        const assertions = [{ step: 0, register: 0, value: 3n }, { step: steps - 1, register: 0, value: x }];
        return { field: f, anchor: anchored ? 'C2_E8' : null,
                 prove: () => prover.proveMimcSerialized(air, options, assertions, 3n),
                 verify: proof => prover.verifyMimcSerialized(air, options, assertions, proof),
                 context: () => air.initProvingContext([], [3n]) };
    },
    ledger128() {
        const runs = anchored ? 4096 : 4, f = defaultField(P128);
        const options = { hashAlgorithm: 'sha256', exeQueryCount: 24, friQueryCount: 12 };                              // X_shaped when anchored
        const air = new AssemblyAir(compile(path.join(ROOT, 'tests', 'golden', 'aa', 'ledger.aa')), 'default', options);
        assert.strictEqual(air.field, f);
        const balances = [], factors = [], deposits = [];
        for (let i = 0; i < runs; i++) { balances.push(BigInt(100 + 7 * i)); factors.push(BigInt(3 + i)); deposits.push([0, 1, 2, 3].map(j => BigInt(5 + i + 2 * j))); }
        const inputs = [balances, factors, deposits];
        const assertions = [{ step: 0, register: 0, value: balances[0] }, { step: 8 * runs - 1, register: 2, value: ledgerLast(f, balances, factors, deposits) }];
        return { field: f, anchor: anchored ? 'X_shaped' : null,
                 prove: () => prover.proveAssemblySerialized(air, options, assertions, inputs),
                 verify: proof => prover.verifyAssemblySerialized(air, options, assertions, proof, [deposits]),
                 context: () => air.initProvingContext(inputs) };
    },
};
for (const [name, p] of [['chain64', Q64], ['chain32', Q32], ['chain224', P224], ['chainRuntime', QRT]]) {
    STATEMENTS[name] = () => {
        const steps = anchored ? 1 << 10 : 64, f = defaultField(p);
        const options = { hashAlgorithm: 'sha256', exeQueryCount: 24, friQueryCount: 12 };
        const air = new AssemblyAir(compile(chainSource(p, steps)), 'chain', options);
        assert.strictEqual(air.field, f);
        assert.strictEqual(air.field.modulus, p);
        let x = 5n;
        for (let i = 0; i < steps - 1; i++) x = (x * x % p * x + KEYS[i % 4]) % p;
        const assertions = [{ step: 0, register: 0, value: 5n }, { step: steps - 1, register: 0, value: x }];
        return { field: f, anchor: null,
                 prove: () => prover.proveAssemblySerialized(air, options, assertions, [], [5n]),
                 verify: proof => prover.verifyAssemblySerialized(air, options, assertions, proof, []),
                 context: () => air.initProvingContext([], [5n]) };
    };
}

// member by member: trace, its polynomials, the constraints, the extension, its Merkle tree — each stage over every statement before the next
function members(list) {
    const st = list.map(s => ({ s, log: [] }));
    const stages = [
        x => { x.ctx = x.s.context(); },
        x => { x.trace = x.ctx.generateExecutionTrace(); x.log.push(sha(x.trace.toBuffer())); },
        x => { x.polys = x.s.field.interpolateRoots(x.ctx.executionDomain, x.trace); },
        x => { x.log.push(sha(x.ctx.evaluateTransitionConstraints(x.polys).toBuffer())); },
        x => { x.ev = x.s.field.evalPolysAtRoots(x.polys, x.ctx.evaluationDomain); x.log.push(sha(x.ev.toBuffer())); },
        x => {
            const h = createHash('blake2s256');                 // (no field: the hash follows its vectors')
            const tree = MerkleTree.create(h.mergeVectorRows(x.s.field.matrixRowsToVectors(x.ev)), h);
            const idx = [1, 2, 7, x.ev.colCount - 1];
            assert(MerkleTree.verifyBatch(tree.root, idx, tree.proveBatch(idx), h));
            x.log.push(tree.root.toString('hex'));
        },
    ];
    for (const stage of stages) for (const x of st) stage(x);
    return st.map(x => x.log);
}

const names = only ? [only] : Object.keys(STATEMENTS);
const built = names.map(n => STATEMENTS[n]());
const out = {};
const logs = members(built);
names.forEach((n, i) => { out[n] = { members: logs[i] }; });
for (let round = 0; round < (only ? 1 : 2); round++) {             // A B C D E F A B C D E F: the one-call entries, alternating fields
    names.forEach((n, i) => {
        const proof = built[i].prove();
        assert.strictEqual(built[i].verify(proof), true);
        const hex = proof.toString('hex');
        if (round) assert.strictEqual(hex, out[n].proofHex, `${n}: a second proof of the same statement differs`);
        Object.assign(out[n], { proofHex: hex, proofBytes: proof.length, proofSha256: sha(proof), anchor: built[i].anchor, modulus: String(built[i].field.modulus) });
    });
}

if (!only) {
    const f128 = defaultField(P128), f64 = defaultField(Q64), frt = defaultField(QRT);
    assert.notStrictEqual(f128.lib, f64.lib);
    // a vector of one field handed to another field's member
    const a = f128.newVectorFrom([1n, 2n, 3n, 4n]), b = f64.newVectorFrom([1n, 2n, 3n, 4n]);
    assert.throws(() => f64.addVectorElements(b, a), TypeError);
    assert.throws(() => f128.evalPolyAtRoots(b, f128.getPowerSeries(f128.getRootOfUnity(4), 4)), TypeError);
    assert.throws(() => createHash('sha256', f64).mergeVectorRows([a]), TypeError);
    assert.throws(() => createHash('sha256').mergeVectorRows([a, b]), TypeError);
    assert.deepStrictEqual(f64.addVectorElements(b, b).toValues(), [2n, 4n, 6n, 8n]);
    // a second runtime modulus; a composite one; an order that does not divide p - 1
    assert.throws(() => galois.createPrimeField(ntPrime(`${rtSeed} other`)), new RegExp(`field of ${QRT} elements`));
    assert.throws(() => galois.createPrimeField(1000003n * 1000033n), /not prime/);
    assert.throws(() => f64.getRootOfUnity(3n), /root of unity of order 3/);
    assert.strictEqual(frt.exp(frt.getRootOfUnity(1 << 16), 1n << 16n), 1n);
    // the addon's library objects: a context only ever reaches the library that created it
    const l128 = f128.lib, l64 = f64.lib, c = f128.ctx, ptr = l128.alloc(c, 64);
    assert.throws(() => l64.call('gs_sync', c), /not created by this library/);
    assert.throws(() => l64.call('gs_download', c, Buffer.alloc(16), ptr, 16), /not created by this library/);
    assert.throws(() => l64.alloc(c, 16), /not created by this library/);
    assert.throws(() => l64.merkleProveBatch(c, ptr, ptr, 4, [0]), /not created by this library/);
    assert.throws(() => l64.proveMimcSerialized(c, '/nonexistent', {}), /not created by this library/);
    assert.throws(() => l64.ctxDestroy(c), /not created by this library/);
    l128.call('gs_free', c, ptr);
    const spare = l64.ctxCreate(0);
    l64.ctxDestroy(spare);
    assert.throws(() => l64.call('gs_sync', spare), /not created by this library/);         // (a destroyed context is nobody's)
    assert.strictEqual(l64.elementSize, f64.elementSize);
    assert.strictEqual(galois.fromLe(frt.lib.modulus, 0, frt.lib.elementSize), QRT);
    out._checks = 'ok';
}
fs.writeFileSync(outPath, JSON.stringify(out));
console.log(`js multi-field OK: ${names.join(' ')}${only ? '' : ' (interleaved)'}`);
