'use strict';
// tools/js_alternating_time.js — from node (one process, on the GPU box): a MiMC 2^13 proof (C2, E = 16) alone, and the same proof
// alternating with 2^13-step x^3 + k chain proofs over the 64- and 224-bit fields (medians, ms; the bytes must not change)
const path = require('path'), crypto = require('crypto');
const ROOT = path.resolve(__dirname, '..');
const { instantiate } = require(path.join(ROOT, 'js', 'shims', '@guildofweavers', 'air-assembly'));
const { proveMimcSerialized, proveAssemblySerialized } = require(path.join(ROOT, 'js', 'prover.js'));
const { compile, AssemblyAir } = require(path.join(ROOT, 'js', 'air_assembly.js'));
const ms = fn => { const t = process.hrtime.bigint(); fn(); return Number(process.hrtime.bigint() - t) / 1e6; };
const med = a => a.slice().sort((x, y) => x - y)[a.length >> 1];
const sha = b => crypto.createHash('sha256').update(b).digest('hex');
const o = { hashAlgorithm: 'blake2s256', extensionFactor: 16, exeQueryCount: 48, friQueryCount: 24 };
const air = instantiate({ mimc: { steps: 1 << 13 } }, 'default', o);
const tr = air.initProvingContext([], [3n]).generateExecutionTrace();
const a = [{ step: 0, register: 0, value: tr.getValue(0, 0) }, { step: (1 << 13) - 1, register: 0, value: tr.getValue(0, (1 << 13) - 1) }];
const A = () => proveMimcSerialized(air, o, a, 3n);
let p; for (let k = 0; k < 5; k++) p = A();
const aloneA = []; for (let k = 0; k < 30; k++) aloneA.push(ms(() => { p = A(); }));
const digestA = sha(p);
const chain = (q, steps) => `(module (field prime ${q}) (const $three scalar 3)
 (function $step (result vector 1) (param $x vector 1) (param $key scalar) (add (exp (load.param $x) (load.const $three)) (load.param $key)))
 (export chain (registers 1) (constraints 1) (steps ${steps}) (static (cycle 1 2 3 4)) (init (param $start vector 1) (load.param $start))
  (transition (call $step (load.trace 0) (get (load.static 0) 0)))
  (evaluation (sub (load.trace 1) (call $step (load.trace 0) (get (load.static 0) 0))))))`;
const others = [[2n ** 64n - 21n * 2n ** 30n + 1n, 'q64'], [2n ** 224n - 2n ** 96n + 1n, 'p224']].map(([q, name]) => {
    const steps = 1 << 13, oo = { hashAlgorithm: 'blake2s256', exeQueryCount: 48, friQueryCount: 24 };
    const ai = new AssemblyAir(compile(chain(q, steps)), 'chain', oo);
    let x = 5n; for (let i = 0; i < steps - 1; i++) x = (x * x % q * x + BigInt(1 + i % 4)) % q;
    const as = [{ step: 0, register: 0, value: 5n }, { step: steps - 1, register: 0, value: x }];
    const run = () => proveAssemblySerialized(ai, oo, as, [], [5n]);
    for (let k = 0; k < 3; k++) run();
    const alone = []; for (let k = 0; k < 15; k++) alone.push(ms(run));
    return { name, run, alone: med(alone), alt: [] };
});
const altA = [];
for (let k = 0; k < 30; k++) {
    altA.push(ms(() => { p = A(); }));
    for (const ob of others) ob.alt.push(ms(ob.run));
}
if (sha(p) !== digestA) throw new Error('alternating changed the bytes');
console.log(JSON.stringify({ C2_E16_alone_ms: med(aloneA), C2_E16_alternating_ms: med(altA), digest: digestA,
    others: others.map(ob => ({ name: ob.name, alone_ms: ob.alone, alternating_ms: med(ob.alt) })) }));
