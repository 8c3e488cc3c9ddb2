'use strict';
// tests/js_diagnose.js <cases.json> <out.json> — js/prover.js: diagnoseGenericSerialized on AIRs given as descriptors and
// diagnoseAssemblySerialized on an air-assembly component with input registers (-> napi diagnoseGenericSerialized ->
// gs_prover_diagnose_on).  Writes { name: { ok, assertions, constraints } } with BigInt values as decimal
// strings; tests/test_diagnose.py compares them with the Python host's reports (which it has checked against its host-integer model).
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const ROOT = path.resolve(__dirname, '..');
const { instantiate } = require(path.join(ROOT, 'js', 'shims', '@guildofweavers', 'air-assembly'));
const { compile, AssemblyAir } = require(path.join(ROOT, 'js', 'air_assembly.js'));
const { diagnoseGenericSerialized, diagnoseAssemblySerialized } = require(path.join(ROOT, 'js', 'prover.js'));
const big = v => Array.isArray(v) ? v.map(big) : BigInt(v);
const plain = v => Array.isArray(v) ? v.map(plain) : (typeof v === 'bigint' ? v.toString() : (v && typeof v === 'object' ? Object.fromEntries(Object.entries(v).map(([k, x]) => [k, plain(x)])) : v));

const out = {};
for (const c of JSON.parse(fs.readFileSync(process.argv[2], 'utf8'))) {
    const assertions = c.assertions.map(a => ({ step: a.step, register: a.register, value: BigInt(a.value) }));
    // an air-assembly component with input registers (c.source), or an AIR given as a descriptor (c.generic)
    const d = c.source ? diagnoseAssemblySerialized(new AssemblyAir(compile(c.source), c.component, c.options), assertions, big(c.inputs), undefined)
                       : diagnoseGenericSerialized(instantiate({ generic: c.generic }, 'default', { extensionFactor: c.extension_factor }), assertions, big(c.seed));
    for (const rec of d.constraints) assert.strictEqual(typeof rec.firstValue, 'bigint');
    for (const rec of d.assertions) assert.strictEqual(typeof rec.found, 'bigint');
    out[c.name] = plain(d);
}
fs.writeFileSync(process.argv[3], JSON.stringify(out));
console.log(`js diagnose OK: ${Object.keys(out).length} statements`);
