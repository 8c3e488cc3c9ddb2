'use strict';
// tests/js_verify_device.js <case.json> — js/prover.js: verifyGenericSerialized(..., {device: true}) (gs_prover_verify_device through the
// addon, on the field's context) against the default, host-only call: the committed proof with 5 000 assertions on one register
// (tests/golden/many_assertions_quintic_2p13.proof) is accepted by both, and a statement with one asserted value changed is refused by
// both with the same message.  The case file carries the AIR's descriptor and the statement (tests/test_verify_device.py writes it).
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const ROOT = path.resolve(__dirname, '..');
const { instantiate } = require(path.join(ROOT, 'js', 'shims', '@guildofweavers', 'air-assembly'));
const { verifyGenericSerialized } = require(path.join(ROOT, 'js', 'prover.js'));

const c = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const air = instantiate({ generic: c.generic }, 'default', { extensionFactor: c.options.extensionFactor });
const proof = fs.readFileSync(c.proof);
const assertions = c.assertions.map(a => ({ step: a.step, register: a.register, value: BigInt(a.value) }));
const message = fn => { try { return fn() === true ? 'ok' : 'false'; } catch (e) { return 'error: ' + e.message; } };

assert.strictEqual(air.field.lib.has('gs_eval_polys_at_points'), true);
assert.strictEqual(verifyGenericSerialized(air, c.options, assertions, proof), true);
assert.strictEqual(verifyGenericSerialized(air, c.options, assertions, proof, { device: true }), true);
assert.strictEqual(verifyGenericSerialized(air, c.options, assertions, proof, { device: false }), true);
const wrong = assertions.map((a, i) => i === 1234 ? { step: a.step, register: a.register, value: a.value + 1n } : a);
const host = message(() => verifyGenericSerialized(air, c.options, wrong, proof));
const device = message(() => verifyGenericSerialized(air, c.options, wrong, proof, { device: true }));
assert.ok(/linear combination correctness/.test(host), host);
assert.strictEqual(device, host);
const cut = proof.subarray(0, proof.length - 100);
assert.strictEqual(message(() => verifyGenericSerialized(air, c.options, assertions, cut, { device: true })), message(() => verifyGenericSerialized(air, c.options, assertions, cut)));
console.log('js verify device OK');
