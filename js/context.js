'use strict';
// one device context per field and process, shared by the galois / merkle / air-assembly replacements: defaultField(modulus) is the field
// of that modulus (created on first use), defaultField() the first one created (the 128-bit field when there is none yet)
const { createPrimeField, MODULUS } = require('./galois');
const fields = new Map();
let first;
function defaultField(modulus) {
    if (modulus === undefined) { if (first) return first; modulus = MODULUS; }
    const m = BigInt(modulus);
    let f = fields.get(m);
    if (!f) {
        f = createPrimeField(m);
        fields.set(m, f);
        if (!first) first = f;
    }
    return f;
}
module.exports = { defaultField };
