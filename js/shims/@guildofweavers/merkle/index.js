'use strict';
// replacement for `@guildofweavers/merkle` (INTEGRATION.md section 2)
const m = require('../../../merkle');
module.exports = {
    MerkleTree: m.MerkleTree,
    // upstream: createHash(algorithm, useWasm) — lib/Stark.ts:50; the flag selected the wasm build.  Here the hash knows no field: it
    // hashes vectors in their own field's library (a process may prove in several fields), bytes in the default field's
    createHash: (algorithm, _useWasm) => m.createHash(algorithm),
};
