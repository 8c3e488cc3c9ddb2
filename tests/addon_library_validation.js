'use strict';
// tests/addon_library_validation.js — the addon's library objects (napi/gstark_napi.cc: open(path)): two field flavours open at once, and
// every member handed something it must refuse — a context of the other library, a destroyed context, a non-context, a bad driver path —
// comes back as a thrown Error, never as a crash or as a call into the wrong library.  tests/test_multi_field.py runs this with the plain
// addon and under the ASAN + UBSAN build (GSTARK_ADDON), against the oracle's libraries (GSTARK_LIB_DIR).
const assert = require('assert');
const path = require('path');
const a = require(process.env.GSTARK_ADDON);
const DIR = process.env.GSTARK_LIB_DIR, DRIVER = process.env.GSTARK_PROVER_LIB;
let n = 0;
function refuses(fn, pattern) { assert.throws(fn, pattern || /./); n++; }

refuses(() => a.open(), /open\(path\)/);
refuses(() => a.open(123), /open\(path\)/);
refuses(() => a.open('/nonexistent/libgstark_hip.so'), /no CPU fallback/);
refuses(() => a.open(DRIVER), /not a gstark library/);

const A = a.open(path.join(DIR, 'liboracle.so')), B = a.open(path.join(DIR, 'liboracle_q64.so'));
assert.strictEqual(typeof A.backend, 'string');
assert(A.elementSize > 0 && B.elementSize > 0 && Buffer.isBuffer(A.modulus) && !A.modulus.equals(B.modulus));
const ca = A.ctxCreate(0), cb = B.ctxCreate(0);
const pa = A.alloc(ca, 4096), pb = B.alloc(cb, 4096);
const foreign = /not created by this library/;

// a context of the other library, through every member that takes one
refuses(() => B.call('gs_sync', ca), foreign);
refuses(() => A.call('gs_upload', cb, pa, Buffer.alloc(A.elementSize), A.elementSize), foreign);
refuses(() => B.call('gs_vec_add', ca, pb, pb, 4, pb), foreign);
refuses(() => B.alloc(ca, 16), foreign);
refuses(() => B.ctxDestroy(ca), foreign);
refuses(() => B.merkleProveBatch(ca, pb, pb, 4, [0]), foreign);
refuses(() => B.proveMimcSerialized(ca, DRIVER, {}), foreign);
refuses(() => B.proveGenericSerialized(ca, DRIVER, {}, Buffer.alloc(8)), foreign);
// not contexts at all, wrong arity, bad driver paths
refuses(() => A.call('gs_sync', {}), /expected a context/);
refuses(() => A.call('gs_sync', 5), /expected a context/);
refuses(() => A.call('gs_sync'), /wrong number of arguments/);
refuses(() => A.call('gs_nope', ca), /unknown gstark function/);
refuses(() => A.alloc(ca, 'x'), /alloc\(ctx, bytes\)/);
refuses(() => A.ctxDestroy(17), /ctxDestroy\(ctx\)/);
refuses(() => A.proveMimcSerialized(ca), /job/);
refuses(() => A.proveMimcSerialized(ca, 7, {}), /driver library path/);
refuses(() => A.proveMimcSerialized(ca, '/nonexistent/libgstark_prover.so', {}), /cannot load/);
refuses(() => A.proveMimcSerialized(ca, path.join(DIR, 'liboracle.so'), {}), /gs_prover_open failed/);
refuses(() => A.proveMimcSerialized(ca, DRIVER, { steps: 'x' }), /malformed job/);
// each library's own context works; a destroyed one is refused by both
A.call('gs_upload', ca, pa, Buffer.alloc(A.elementSize), A.elementSize);
B.call('gs_sync', cb);
B.call('gs_free', cb, pb);
B.ctxDestroy(cb);
refuses(() => B.call('gs_sync', cb), foreign);
refuses(() => B.alloc(cb, 16), foreign);
refuses(() => A.call('gs_sync', cb), foreign);
// the module-level surface is the last load()'s library, next to the objects
assert.strictEqual(typeof a.load(path.join(DIR, 'liboracle_q64.so')), 'string');
refuses(() => a.call('gs_sync', ca), foreign);
A.call('gs_free', ca, pa);
A.ctxDestroy(ca);
console.log(`addon library validation OK: ${n} malformed calls refused`);
