// prover.cc — the whole of Stark.prove() (lib/Stark.ts:81-163) as NATIVE host code above the C ABI.
//
// The Python package mirrors lib/Stark.ts and lib/components/*.ts call by call (genstark_amd/_mirror/stark.py, _mirror/components/); that
// mirror is the readable reference for the sequence below and stays the thing the parity tests compare against.  This file
// is the same sequence — context set-up, trace, P(x), low-degree extension, evaluation tree, CompositionPolynomial
// (CompositionPolynomial.ts:29-146, BoundaryConstraints.ts:15-95, ZeroPolynomial.ts:36-44), LinearCombination (:36-64),
// LowDegreeProver (:39-68, :176-252), QueryIndexGenerator, the spot checks and Serializer.serializeProof (:35-79) — without an
// interpreter between two launches: ~250 ABI calls per proof issue back to back, the few host-side steps (Fiat-Shamir
// hashing of roots, Lagrange interpolation of <= 256 points, the authentication-path plans) run on native limbs.
//
// It is written against include/gstark.h ONLY (plain C++, no HIP): gs_prover_bind() resolves the entry points from whatever
// implementation of the ABI the caller loaded, so the product binds libgstark_hip.so and the CPU tests bind the oracle's
// implementation, exactly like the Python mirror.  Output: the serialized proof (the bytes Serializer.serializeProof gives).
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <map>
#include <chrono>
#include <deque>
#include <string>
#include <vector>

#include "../../include/gstark.h"
#include "../../include/gstark_prover.h"
#include "../../include/gstark_comm.h"
#include "../../include/gstark_boundary.h"
#include "../../include/gstark_mimc.h"
#include "../../include/gstark_diagnose.h"
// One build of this file per field flavour of the ABI library (csrc/build.sh: the same -DGS_SMALL_Q / -DGS_WIDE_BITS): the host-side
// scalars (domain roots, Fiat-Shamir coefficients, boundary interpolants, the remainder check) use the flavour's host arithmetic,
// elements are gs_element_size() bytes on the ABI and in the proof.
#if defined(GS_WIDE_BITS)
#include "gf_wide.h"
#endif
#include "host_field.h"
#include "air_program.h"      // opcodes and validator of AIR programs (verifier.h)
#include "host_poly.h"
#include "host_hash.h"

namespace {

// ---- the slice of the ABI this driver uses, resolved at bind time ------------------------------------------------------
#define GS_API_LIST(X)                                                                                                        \
    X(gs_alloc) X(gs_free) X(gs_upload) X(gs_download) X(gs_gather) X(gs_last_error) X(gs_power_series) X(gs_vec_add) X(gs_vec_mul) \
    X(gs_vec_sub_scalar) X(gs_vec_div) X(gs_combine_many) X(gs_combine_adjusted) X(gs_pluck) X(gs_transpose_vector) X(gs_sub_matrix_from_vectors)     \
    X(gs_eval_polys_at_roots) X(gs_interpolate_roots) X(gs_interpolate_quartic_domain) X(gs_eval_quartic_batch)                \
    X(gs_hash_merge_rows) X(gs_hash_digest_values) X(gs_merkle_build) X(gs_merkle_commit_rows) X(gs_merkle_prove_batch) X(gs_small_interpolate)          \
    X(gs_small_eval_poly) X(gs_pseudorandom_indexes) X(gs_mimc_trace) X(gs_mimc_constraints) X(gs_air_trace)                    \
    X(gs_air_trace_segments) X(gs_air_constraints) X(gs_air_constraints_strided) X(gs_composition_tail) X(gs_composition_tail_coset) X(gs_zero_poly_inverses) X(gs_div_by_domain_roots) X(gs_mimc_composition) X(gs_fri_fold) X(gs_fri_fold_seeded) X(gs_defer_begin) X(gs_defer_end) X(gs_readback_post) X(gs_readback_wait) X(gs_merkle_commit_rows_seed) X(gs_fri_fold_at) \
    X(gs_vec_mul_scalar) X(gs_copy) X(gs_gather_words) X(gs_transpose_records) X(gs_fri_fold_seeded_scaled) X(gs_fri_layers) X(gs_sync) X(gs_zero_poly_inverses_coset) X(gs_div_by_domain_roots_coset)
// ... and the entry points an implementation may lack (include/gstark_boundary.h, gstark_diagnose.h): null then, and the driver keeps its host path
// (include/gstark_mimc.h: without them the fused MiMC branch calls gs_mimc_composition)
#define GS_API_OPTIONAL_LIST(X) X(gs_boundary_polys) X(gs_eval_polys_at_points) X(gs_mimc_composition_prepare) X(gs_mimc_composition_tables) X(gs_nonzero_spans)
struct Api {
#define X(name) decltype(&::name) name = nullptr;
    GS_API_LIST(X)
    GS_API_OPTIONAL_LIST(X)
#undef X
};
// The driver is written against `A.gs_xxx(...)`: A is the binding of the CURRENT call on this thread — the process-wide default
// (gs_prover_bind) unless the entry point was handed a binding of its own (gs_prover_open, the `_on` entry points).
Api g_default_api;
bool g_bound = false;
thread_local const Api *g_api = &g_default_api;
#define A (*g_api)
struct UseApi {          // scope of one entry point
    const Api *saved;
    explicit UseApi(const Api *a) : saved(g_api) { g_api = a; }
    ~UseApi() { g_api = saved; }
};

struct Fail {
    int code;
    std::string msg;
};
[[noreturn]] void fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Fail{code, buf};
}

typedef hfe F;
const uint64_t ELEM = HF_ELT;                   // 16, or 32 in the 256- / 224-bit fields
const uint64_t DIGEST = 32, MAX_ARRAY = 256;
const uint64_t WORD = 16, EW = ELEM / WORD;     // gs_gather_words / gs_defer_* move 16-byte words
static_assert(ELEM <= GS_PROVER_ELT_MAX, "element wider than the job's scalar fields");
typedef std::vector<uint8_t> Bytes;

struct Ctx {
    gs_ctx *c;
    void check(int rc, const char *what) {
        if (rc) fail(rc, "%s: %s", what, c ? A.gs_last_error(c) : "error");
    }
};

// device block owned for the duration of a proof (gs_free parks it in the context's cache: no synchronisation)
struct Buf {
    Ctx *x = nullptr;
    void *p = nullptr;
    Buf() {}
    Buf(Ctx &cx, uint64_t bytes) : x(&cx) { cx.check(A.gs_alloc(cx.c, bytes ? bytes : 16, &p), "gs_alloc"); }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : x(o.x), p(o.p) { o.p = nullptr; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) { release(); x = o.x; p = o.p; o.p = nullptr; }
        return *this;
    }
    void release() { if (p) { A.gs_free(x->c, p); p = nullptr; } }
    ~Buf() { release(); }
    uint8_t *at(uint64_t byte_offset) const { return (uint8_t *)p + byte_offset; }
};

// a field element on the ABI and in the proof: ELEM bytes, little-endian
void store_elem(F v, uint8_t *out) { hf_store(out, v); }
F load_elem(const uint8_t *b) { return hf_load(b); }
// ... and as a value, for the scalar arguments of the entry points: enc(v) is built in the argument list and lives until the call returns
struct Enc {
    uint8_t b[ELEM];
    operator const uint8_t *() const { return b; }
};
Enc enc(F v) { Enc e; hf_store(e.b, v); return e; }

// ---- galois prng (genstark_amd/field.py: prng — restated) and the index generator -----------------
std::vector<F> prng_many(const Bytes &seed, size_t count) {
    std::vector<F> out(count);
    uint8_t st[32], msg[32];
    host_sha256(seed.data(), seed.size(), st);
    for (size_t i = 0; i < count; i++) {
        out[i] = hf_from_digest(st);
        int n = host_bigint_bytes(st, 32, msg);
        host_sha256(msg, (size_t)n, st);
    }
    return out;
}
F prng_one(const Bytes &seed) {
    uint8_t st[32];
    host_sha256(seed.data(), seed.size(), st);
    return hf_from_digest(st);
}
std::vector<uint64_t> query_indexes(const Bytes &seed, uint32_t count, uint64_t max, uint32_t exclude) {
    uint64_t max_count = exclude ? max - max / exclude : max;
    if (max_count < count) fail(GS_ERR_ARG, "Cannot select %u unique pseudorandom indexes from %llu values", count, (unsigned long long)max);
    std::vector<uint64_t> out(count ? count : 1);
    if (A.gs_pseudorandom_indexes(seed.data(), (uint32_t)seed.size(), count, max, exclude, out.data()))
        fail(GS_ERR_ARG, "Could not generate %u pseudorandom indexes", count);
    out.resize(count);
    return out;
}

// ---- Merkle batch proofs and the wire format (lib/Serializer.ts:35-79, lib/utils/serialization.ts) ------------------
struct MerkleProof {          // flat: one allocation per part instead of one per digest (a proof holds ~10^4 of them)
    Bytes values;              // nvalues records of value_size bytes (the queried rows)
    uint64_t value_size = 0;
    uint32_t nvalues = 0;
    Bytes nodes;               // digests, column after column
    std::vector<uint32_t> lens;
    uint8_t depth = 0;
};
void write_merkle_proof(Bytes &out, const MerkleProof &p, uint64_t leaf_size) {
    // values: lib/utils/serialization.ts writeArray
    if (!p.nvalues) fail(GS_ERR_ARG, "Array cannot be zero-length");
    if (p.nvalues > MAX_ARRAY) fail(GS_ERR_ARG, "Array length (%u) cannot exceed 256", p.nvalues);
    out.push_back(p.nvalues == MAX_ARRAY ? 0 : (uint8_t)p.nvalues);
    out.insert(out.end(), p.values.begin(), p.values.begin() + (uint64_t)p.nvalues * p.value_size);
    // nodes: writeMatrix
    if (p.lens.size() > MAX_ARRAY) fail(GS_ERR_ARG, "Matrix column count (%zu) cannot exceed 256", p.lens.size());
    out.push_back(p.lens.size() == MAX_ARRAY ? 0 : (uint8_t)p.lens.size());
    uint64_t total = 0;
    for (uint32_t len : p.lens) {
        if (len >= 128) fail(GS_ERR_ARG, "Matrix column length (%u) cannot exceed 127", len);
        const uint8_t type = (len && DIGEST == leaf_size) ? 1 : 0;
        out.push_back((uint8_t)((len << 1) | type));
        total += len;
    }
    out.insert(out.end(), p.nodes.begin(), p.nodes.begin() + total * DIGEST);
    out.push_back(p.depth);
}

struct Tree {
    Buf leaves, nodes;   // digests; nodes in heap order
    uint64_t n = 0;
    Bytes root;
    Buf point;           // FRI trees: prng(root), derived by the launch that produced the root (gs_merkle_commit_rows_seed)
    uint64_t ticket = 0; // ... which also posted the root to the host
};
// Hash.mergeVectorRows(vectors) + MerkleTree.create (lib/Stark.ts:115-118; LowDegreeProver.ts:45-46, 201-202) as one ABI call.
// read_root = false leaves the root on the device (nodes + DIGEST): the FRI layers derive their evaluation points from it there
// (gs_fri_fold_seeded) and all roots come back in one round trip
Tree commit_rows(Ctx &x, int alg, const void *const *vecs, uint32_t count, uint64_t n, bool read_root = true) {
    Tree t;
    t.n = n;
    t.leaves = Buf(x, n * DIGEST);
    t.nodes = Buf(x, n * DIGEST);
    x.check(A.gs_merkle_commit_rows(x.c, (gs_hash_alg)alg, vecs, count, n, t.leaves.p, t.nodes.p), "gs_merkle_commit_rows");
    t.root.resize(DIGEST);
    if (read_root) x.check(A.gs_download(x.c, t.root.data(), t.nodes.at(DIGEST), DIGEST), "gs_download(root)");
    return t;
}
// gs_defer_begin ... gs_defer_end as a scope: when a call inside the window throws, the window is still closed (the context would
// otherwise stay in deferral mode and the next prove() on it would fail with "already deferring")
struct DeferWindow {
    Ctx &x;
    bool open = false;
    explicit DeferWindow(Ctx &cx) : x(cx) { x.check(A.gs_defer_begin(x.c), "gs_defer_begin"); open = true; }
    void end() { open = false; x.check(A.gs_defer_end(x.c), "gs_defer_end"); }
    ~DeferWindow() { if (open) A.gs_defer_end(x.c); }
};
// The query answers of a proof are issued inside one deferral window (gs_defer_begin / gs_defer_end): the calls below queue the
// device work into buffers that stay put (std::deque) and `unpack` builds the proof objects after the single synchronisation.
struct Readbacks {
    struct Batch { MerkleProof *mp; Bytes digests; uint32_t ncols = 0; };
    struct Rows { MerkleProof *mp; Bytes raw; uint64_t rec = 0; uint32_t n = 0; };
    std::deque<Batch> batches;
    std::deque<Rows> rows;
    void prove_batch(Ctx &x, const Tree &t, const std::vector<uint64_t> &idx, MerkleProof *mp) {
        int depth = 0;
        while ((1ull << depth) < t.n) depth++;
        mp->depth = (uint8_t)depth;
        const uint32_t count = (uint32_t)idx.size();
        if (!count) return;
        batches.emplace_back();
        Batch &b = batches.back();
        b.mp = mp;
        const uint64_t cap = (uint64_t)count * (depth ? depth : 1);
        b.digests.resize(count * DIGEST);         // the leaf digests: the proof carries the rows themselves instead (gather below)
        mp->nodes.resize(cap * DIGEST);
        mp->lens.assign(count, 0);
        x.check(A.gs_merkle_prove_batch(x.c, t.leaves.p, t.nodes.p, t.n, idx.data(), count, b.digests.data(), &b.ncols, mp->lens.data(), mp->nodes.data(), cap),
                "gs_merkle_prove_batch");
        mp->lens.resize(b.ncols);                 // the shape is known at once; the digests arrive with gs_defer_end
    }
    void gather(Ctx &x, const void *src, uint64_t rec, const std::vector<uint64_t> &idx, uint64_t per_row, MerkleProof *mp) {
        if (idx.empty()) return;
        mp->values.resize(idx.size() * rec);
        mp->value_size = rec * per_row;
        mp->nvalues = (uint32_t)(idx.size() / per_row);
        x.check(A.gs_gather(x.c, src, rec, idx.data(), idx.size(), mp->values.data()), "gs_gather");
    }
    // rows of transposeVector(column, 4), read strided (see gather_rows4)
    void gather_rows4(Ctx &x, const void *column, uint64_t nrows, const std::vector<uint64_t> &positions, MerkleProof *mp) {
        std::vector<uint64_t> idx;
        idx.reserve(positions.size() * 4);
        for (uint64_t r : positions)
            for (uint64_t c = 0; c < 4; c++) idx.push_back(r + c * nrows);
        gather(x, column, ELEM, idx, 4, mp);
    }
};

MerkleProof prove_batch(Ctx &x, const Tree &t, const std::vector<uint64_t> &idx) {
    MerkleProof mp;
    Readbacks rb;
    rb.prove_batch(x, t, idx, &mp);               // outside a deferral window the call returns with the digests in place
    return mp;
}
// rows of transposeVector(column, 4) without the transposed copy: row r = column[r], column[r + rows], column[r + 2 rows], column[r + 3 rows]
void gather_rows4(Ctx &x, const void *column, uint64_t rows, const std::vector<uint64_t> &positions, MerkleProof *mp) {
    Readbacks rb;
    rb.gather_rows4(x, column, rows, positions, mp);
}
// tree over the rows of transposeVector(column, 4) (Hash.digestValues of the transposed matrix + MerkleTree.create, LowDegreeProver.ts:45-46,
// 201-202): the row digests are mergeVectorRows of the four quarters of the column (the same 64-byte messages)
// want_point: a layer will be folded at prng(this tree's root); the root is posted to the host either way (t.ticket)
Tree commit_rows4(Ctx &x, int alg, const void *column, uint64_t rows, bool want_point) {
    const void *quarters[4];
    for (uint64_t c = 0; c < 4; c++) quarters[c] = (const uint8_t *)column + c * rows * ELEM;
    Tree t;
    t.n = rows;
    t.leaves = Buf(x, rows * DIGEST);
    t.nodes = Buf(x, rows * DIGEST);
    if (want_point) t.point = Buf(x, ELEM);
    x.check(A.gs_merkle_commit_rows_seed(x.c, (gs_hash_alg)alg, quarters, 4, rows, t.leaves.p, t.nodes.p, want_point ? t.point.p : nullptr, &t.ticket),
            "gs_merkle_commit_rows_seed");
    t.root.resize(DIGEST);
    return t;
}
// ---- input registers of an air-assembly component: where every value of every input register sits in the trace, from the registers'
// declarations and the SHAPES of their values alone (genstark_amd/airassembly.py: _Layout, restated).  prove() checks the shapes it
// serializes with this; verify() sizes the trace from the shapes a proof carries (initVerificationContext(proof.iShapes, ...),
// lib/Stark.ts:176).  Messages as the Python loader words them.
typedef std::vector<std::vector<uint32_t>> Shapes;
struct InputLayout {
    std::vector<uint32_t> depth;
    std::vector<uint64_t> span, count;      // steps one value is held; values of the register
    uint64_t length = 0;                    // trace steps the inputs lay out
};
const uint64_t MAX_LAYOUT = 1ull << 40;     // products are capped here: nothing this driver proves or verifies is longer
uint64_t capped_mul(uint64_t a, uint64_t b) {
    if (a && b > MAX_LAYOUT / a) return MAX_LAYOUT;
    return std::min(a * b, MAX_LAYOUT);
}
InputLayout input_layout(const gs_prover_air &air, const Shapes &shapes) {
    const uint32_t n = air.ninputs;
    const gs_input_register *in = air.inputs;
    if (shapes.size() != n) fail(GS_ERR_ARG, "%u input registers: one entry (shape) for each is needed, got %zu", n, shapes.size());
    InputLayout L;
    L.depth.resize(n); L.span.assign(n, 0); L.count.resize(n);
    for (uint32_t j = 0; j < n; j++) {
        const int32_t ref = in[j].parent >= 0 ? in[j].parent : in[j].peer;
        if ((in[j].parent >= 0 || in[j].peer >= 0) && !(ref >= 0 && (uint32_t)ref < j))
            fail(GS_ERR_ARG, "input register: childof / peerof must name an earlier input register");
        if (in[j].parent >= 0 && in[j].peer >= 0 && (uint32_t)in[j].peer >= j) fail(GS_ERR_ARG, "input register: childof / peerof must name an earlier input register");
        L.depth[j] = (in[j].parent < 0 && in[j].peer < 0) ? 0 : L.depth[ref] + (in[j].parent >= 0 ? 1 : 0);
        if (shapes[j].size() != (size_t)L.depth[j] + 1) fail(GS_ERR_ARG, "input register %u: values nested %u deep expected", j, L.depth[j] + 1);
        if (in[j].peer >= 0 && shapes[j] != shapes[in[j].peer]) fail(GS_ERR_ARG, "input register %u: the shape of its peer %d expected", j, in[j].peer);
        if (in[j].parent >= 0 && !std::equal(shapes[j].begin(), shapes[j].end() - 1, shapes[in[j].parent].begin(), shapes[in[j].parent].end()))
            fail(GS_ERR_ARG, "input register %u: one list per value of register %d expected", j, in[j].parent);
    }
    // steps one value of a register is held: its own (steps n), or what its children take (`known`: a span of 0 steps — a child list of
    // zero values — is a value like any other here, as in the loader; the length rule below refuses it)
    std::vector<char> known(n, 0);
    for (uint32_t j = 0; j < n; j++) if (in[j].steps) { L.span[j] = in[j].steps; known[j] = 1; }
    for (bool changed = true; changed;) {
        changed = false;
        for (uint32_t j = 0; j < n; j++) {
            if (known[j] && in[j].parent >= 0) {
                const uint64_t want = capped_mul(L.span[j], shapes[j].back());
                const uint32_t root = (uint32_t)in[j].parent;
                if (!known[root]) { L.span[root] = want; known[root] = 1; changed = true; }
                else if (L.span[root] != want && !in[root].steps) fail(GS_ERR_ARG, "input registers: the children of one register take different numbers of steps");
            }
            if (!known[j] && in[j].peer >= 0 && known[in[j].peer]) { L.span[j] = L.span[in[j].peer]; known[j] = 1; changed = true; }
            if (known[j] && in[j].peer >= 0 && !known[in[j].peer]) { L.span[in[j].peer] = L.span[j]; known[in[j].peer] = 1; changed = true; }
        }
    }
    for (uint32_t j = 0; j < n; j++)
        if (!known[j]) fail(GS_ERR_ARG, "input registers: cannot tell how many steps a value is held (no (steps n) below it)");
    for (uint32_t j = 0; j < n; j++) {
        uint64_t count = 1;
        for (uint32_t d : shapes[j]) count = capped_mul(count, d);
        L.count[j] = count;
        const uint64_t len = capped_mul(count, L.span[j]);
        if (L.length && len != L.length) fail(GS_ERR_ARG, "input registers imply different trace lengths");
        L.length = len;
    }
    for (uint32_t j = 0; j < n; j++)            // (a register of no values, or of values held for 0 steps, that came first was skipped above)
        if (capped_mul(L.count[j], L.span[j]) != L.length) fail(GS_ERR_ARG, "input registers imply different trace lengths");
    if (n && (L.length < 2 || (L.length & (L.length - 1)) || L.length >= MAX_LAYOUT))
        fail(GS_ERR_ARG, "the inputs make a trace of %llu steps: a power of 2 is required", (unsigned long long)L.length);
    return L;
}
// iShapes as the job carries them (per register: rank, then the dimensions) -> Shapes
Shapes job_shapes(const gs_prover_air &air) {
    Shapes out(air.ninputs);
    if (air.ninputs && !air.input_shapes) fail(GS_ERR_ARG, "an AIR with input registers needs the shapes of its inputs");
    const uint32_t *q = air.input_shapes;
    for (uint32_t j = 0; j < air.ninputs; j++) {
        const uint32_t rank = *q++;
        if (rank > 255) fail(GS_ERR_ARG, "input register %u: values nested %u deep", j, rank);
        out[j].assign(q, q + rank);
        q += rank;
    }
    return out;
}
// Serializer.serializeProof's last part (lib/Serializer.ts:70-78): count, then per shape its rank and the dimensions as uint32 LE
void write_input_shapes(Bytes &out, const Shapes &shapes) {
    if (shapes.size() > 255) fail(GS_ERR_ARG, "too many input registers");
    out.push_back((uint8_t)shapes.size());
    for (const auto &sh : shapes) {
        out.push_back((uint8_t)sh.size());
        for (uint32_t d : sh) for (int b = 0; b < 4; b++) out.push_back((uint8_t)(d >> (8 * b)));
    }
}
// what prove() does with a job's input registers before any device work: the shapes must lay out exactly the trace the job states
Shapes checked_job_shapes(const gs_prover_job &job) {
    if (!job.air.ninputs) return Shapes();
    if (!job.air.inputs) fail(GS_ERR_ARG, "invalid job: input registers without their declarations");
    Shapes shapes = job_shapes(job.air);
    const InputLayout L = input_layout(job.air, shapes);
    if (L.length != job.steps) fail(GS_ERR_ARG, "the inputs lay out a trace of %llu steps, the job states %llu", (unsigned long long)L.length, (unsigned long long)job.steps);
    return shapes;
}
// the root of unity of the evaluation domain from the job's (root_of_unity_log2: squared down from a root of higher order)
F domain_root(const gs_prover_job &job, uint64_t N) {
    F w = load_elem(job.root_of_unity);
    if (!job.root_of_unity_log2) return w;
    if (job.root_of_unity_log2 > 63 || N > (1ull << job.root_of_unity_log2)) fail(GS_ERR_ARG, "the field has no root of unity of order %llu", (unsigned long long)N);
    for (uint64_t order = 1ull << job.root_of_unity_log2; order > N; order >>= 1) w = hf_mul(w, w);
    return w;
}

std::vector<uint64_t> unique_in_order(const std::vector<uint64_t> &v) {
    std::vector<uint64_t> out;
    std::map<uint64_t, bool> seen;
    for (uint64_t e : v)
        if (!seen.count(e)) { seen[e] = true; out.push_back(e); }
    return out;
}

// the body of a C entry point: a Fail returns its code (and message), any other exception `other` (and its what())
template <class Body>
int guarded(char *err, uint64_t errcap, int other, Body &&body) {
    try {
        return body();
    } catch (const Fail &f) {
        if (err && errcap) snprintf(err, (size_t)errcap, "%s", f.msg.c_str());
        return f.code ? f.code : GS_ERR_ARG;
    } catch (const std::exception &e) {
        if (err && errcap) snprintf(err, (size_t)errcap, "%s", e.what());
        return other;
    }
}
// a prove entry point: the serialized proof into out[0..cap); *len receives the size (also when cap is too small: GS_ERR_ARG then)
template <class Prove>
int prove_guarded(gs_ctx *ctx, uint8_t *out, uint64_t cap, uint64_t *len, char *err, uint64_t errcap, Prove &&prove) {
    return guarded(err, errcap, GS_ERR_OOM, [&]() -> int {
        Ctx x{ctx};
        Bytes proof;
        prove(x, proof);
        *len = proof.size();
        if (proof.size() > cap || !out) return GS_ERR_ARG;
        memcpy(out, proof.data(), proof.size());
        return GS_OK;
    });
}

}  // namespace

// What the last prove() on this thread did: wall-clock of the phases (host clock at the phase boundaries; no device
// synchronisation is added, so a phase lasts until its last BLOCKING call returned) and the transform work it launched.
static thread_local gs_prover_stats g_stats;
static thread_local bool g_sync_phases = false;      // gs_prover_sync_phases
static thread_local bool g_member_sequence = false;  // gs_prover_member_sequence
static thread_local bool g_host_boundary = false;    // gs_prover_host_boundary
// gs_composition_tail[_coset] takes up to four assertions per register, 64 asserted registers, 96 committed vectors
static bool tail_fits(const gs_prover_job &job, uint32_t vectors) {
    if (g_member_sequence || vectors > 96) return false;
    std::vector<std::pair<uint32_t, uint32_t>> per_reg;
    for (uint32_t i = 0; i < job.nassertions; i++) {
        bool found = false;
        for (auto &e : per_reg)
            if (e.first == job.assertions[i].reg) { found = true; if (++e.second > 4) return false; }
        if (!found) per_reg.push_back({job.assertions[i].reg, 1u});
    }
    return per_reg.size() <= 64;
}

// the two transform entry points, counted: rows * n points per call.  The library serves a transform of fewer than 256 points
// or of a polynomial of at most 8 coefficients with a Horner kernel (ntt.hip: ntt_run), which is not an NTT: counted apart.
static int counted_interpolate_roots(gs_ctx *c, const void *ys, uint32_t rows, const uint8_t *omega, uint64_t n, void *out) {
    if (n >= 256) { g_stats.ntt_points += (uint64_t)rows * n; g_stats.ntt_transforms += rows; }
    else g_stats.horner_points += (uint64_t)rows * n;
    return A.gs_interpolate_roots(c, ys, rows, omega, n, out);
}
static int counted_eval_polys_at_roots(gs_ctx *c, const void *polys, uint32_t rows, uint64_t poly_len, const uint8_t *omega, uint64_t n, void *out) {
    if (n >= 256 && poly_len > 8) { g_stats.ntt_points += (uint64_t)rows * n; g_stats.ntt_transforms += rows; }
    else g_stats.horner_points += (uint64_t)rows * n;
    return A.gs_eval_polys_at_roots(c, polys, rows, poly_len, omega, n, out);
}

extern "C" {

static int bind_api(Api &api, void *dl_handle) {
    if (!dl_handle) return GS_ERR_ARG;
#define X(name)                                                 \
    api.name = (decltype(api.name))dlsym(dl_handle, #name);     \
    if (!api.name) return GS_ERR_UNSUPPORTED;
    GS_API_LIST(X)
#undef X
#define X(name) api.name = (decltype(api.name))dlsym(dl_handle, #name);
    GS_API_OPTIONAL_LIST(X)
#undef X
    // the library must compute in the field this build of the driver does its host-side scalars in
    auto esize = (int (*)())dlsym(dl_handle, "gs_element_size");
    auto modulus = (int (*)(uint8_t *))dlsym(dl_handle, "gs_field_modulus");
    if (!esize || !modulus || (uint64_t)esize() != ELEM) return GS_ERR_UNSUPPORTED;
    uint8_t m[GS_PROVER_ELT_MAX] = {0}, want[GS_PROVER_ELT_MAX] = {0};
    if (modulus(m)) return GS_ERR_UNSUPPORTED;
#if defined(GF_RUNTIME_MODULUS)
    // the runtime-modulus build of the driver computes in whatever field the library it is bound to was given (gs_set_modulus) — one per
    // process, like the library's
    { uint32_t pl[GF_LIMBS]; memcpy(pl, m, sizeof pl); if (gf_rt_configure(pl)) return GS_ERR_UNSUPPORTED; }
#endif
    hf_modulus_bytes(want);
    return memcmp(m, want, ELEM) ? GS_ERR_UNSUPPORTED : GS_OK;
}
int gs_prover_bind(void *dl_handle) {
    const int rc = bind_api(g_default_api, dl_handle);
    if (rc == GS_OK) g_bound = true;
    return rc;
}
int gs_prover_open(void *dl_handle, gs_prover_binding **out) {
    if (!out) return GS_ERR_ARG;
    Api *api = new Api();
    const int rc = bind_api(*api, dl_handle);
    if (rc) { delete api; return rc; }
    *out = reinterpret_cast<gs_prover_binding *>(api);
    return GS_OK;
}
void gs_prover_close(gs_prover_binding *b) { delete reinterpret_cast<Api *>(b); }
int gs_prover_element_size(void) { return (int)ELEM; }

static void prove_impl(Ctx &x, const gs_prover_job &job, Bytes &out);
static int prove_entry(gs_ctx *ctx, const struct gs_prover_job *job, uint8_t *out, uint64_t cap, uint64_t *len, char *err, uint64_t errcap);
static bool remainder_is_low_degree(const std::vector<F> &remainder, uint64_t E, uint64_t m, F rou, int method);

// Serialized proof into out[0..cap); *len receives the size (also when cap is too small: GS_ERR_ARG then).
int gs_prover_prove_on(const gs_prover_binding *b, gs_ctx *ctx, const struct gs_prover_job *job, uint8_t *out, uint64_t cap, uint64_t *len, char *err,
                       uint64_t errcap) {
    if (!b) return GS_ERR_ARG;
    UseApi use(reinterpret_cast<const Api *>(b));
    return prove_entry(ctx, job, out, cap, len, err, errcap);
}
int gs_prover_prove(gs_ctx *ctx, const struct gs_prover_job *job, uint8_t *out, uint64_t cap, uint64_t *len, char *err, uint64_t errcap) {
    if (!g_bound) return GS_ERR_UNSUPPORTED;
    UseApi use(&g_default_api);
    return prove_entry(ctx, job, out, cap, len, err, errcap);
}
static int prove_entry(gs_ctx *ctx, const struct gs_prover_job *job, uint8_t *out, uint64_t cap, uint64_t *len, char *err, uint64_t errcap) {
    if (!ctx || !job || !len) return GS_ERR_ARG;
    return prove_guarded(ctx, out, cap, len, err, errcap, [&](Ctx &x, Bytes &proof) { prove_impl(x, *job, proof); });
}

static int remainder_check_entry(const uint8_t *values, uint64_t len, uint32_t extension_factor, uint64_t max_degree_plus1, const uint8_t *root_of_unity, int method);
int gs_prover_remainder_check(const uint8_t *values, uint64_t len, uint32_t extension_factor, uint64_t max_degree_plus1, const uint8_t *root_of_unity,
                              int method) {
    if (!g_bound) return GS_ERR_UNSUPPORTED;
    UseApi use(&g_default_api);
    return remainder_check_entry(values, len, extension_factor, max_degree_plus1, root_of_unity, method);
}
int gs_prover_remainder_check_on(const gs_prover_binding *b, const uint8_t *values, uint64_t len, uint32_t extension_factor, uint64_t max_degree_plus1,
                                 const uint8_t *root_of_unity, int method) {
    if (!b) return GS_ERR_ARG;
    UseApi use(reinterpret_cast<const Api *>(b));
    return remainder_check_entry(values, len, extension_factor, max_degree_plus1, root_of_unity, method);
}
static int remainder_check_entry(const uint8_t *values, uint64_t len, uint32_t extension_factor, uint64_t max_degree_plus1, const uint8_t *root_of_unity, int method) {
    if (!values || !root_of_unity || !len || (method != 0 && method != 1)) return GS_ERR_ARG;
    return guarded(nullptr, 0, GS_ERR_OOM, [&]() -> int {
        std::vector<F> v(len);
        for (uint64_t i = 0; i < len; i++) v[i] = load_elem(values + ELEM * i);
        return remainder_is_low_degree(v, extension_factor, max_degree_plus1, load_elem(root_of_unity), method) ? 1 : 0;
    });
}

void gs_prover_sync_phases(int on) { g_sync_phases = on != 0; }
void gs_prover_member_sequence(int on) { g_member_sequence = on != 0; }
void gs_prover_host_boundary(int on) { g_host_boundary = on != 0; }

int gs_prover_abi_version(void) { return GS_PROVER_ABI_VERSION; }

int gs_prover_input_layout(const struct gs_input_register *inputs, uint32_t ninputs, const uint32_t *shapes, uint64_t *length, char *err, uint64_t errcap) {
    if ((ninputs && (!inputs || !shapes)) || !length) return GS_ERR_ARG;
    return guarded(err, errcap, GS_ERR_OOM, [&]() -> int {
        gs_prover_air air;
        memset(&air, 0, sizeof air);
        air.inputs = inputs; air.ninputs = ninputs; air.input_shapes = shapes;
        *length = input_layout(air, job_shapes(air)).length;
        return GS_OK;
    });
}

int gs_prover_last_stats(struct gs_prover_stats *out) {
    if (!out) return GS_ERR_ARG;
    *out = g_stats;
    return GS_OK;
}

}  // extern "C"

// GSTARK_PROVER_TIMING=1: host wall-clock at the phase boundaries on stderr (no device synchronisation is added, so a phase
// shows the time until its last BLOCKING call returned)
struct PhaseClock {
    bool on = getenv("GSTARK_PROVER_TIMING") != nullptr;      // also echo the marks on stderr
    const bool sync = g_sync_phases;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0, last_readme = t0;
    PhaseClock() { memset(&g_stats, 0, sizeof g_stats); }
    // one of the reference's log points (lib/Stark.ts:92-152; README.md:62-73).  Measuring mode only (gs_prover_sync_phases): the
    // device is drained here, so the entry is this phase's own wall-clock
    void readme(Ctx &x, const char *fmt, ...) {
        if (!sync) return;
        x.check(A.gs_sync(x.c), "gs_sync");
        auto now = std::chrono::steady_clock::now();
        if (g_stats.nreadme < GS_PROVER_MAX_PHASES) {
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(g_stats.readme_label[g_stats.nreadme], sizeof g_stats.readme_label[0], fmt, ap);
            va_end(ap);
            g_stats.readme_ms[g_stats.nreadme++] = std::chrono::duration<double, std::milli>(now - last_readme).count();
        }
        last_readme = now;
    }
    void mark(const char *what) {
        auto now = std::chrono::steady_clock::now();
        const double total = std::chrono::duration<double, std::milli>(now - t0).count();
        const double delta = std::chrono::duration<double, std::milli>(now - last).count();
        if (g_stats.nphases < GS_PROVER_MAX_PHASES) {
            snprintf(g_stats.phase_label[g_stats.nphases], sizeof g_stats.phase_label[0], "%s", what);
            g_stats.phase_ms[g_stats.nphases++] = delta;
        }
        g_stats.total_ms = total;
        if (on) fprintf(stderr, "[prover] %-44s %8.3f ms  (+%.3f)\n", what, total, delta);
        last = now;
    }
    // the interval since the last mark as TWO entries: `first_ms` of it under `a` (time the host spent blocked, measured by the caller),
    // the rest under `b`
    void mark_split(const char *a, double first_ms, const char *b) {
        auto now = std::chrono::steady_clock::now();
        const double delta = std::chrono::duration<double, std::milli>(now - last).count();
        const double total = std::chrono::duration<double, std::milli>(now - t0).count();
        const char *labels[2] = {a, b};
        const double parts[2] = {std::min(first_ms, delta), delta - std::min(first_ms, delta)};
        for (int k = 0; k < 2; k++)
            if (g_stats.nphases < GS_PROVER_MAX_PHASES) {
                snprintf(g_stats.phase_label[g_stats.nphases], sizeof g_stats.phase_label[0], "%s", labels[k]);
                g_stats.phase_ms[g_stats.nphases++] = parts[k];
            }
        g_stats.total_ms = total;
        if (on) fprintf(stderr, "[prover] %-44s %8.3f ms  (+%.3f)\n[prover] %-44s %8.3f ms  (+%.3f)\n", a, total - parts[1], parts[0], b, total, parts[1]);
        last = now;
    }
};

// LowDegreeProver.verifyRemainder (:223-252): the remainder — `len` values on the powers of `rou` (order len) — must agree, at
// every position i that is not a multiple of E, with the polynomial of degree < m through the first m of those positions.
//   method 0: as the reference does it (interpolate the first m, evaluate at the rest: ~3 m^2 products);
//   method 1: the same predicate on coefficients.  The excluded points rou^(E j) are the B-th roots of unity, B = len / E, so the
//     checked points are the roots of V(x) = (x^len - 1)/(x^B - 1) = 1 + x^B + x^2B + ...  Let g be the interpolant of ALL len values
//     (an inverse transform of size len).  A polynomial f of degree < m agrees with g on the roots of V  <=>  g - f = V h with
//     deg h < B  <=>  the coefficients g_k, k >= m, depend on k mod B only (V h is h's coefficients repeated E times).  That f is
//     the reference's interpolant (degree < m through m of the points), so both methods accept exactly the same remainders;
//     len log len products instead of 3 m^2.  Used when E divides len (always, for the domains of this prover).
// returns true when the remainder passes
static bool remainder_is_low_degree(const std::vector<F> &remainder, uint64_t E, uint64_t m, F rou, int method) {
    const uint64_t len = remainder.size();
    std::vector<uint64_t> positions;
    for (uint64_t i = 0; i < len; i++) if (!E || i % E) positions.push_back(i);
    if (m > positions.size()) fail(GS_ERR_ARG, "Remainder degree is greater than number of remainder values");
    if (!m || m == positions.size()) return true;
    if (method == 1 && E && len >= E && len % E == 0 && !(len & (len - 1))) {
        const uint64_t B = len / E;
        std::vector<F> g(remainder);
        host_transform(g, hf_pow(rou, (hfe)(len - 1)));     // with rou^-1; unscaled: the predicate compares (canonical) coefficients with each other
        for (uint64_t k = m; k + B < len; k++)
            if (g[k] != g[k + B]) return false;
        return true;
    }
    std::vector<F> domain(len);
    F cur = 1;
    for (uint64_t i = 0; i < len; i++) { domain[i] = cur; cur = hf_mul(cur, rou); }
    Bytes xs(m * ELEM), ys(m * ELEM), poly(m * ELEM);
    for (uint64_t i = 0; i < m; i++) { store_elem(domain[positions[i]], xs.data() + ELEM * i); store_elem(remainder[positions[i]], ys.data() + ELEM * i); }
    if (A.gs_small_interpolate(xs.data(), ys.data(), (uint32_t)m, poly.data())) fail(GS_ERR_ARG, "gs_small_interpolate failed");
    const uint32_t rest = (uint32_t)(positions.size() - m);
    Bytes rx(rest * ELEM), rv(rest * ELEM);
    for (uint32_t i = 0; i < rest; i++) store_elem(domain[positions[m + i]], rx.data() + ELEM * i);
    if (A.gs_small_eval_poly(poly.data(), (uint32_t)m, rx.data(), rest, rv.data())) fail(GS_ERR_ARG, "gs_small_eval_poly failed");
    for (uint32_t i = 0; i < rest; i++)
        if (load_elem(rv.data() + ELEM * i) != remainder[positions[m + i]]) return false;
    return true;
}

namespace {

// ---- the statement plan: what both provers and the verifier derive from the statement and must agree on to the byte ----------
// compositionFactor = 2^ceil(log2(max constraint degree))
uint64_t composition_factor(const gs_prover_air &air) {
    uint32_t max_degree = 1;
    for (uint32_t i = 0; i < air.nconstraints; i++) max_degree = std::max(max_degree, air.degrees[i]);
    uint64_t cf = 1;
    while (cf < max_degree) cf <<= 1;
    return cf;
}
// FiniteField.interpolate(xs, ys) for the handful of points of an assertion set (the library's gs_small_interpolate): coefficients as
// bytes at `out`, or as elements
void interpolate(const std::vector<F> &xs, const std::vector<F> &ys, uint8_t *out) {
    const size_t n = xs.size();
    Bytes xb(n * ELEM), yb(n * ELEM);
    for (size_t i = 0; i < n; i++) { store_elem(xs[i], xb.data() + ELEM * i); store_elem(ys[i], yb.data() + ELEM * i); }
    if (A.gs_small_interpolate(xb.data(), yb.data(), (uint32_t)n, out)) fail(GS_ERR_ARG, "gs_small_interpolate failed");
}
std::vector<F> lagrange(const std::vector<F> &xs, const std::vector<F> &ys) {
    Bytes cb(xs.size() * ELEM);
    interpolate(xs, ys, cb.data());
    std::vector<F> out(xs.size());
    for (size_t i = 0; i < out.size(); i++) out[i] = load_elem(cb.data() + ELEM * i);
    return out;
}
Bytes pack(const std::vector<F> &v, size_t from, size_t count) {
    Bytes b(count * ELEM);
    for (size_t i = 0; i < count; i++) store_elem(v[from + i], b.data() + ELEM * i);
    return b;
}
std::vector<uint64_t> augmented_rows(const std::vector<uint64_t> &positions, uint64_t column_length) {      // LowDegreeProver.ts:302-309
    std::vector<uint64_t> out;
    for (uint64_t p : positions) out.push_back(p % (column_length / 4));
    return unique_in_order(out);
}

struct Plan {
    uint64_t T, E, N;
    F omega;                                            // generator of the evaluation domain (N points)
    uint64_t cf, Nc, combination_degree, composition_degree, b_inc;     // CompositionPolynomial.ts:196-204
    uint32_t exe_query_count, fri_query_count;
    // boundary constraints per asserted register, in order of first appearance (BoundaryConstraints.ts:15-45)
    // (xs: the assertions' points omega^(step E) — what the host-side interpolation works on; make_plan leaves them to fill_xs on request)
    struct Reg { uint32_t reg; std::vector<uint64_t> steps; std::vector<F> xs, ys; };
    std::vector<Reg> regs;
    void fill_xs() {
        size_t total = 0;
        for (auto &r : regs) total += r.steps.size();
        // an exponentiation per assertion, or — many assertions — the execution domain's points once (T products) and look-ups
        std::vector<F> table;
        if (total * 32 > T) {
            table.resize(T);
            const F g = hf_pow(omega, (hfe)E);
            F cur = 1;
            for (uint64_t j = 0; j < T; j++) { table[j] = cur; cur = hf_mul(cur, g); }
        }
        for (auto &r : regs) {
            r.xs.resize(r.steps.size());
            for (size_t k = 0; k < r.steps.size(); k++)
                r.xs[k] = !table.empty() && r.steps[k] < T ? table[r.steps[k]] : hf_pow(omega, (hfe)(r.steps[k] * E));
        }
    }

    // constraints grouped by degree (times T), in order of first appearance (CompositionPolynomial.ts:206-225)
    std::vector<std::pair<uint64_t, std::vector<uint32_t>>> groups;
    uint32_t dcount, bcoef;                              // coefficients of Q's terms, of the boundary terms

    // the coefficient stream from the evaluation root (lib/Stark.ts:121): dcount for Q, bcoef for B, then lccount(V) for the linear
    // combination of V committed vectors (LinearCombination.ts:58-59)
    uint32_t lccount(uint32_t V) const { return b_inc > 0 ? 2 * V : V; }
    std::vector<F> coefficients(const Bytes &root, uint32_t V) const { return prng_many(root, dcount + bcoef + lccount(V)); }

    // the product of (x - x_i) over a register's assertions (BoundaryConstraints.ts:24-30)
    std::vector<F> zero_poly(const Reg &r) const {
        return host_linear_product(r.xs);
    }
    // the asserted registers as rows of `width` (the most assertions on one register) for the boundary kernels: where each assertion's
    // point lies, in units of the domain's generator (step * unit), the count per row and — with_interpolants — each row's interpolant
    struct Boundary {
        uint32_t width = 0;
        std::vector<uint64_t> at;
        std::vector<uint32_t> per_row;
        Bytes interpolants;
    };
    Boundary boundary(uint64_t unit, bool with_interpolants) const {
        Boundary b;
        for (auto &r : regs) b.width = std::max(b.width, (uint32_t)r.steps.size());
        b.at.assign(regs.size() * b.width, 0);
        b.per_row.resize(regs.size());
        if (with_interpolants) b.interpolants.assign(regs.size() * b.width * ELEM, 0);
        for (size_t r = 0; r < regs.size(); r++) {
            b.per_row[r] = (uint32_t)regs[r].steps.size();
            for (size_t k = 0; k < regs[r].steps.size(); k++) b.at[r * b.width + k] = regs[r].steps[k] * unit;
            if (with_interpolants) interpolate(regs[r].xs, regs[r].ys, b.interpolants.data() + r * b.width * ELEM);    // BoundaryConstraints.ts:42
        }
        return b;
    }

    // query positions (lib/Stark.ts:146-152, QueryIndexGenerator.ts:28-32) from the root of the linear combination's tree ...
    std::vector<uint64_t> exe_positions(const Bytes &lc_root) const {
        return query_indexes(lc_root, (uint32_t)std::min<uint64_t>(exe_query_count, N - N / E), N, (uint32_t)E);
    }
    // ... the leaves of the evaluation tree they open: each position and its next step (lib/Stark.ts:274-296) ...
    std::vector<uint64_t> evaluation_positions(const std::vector<uint64_t> &positions) const {
        std::vector<uint64_t> aug;
        for (uint64_t p : positions) { aug.push_back(p); aug.push_back((p + E) % N); }
        return unique_in_order(aug);
    }
    // ... and per FRI layer, from the root of its column's tree: positions in the column, the rows of the column's tree (:209-219)
    struct Queries { std::vector<uint64_t> positions, rows; };
    Queries layer_queries(const Bytes &column_root, uint64_t column_length) const {
        Queries q;
        q.positions = query_indexes(column_root, fri_query_count, column_length, (uint32_t)E);
        q.rows = augmented_rows(q.positions, column_length);
        return q;
    }
};
// the trace of T steps at extension factor E, omega of order T E
Plan make_plan(const gs_prover_job &job, uint64_t T, uint64_t E, F omega, bool with_xs = true) {
    const gs_prover_air &air = job.air;
    Plan p;
    p.T = T; p.E = E; p.N = T * E; p.omega = omega;
    p.cf = composition_factor(air);
    p.Nc = T * p.cf;
    p.combination_degree = p.cf * T;
    p.composition_degree = std::max(p.combination_degree - T, T);
    p.b_inc = p.composition_degree - T;
    p.exe_query_count = job.exe_query_count;
    p.fri_query_count = job.fri_query_count;
    std::vector<int32_t> slot(air.registers, -1);             // register -> its entry of p.regs (a statement may assert thousands of cells)
    for (uint32_t i = 0; i < job.nassertions; i++) {
        const gs_assertion &a = job.assertions[i];
        int32_t at = -1;
        if (a.reg < slot.size()) at = slot[a.reg];
        else for (size_t k = 0; k < p.regs.size(); k++) if (p.regs[k].reg == a.reg) at = (int32_t)k;      // (out of range: refused by the caller)
        if (at < 0) {
            at = (int32_t)p.regs.size();
            p.regs.push_back(Plan::Reg{a.reg, {}, {}, {}});
            if (a.reg < slot.size()) slot[a.reg] = at;
        }
        Plan::Reg &r = p.regs[at];
        r.steps.push_back(a.step);
        r.ys.push_back(load_elem(a.value));
    }
    if (with_xs) p.fill_xs();
    for (uint32_t i = 0; i < air.nconstraints; i++) {
        const uint64_t d = (uint64_t)air.degrees[i] * T;
        bool found = false;
        for (auto &g : p.groups) if (g.first == d) { g.second.push_back(i); found = true; }
        if (!found) p.groups.push_back({d, {i}});
    }
    p.dcount = air.nconstraints;
    for (auto &g : p.groups) if (g.first < p.combination_degree) p.dcount += (uint32_t)g.second.size();
    p.bcoef = (uint32_t)p.regs.size() * (p.composition_degree > T ? 2 : 1);
    return p;
}

// Q = every constraint's plain term + each group's degree-adjusted terms (CompositionPolynomial.ts:83-107), n values per vector:
// gs_combine_adjusted merges sum k_i q_i + powers o sum k'_i q_i in one pass, the adjusted vectors are not materialised (one further
// pass per additional group of a degree of its own: different powers).  powers(e) gives x^e over the same n points
template <class Powers>
void merge_q(Ctx &x, const Plan &plan, const std::vector<F> &co, const std::vector<const void *> &qa, uint64_t n, Powers &&powers, void *merged) {
    const uint32_t nq = (uint32_t)qa.size();
    Bytes plain = pack(co, 0, nq);
    uint32_t next = nq;                                      // coefficients of the adjusted terms follow, group by group
    bool first = true;
    for (auto &g : plan.groups) {
        if (g.first == plan.combination_degree) continue;
        Buf pw = powers(plan.combination_degree - g.first);
        if (first) {                                         // every constraint's plain term + this group's adjusted terms
            Bytes adj(nq * ELEM, 0);
            for (uint32_t i : g.second) store_elem(co[next++], adj.data() + ELEM * i);
            x.check(A.gs_combine_adjusted(x.c, qa.data(), plain.data(), adj.data(), nq, pw.p, nullptr, n, merged), "gs_combine_adjusted(Q)");
        } else {
            std::vector<const void *> members;
            Bytes adj(g.second.size() * ELEM);
            for (size_t k = 0; k < g.second.size(); k++) { members.push_back(qa[g.second[k]]); store_elem(co[next++], adj.data() + ELEM * k); }
            x.check(A.gs_combine_adjusted(x.c, members.data(), nullptr, adj.data(), (uint32_t)members.size(), pw.p, merged, n, merged), "gs_combine_adjusted(Q)");
        }
        first = false;
    }
    if (first) x.check(A.gs_combine_many(x.c, qa.data(), plain.data(), nq, n, merged), "gs_combine_many(Q)");
}

// LowDegreeProver.verifyRemainder (:223-252) for a prover: the remainder after `depth` layers lies on the powers of omega^(4^depth)
void check_remainder(const Plan &plan, const std::vector<F> &remainder, uint32_t depth) {
    F rou = plan.omega;
    uint64_t max_degree_plus1 = plan.composition_degree;
    for (uint32_t d = 0; d < depth; d++) { rou = hf_mul(rou, rou); rou = hf_mul(rou, rou); max_degree_plus1 /= 4; }
    if (!remainder_is_low_degree(remainder, plan.E, max_degree_plus1, rou, 1))
        fail(GS_ERR_ARG, "Low degree proof failed: Remainder is not a valid degree %llu polynomial", (unsigned long long)(max_degree_plus1 - 1));
}

// Serializer.serializeProof (:35-79)
struct Component { Bytes columnRoot; MerkleProof columnProof, polyProof; };
void write_proof(Bytes &out, const Bytes &evRoot, const MerkleProof &evProof, uint32_t V, const Bytes &lcRoot, const MerkleProof &lcProof,
                 const std::vector<Component> &components, const std::vector<F> &remainder, const Shapes &input_shapes) {
    out.clear();
    out.insert(out.end(), evRoot.begin(), evRoot.end());
    write_merkle_proof(out, evProof, (uint64_t)V * ELEM);
    out.insert(out.end(), lcRoot.begin(), lcRoot.end());
    write_merkle_proof(out, lcProof, 4 * ELEM);
    if (components.size() > 255) fail(GS_ERR_ARG, "too many FRI components");
    out.push_back((uint8_t)components.size());
    for (auto &c : components) {
        out.insert(out.end(), c.columnRoot.begin(), c.columnRoot.end());
        write_merkle_proof(out, c.columnProof, 4 * ELEM);
        write_merkle_proof(out, c.polyProof, 4 * ELEM);
    }
    if (remainder.size() > MAX_ARRAY) fail(GS_ERR_ARG, "remainder too long");
    out.push_back(remainder.size() == MAX_ARRAY ? 0 : (uint8_t)remainder.size());
    for (F v : remainder) { uint8_t b[ELEM]; store_elem(v, b); out.insert(out.end(), b, b + ELEM); }
    write_input_shapes(out, input_shapes);
}

// ---- the steps both provers issue, each written once --------------------------------------------------------------------------
// What a job is refused for (the assertions: lib/Stark.ts:356-375).  Each prover runs these where ITS sequence reaches them.
void check_job(const gs_prover_job &job) {
    const uint64_t T = job.steps, E = job.extension_factor;
    if (!T || (T & (T - 1)) || !E || (E & (E - 1)) || !job.air.registers || !job.air.nconstraints || !job.nassertions) fail(GS_ERR_ARG, "invalid job");
}
void check_extension_factor(const gs_prover_job &job) {
    if (job.extension_factor < 2 * composition_factor(job.air)) fail(GS_ERR_ARG, "extension factor must be at least 2x the composition factor");
}
void check_fri_length(uint64_t N) {
    if (N < 128) fail(GS_ERR_ARG, "Invalid array length");
}
void check_assertion_ranges(const gs_prover_job &job) {
    for (uint32_t i = 0; i < job.nassertions; i++) {
        const gs_assertion &a = job.assertions[i];
        if (a.reg >= job.air.registers) fail(GS_ERR_ARG, "Invalid assertion: register %u is outside of register bank", a.reg);
        if (a.step >= job.steps) fail(GS_ERR_ARG, "Invalid assertion: step %llu is outside of execution trace", (unsigned long long)a.step);
    }
}
// cell(i): the bytes the trace holds where assertion i points
template <class Cell>
void check_asserted_cells(const gs_prover_job &job, Cell &&cell) {
    for (uint32_t i = 0; i < job.nassertions; i++)
        if (memcmp(cell(i), job.assertions[i].value, ELEM))
            fail(GS_ERR_ARG, "Assertion at step %llu, register %u conflicts with execution trace", (unsigned long long)job.assertions[i].step,
                 job.assertions[i].reg);
}

// generateExecutionTrace (lib/Stark.ts:97) into `out`, registers x steps.  first_rows / segments: the job's, or — a rank generating its
// own segments of a segmented AIR — that rank's
void launch_trace(Ctx &x, const gs_prover_job &job, const uint8_t *first_rows, uint64_t segments, void *out) {
    const gs_prover_air &air = job.air;
    if (air.kind == 0)
        x.check(A.gs_mimc_trace(x.c, air.seed, air.round_constants, air.nrc, job.steps, out), "gs_mimc_trace");
    else if (segments)
        x.check(A.gs_air_trace_segments(x.c, air.t_code, air.t_ninstr, air.i_code, air.i_ninstr, air.consts, air.nconsts, air.vm_regs, air.registers,
                                        air.static_values, air.static_periods, air.nstatic, first_rows, segments, air.segment_len, out),
                "gs_air_trace_segments");
    else
        x.check(A.gs_air_trace(x.c, air.t_code, air.t_ninstr, air.consts, air.nconsts, air.vm_regs, air.registers, air.static_values, air.static_periods,
                               air.nstatic, first_rows, job.steps, out), "gs_air_trace");
}

// The points the composition steps run over: {shift * root^k, k < n}.  The single-device prover works on the whole evaluation domain,
// {N, omega, 1, E}; rank g of G on its strided share of it, {N / G, omega^G, omega^g, E / G}.  The library takes the whole domain through
// its plain entry points and a share — rank 0's, whose shift is 1, included — through their _coset twins.
struct Coset {
    uint64_t n;
    F root, shift;
    uint64_t unit;       // one trace step in powers of root: an assertion at step s is the point root^(s unit); x^T takes `unit` values
    bool whole;
};
// x^e over the points of a coset
Buf coset_powers(Ctx &x, const Coset &c, uint64_t e) {
    Buf out(x, c.n * ELEM);
    x.check(A.gs_power_series(x.c, enc(hf_pow(c.root, (hfe)e)), c.n, out.p), "gs_power_series");
    if (c.shift != (F)1) x.check(A.gs_vec_mul_scalar(x.c, out.p, enc(hf_pow(c.shift, (hfe)e)), c.n, out.p), "gs_vec_mul_scalar(coset shift)");
    return out;
}
// 1/Z(x) (ZeroPolynomial.ts:36-44 and the division of CompositionPolynomial.ts:117).  x^T - 1 takes only c.unit distinct values: up to 32
// of them are a table and one product per point inside one kernel; beyond that (no host builds such a statement: extension factors
// stop at 32) the vectors are formed as the reference forms them
Buf zero_poly_inverses(Ctx &x, const Plan &plan, const Coset &c) {
    const uint64_t n = c.n, T = plan.T;
    const Enc last = enc(hf_pow(plan.omega, (hfe)((T - 1) * plan.E)));                              // :21-23: the last step's point
    Buf out(x, n * ELEM);
    if (c.unit <= 32) {
        if (c.whole) x.check(A.gs_zero_poly_inverses(x.c, enc(c.root), n, T, last, out.p), "gs_zero_poly_inverses");
        else x.check(A.gs_zero_poly_inverses_coset(x.c, enc(c.root), n, enc(c.shift), T, last, out.p), "gs_zero_poly_inverses_coset");
        return out;
    }
    Buf domain = coset_powers(x, c, 1), xToTheSteps, num(x, n * ELEM), den(x, n * ELEM);
    if (c.whole) {
        xToTheSteps = Buf(x, n * ELEM);
        x.check(A.gs_pluck(x.c, domain.p, n, T, n, xToTheSteps.p), "gs_pluck");                      // :40
    } else {
        xToTheSteps = coset_powers(x, c, T);                                                        // pluck(domain, T, N) = (w^T)^i, my share
    }
    x.check(A.gs_vec_sub_scalar(x.c, xToTheSteps.p, enc((F)1), n, num.p), "gs_vec_sub_scalar");
    x.check(A.gs_vec_sub_scalar(x.c, domain.p, last, n, den.p), "gs_vec_sub_scalar");
    x.check(A.gs_vec_div(x.c, den.p, num.p, n, out.p), "gs_vec_div(1/Z)");
    return out;
}
// 5.4-5.7 and 6 in ONE pass (gs_composition_tail[_coset]) when the assertions fit its per-register limits (tail_fits): D = Q / Z, the
// boundary quotients from the registers' extensions `pv`, their degree-adjusted merge, and LinearCombination.computeMany (:36-64: the
// same coefficient stream continues) over the committed vectors on top.  z_inverses null: the kernel makes 1/Z(x) itself
void composition_tail(Ctx &x, const Plan &plan, const Coset &c, const std::vector<F> &coefficients, const void *qe, const void *z_inverses,
                      const std::vector<const void *> &pv, const std::vector<const void *> &eVectors, void *out) {
    const uint32_t bcount = (uint32_t)plan.regs.size(), V = (uint32_t)eVectors.size();
    const bool adjust = plan.b_inc > 0;
    const Plan::Boundary bd = plan.boundary(c.unit, true);                // an interpolant through m assertions has m coefficients
    const Bytes bco = pack(coefficients, plan.dcount, plan.bcoef), cb = pack(coefficients, plan.dcount + plan.bcoef, plan.lccount(V));
    const Enc last = enc(hf_pow(plan.omega, (hfe)((plan.T - 1) * plan.E)));                         // ZeroPolynomial.ts:21-23
    if (c.whole)
        x.check(A.gs_composition_tail(x.c, c.n, enc(c.root), qe, z_inverses, plan.T, last, pv.data(), bcount, bd.interpolants.data(), bd.width, bd.at.data(),
                                      bd.per_row.data(), bd.width, bco.data(), adjust ? bco.data() + ELEM * bcount : nullptr, eVectors.data(), V, cb.data(),
                                      adjust ? cb.data() + ELEM * V : nullptr, nullptr, plan.b_inc, nullptr, out), "gs_composition_tail");
    else
        x.check(A.gs_composition_tail_coset(x.c, c.n, enc(c.root), enc(c.shift), qe, z_inverses, plan.T, last, pv.data(), bcount, bd.interpolants.data(), bd.width,
                                            bd.at.data(), bd.per_row.data(), bd.width, bco.data(), adjust ? bco.data() + ELEM * bcount : nullptr, eVectors.data(), V,
                                            cb.data(), adjust ? cb.data() + ELEM * V : nullptr, nullptr, plan.b_inc, nullptr, out), "gs_composition_tail_coset");
}
// ... and the same member by member -> cEval; qe and zInverses are consumed.
// device_boundary: I_r and Z_r are built on the device (gs_boundary_polys: the whole domain only) instead of this host core
void member_sequence(Ctx &x, const Plan &plan, const Coset &c, bool device_boundary, const std::vector<F> &coefficients, Buf &qe, Buf &zInverses,
                     const std::vector<const void *> &pv, const Buf &psbPowers, void *cEval) {
    const uint64_t n = c.n;
    const uint32_t bcount = (uint32_t)plan.regs.size();
    // 5.4 D(x) = Q(x) / Z(x) (:113-121)
    Buf dEval(x, n * ELEM);
    x.check(A.gs_vec_mul(x.c, qe.p, zInverses.p, n, dEval.p), "gs_vec_mul(D)");
    qe.release();
    zInverses.release();
    // 5.5 boundary constraints (BoundaryConstraints.ts:71-95)
    const Plan::Boundary bd = plan.boundary(c.unit, false);
    const uint32_t ilen = bd.width, zlen = bd.width + 1;                  // m assertions: m interpolant coefficients, m + 1 of Z_r
    if (!c.whole && (ilen > n || zlen > n)) fail(GS_ERR_UNSUPPORTED, "more assertions on a register than points per rank");
    // rows of coefficients for the device; on a share a polynomial is evaluated at shift * root^k: its coefficients scaled by shift^j
    auto upload_rows = [&](const std::vector<std::vector<F>> &rows, size_t len) {
        Bytes host(rows.size() * len * ELEM, 0);                        // shorter rows are zero-extended (newMatrixFromVectors)
        for (size_t r = 0; r < rows.size(); r++) {
            F sj = 1;
            for (size_t k = 0; k < rows[r].size(); k++) {
                store_elem(c.whole ? rows[r][k] : hf_mul(rows[r][k], sj), host.data() + (r * len + k) * ELEM);
                if (!c.whole) sj = hf_mul(sj, c.shift);
            }
        }
        Buf b(x, host.size());
        x.check(A.gs_upload(x.c, b.p, host.data(), host.size()), "gs_upload(boundary polynomials)");
        return b;
    };
    Buf iPolys, zPolys;
    if (device_boundary) {
        iPolys = Buf(x, (uint64_t)bcount * ilen * ELEM);
        zPolys = Buf(x, (uint64_t)bcount * zlen * ELEM);
        std::vector<uint64_t> at((size_t)bcount * bd.width, 0);
        Bytes ys((size_t)bcount * bd.width * ELEM, 0);
        for (uint32_t r = 0; r < bcount; r++)
            for (size_t k = 0; k < plan.regs[r].steps.size(); k++) {
                at[(size_t)r * bd.width + k] = plan.regs[r].steps[k];
                store_elem(plan.regs[r].ys[k], ys.data() + ((size_t)r * bd.width + k) * ELEM);
            }
        x.check(A.gs_boundary_polys(x.c, enc(plan.omega), plan.N, plan.T, at.data(), ys.data(), bd.per_row.data(), bcount, bd.width, iPolys.p, zPolys.p),
                "gs_boundary_polys");
    } else {
        std::vector<std::vector<F>> ipolys;
        for (auto &r : plan.regs) ipolys.push_back(lagrange(r.xs, r.ys));
        iPolys = upload_rows(ipolys, ilen);
    }
    Buf iValues(x, (uint64_t)bcount * n * ELEM), pi(x, (uint64_t)bcount * n * ELEM), bEval(x, (uint64_t)bcount * n * ELEM);
    x.check(counted_eval_polys_at_roots(x.c, iPolys.p, bcount, ilen, enc(c.root), n, iValues.p), "gs_eval_polys_at_roots(I)");
    x.check(A.gs_sub_matrix_from_vectors(x.c, pv.data(), iValues.p, bcount, n, pi.p), "gs_sub_matrix_from_vectors");
    if (bd.width <= 4) {
        // the divisors' roots are points root^j of the domain: look-ups in its table 1 / (shift root^j - 1) instead of evaluating Z_r(x)
        // and inverting it (same values: BoundaryConstraints.ts:88,92)
        if (c.whole) x.check(A.gs_div_by_domain_roots(x.c, pi.p, bcount, n, enc(c.root), bd.at.data(), bd.per_row.data(), bd.width, bEval.p), "gs_div_by_domain_roots");
        else x.check(A.gs_div_by_domain_roots_coset(x.c, pi.p, bcount, n, enc(c.root), enc(c.shift), bd.at.data(), bd.per_row.data(), bd.width, bEval.p),
                     "gs_div_by_domain_roots_coset");
    } else {
        if (!device_boundary) {
            std::vector<std::vector<F>> zpolys;
            for (auto &r : plan.regs) zpolys.push_back(plan.zero_poly(r));
            zPolys = upload_rows(zpolys, zlen);
        }
        Buf zValues(x, (uint64_t)bcount * n * ELEM);
        x.check(counted_eval_polys_at_roots(x.c, zPolys.p, bcount, zlen, enc(c.root), n, zValues.p), "gs_eval_polys_at_roots(Zb)");
        x.check(A.gs_vec_div(x.c, pi.p, zValues.p, (uint64_t)bcount * n, bEval.p), "gs_vec_div(B)");
    }
    iValues.release(); pi.release();
    // 5.6 degree adjustment of B (:124-138) and 5.7 merge (:140-146), with D added in the same pass
    const Bytes bco = pack(coefficients, plan.dcount, plan.bcoef);
    std::vector<const void *> ba;
    for (uint32_t i = 0; i < bcount; i++) ba.push_back(bEval.at((uint64_t)i * n * ELEM));
    x.check(A.gs_combine_adjusted(x.c, ba.data(), bco.data(), plan.b_inc > 0 ? bco.data() + ELEM * bcount : nullptr, bcount, plan.b_inc > 0 ? psbPowers.p : nullptr,
                                  dEval.p, n, cEval), "gs_combine_adjusted(B + D)");
}
// 6 random linear combination (LinearCombination.ts:36-64).  psIncrementalDegree = compositionDegree - T: the same powers as B's;
// P_r o powers is not materialised, C is added in the pass
void linear_combination(Ctx &x, const Plan &plan, const std::vector<F> &coefficients, const std::vector<const void *> &eVectors, const Buf &psbPowers,
                        const void *cEval, uint64_t n, void *lEval) {
    const uint32_t V = (uint32_t)eVectors.size();
    const Bytes cb = pack(coefficients, plan.dcount + plan.bcoef, plan.lccount(V));
    x.check(A.gs_combine_adjusted(x.c, eVectors.data(), cb.data(), plan.b_inc > 0 ? cb.data() + ELEM * V : nullptr, V, plan.b_inc > 0 ? psbPowers.p : nullptr, cEval, n,
                                  lEval), "gs_combine_adjusted(L)");
}

// One FRI layer's products: the folded column (a quarter of the layer's values) and the tree over its rows
struct Fold { Buf next; Tree cTree; };
// LowDegreeProver.ts:176-221 on a column that is whole and in natural order, the recursion unrolled: every layer's buffers first, then
// ONE call (gs_fri_layers = per layer gs_fri_fold_at :189-198 + gs_merkle_commit_rows_seed :201-202, with as few dependent launches as
// the sizes allow).  `column`: len values, layer log4(step) of a domain of N points; `point`: where its first fold is taken, on the device
std::vector<Fold> fri_layers(Ctx &x, int alg, F omega, uint64_t N, uint64_t step, const void *column, uint64_t len, const void *point) {
    std::vector<Fold> folds;
    for (uint64_t l = len; l > 256; l /= 4) {
        const uint64_t rows = l / 4;
        folds.emplace_back();
        Fold &f = folds.back();
        f.next = Buf(x, rows * ELEM);
        f.cTree.n = rows / 4;
        f.cTree.leaves = Buf(x, rows / 4 * DIGEST);
        f.cTree.nodes = Buf(x, rows / 4 * DIGEST);
        if (rows > 256) f.cTree.point = Buf(x, ELEM);                                                 // (no layer below the last tree)
        f.cTree.root.resize(DIGEST);
    }
    if (folds.empty()) return folds;
    std::vector<gs_fri_layer> outs(folds.size());
    for (size_t d = 0; d < folds.size(); d++) outs[d] = gs_fri_layer{folds[d].next.p, folds[d].cTree.leaves.p, folds[d].cTree.nodes.p, folds[d].cTree.point.p, 0};
    x.check(A.gs_fri_layers(x.c, (gs_hash_alg)alg, enc(omega), N, step, column, len, point, (uint32_t)outs.size(), outs.data()), "gs_fri_layers");
    for (size_t d = 0; d < folds.size(); d++) folds[d].cTree.ticket = outs[d].ticket;
    return folds;
}

}  // namespace

static void prove_impl(Ctx &x, const gs_prover_job &job, Bytes &out) {
    PhaseClock clock;
    const gs_prover_air &air = job.air;
    const uint64_t T = job.steps, E = job.extension_factor, N = T * E;
    const uint32_t R = air.registers;
    const int alg = job.hash_alg;
    check_job(job);
    const Shapes input_shapes = checked_job_shapes(job);          // iShapes of the proof (lib/Stark.ts:161); empty without input registers
    check_extension_factor(job);
    const F omega = domain_root(job, N);
    Plan plan = make_plan(job, T, E, omega, false);
    const uint64_t Nc = plan.Nc, combination_degree = plan.combination_degree, b_inc = plan.b_inc;
    const F comp_rou = hf_pow(omega, (hfe)(N / Nc)), exec_rou = hf_pow(omega, (hfe)E);
    const Coset domain{N, omega, 1, E, true};                     // the whole evaluation domain

    // 1 ----- evaluation context (lib/Stark.ts:92-94): the kernels below derive domain points from omega; the evaluation domain is
    // materialised only by the general Z(x) sequence

    // work of CompositionPolynomial.evaluateAll that does not depend on the trace goes first: the device computes it while
    // the host core below runs the trace recurrence (same values, issue order only)
    // MiMC with up to four assertions: the whole of CompositionPolynomial.evaluateAll is one kernel over the evaluation domain
    // (gs_mimc_composition, below); otherwise the member-by-member sequence, whose trace-independent part is issued here
    uint32_t assertions_on_r0 = 0;
    for (uint32_t i = 0; i < job.nassertions; i++) assertions_on_r0 += job.assertions[i].reg == 0;
    const bool fused = air.kind == 0 && E <= 32 && air.nconstraints == 1 && assertions_on_r0 == job.nassertions && job.nassertions <= 4;
    // the generic sequence's tail in one pass (gs_composition_tail) when the assertions fit its per-register limits: neither 1/Z(x) nor
    // the power series of the degree adjustment is materialised then
    const bool tail = !fused && tail_fits(job, R + air.nsecret);
    const bool tail_makes_z = tail && domain.unit <= 32;
    // registers with many assertions: I_r and Z_r are built on the device (gs_boundary_polys) where the bound
    // library has that entry point — otherwise, and for the few assertions of every other statement, on this host core
    uint32_t most_assertions = 0;
    for (auto &r : plan.regs) most_assertions = std::max(most_assertions, (uint32_t)r.steps.size());
    // (the device path costs a fixed ~0.3 ms of transforms and launches whatever the count; measured, profiles/boundary_polys.md: at 128
    //  assertions on a register the host path is still ahead — 1.44 vs 1.53 ms at 2^13 steps, 5.09 vs 5.23 at 2^16 —, at 256 it is behind)
    const uint32_t DEVICE_BOUNDARY_ABOVE = 128;
    const bool device_boundary = !fused && !tail && most_assertions > DEVICE_BOUNDARY_ABOVE && A.gs_boundary_polys && !g_host_boundary && plan.regs.size() <= 64 &&
                                 most_assertions <= T && T <= (1ull << 28);
    if (!device_boundary) plan.fill_xs();
    Buf zInverses;
    if (!fused && !tail_makes_z) zInverses = zero_poly_inverses(x, plan, domain);
    Buf psbPowers;                                                 // x^(compositionDegree - T) over the evaluation domain
    const bool lc_folds = fused && R + air.nsecret == 1;           // LinearCombination folded into the composition kernel too
    if (b_inc > 0 && !lc_folds && !tail) psbPowers = coset_powers(x, domain, b_inc);       // also what LinearCombination.ts:44-52 multiplies by

    // MiMC: the cyclic register K over the evaluation domain — its 64 coefficients from the composition-domain table, then its values
    // at the (k_len * N/Nc)-th roots of unity (the constraint is evaluated on all N points from the extension of P)
    Buf kN;
    uint64_t klen_n = 0;
    if (air.kind == 0) {
        klen_n = air.k_len * (N / Nc);
        Buf kPoly(x, air.k_len * ELEM);
        kN = Buf(x, klen_n * ELEM);
        x.check(counted_interpolate_roots(x.c, air.k_table, 1, enc(hf_pow(omega, (hfe)(N / air.k_len))), air.k_len, kPoly.p), "gs_interpolate_roots(K)");
        x.check(counted_eval_polys_at_roots(x.c, kPoly.p, 1, air.k_len, enc(hf_pow(omega, (hfe)(N / klen_n))), klen_n, kN.p), "gs_eval_polys_at_roots(K)");
    }

    // MiMC, fused: the per-point factors of the composition pass that need neither the trace nor a coefficient — the domain points, the
    // interpolant through the assertions, the divisions by (x - x_a) — are tabulated now, while the device has nothing else to do
    // (include/gstark_mimc.h), where the bound library has the entry points; it answers GS_OK also when it declines to make the
    // tables and its composition call then runs gs_mimc_composition.  Assertions the checks below will refuse are left to them
    Plan::Boundary fused_bd;
    bool comp_tables = false;
    if (fused && A.gs_mimc_composition_prepare && A.gs_mimc_composition_tables) {
        const std::vector<uint64_t> &at = plan.regs[0].steps;
        bool sound = true;
        for (size_t i = 0; i < at.size(); i++) {
            if (at[i] >= T) sound = false;
            for (size_t k = 0; k < i; k++) if (at[k] == at[i]) sound = false;
        }
        if (sound) {
            fused_bd = plan.boundary(E, true);
            comp_tables = A.gs_mimc_composition_prepare(x.c, N, T, enc(omega), fused_bd.at.data(), fused_bd.per_row[0], fused_bd.interpolants.data()) == GS_OK;
        }
    }

    clock.mark("context + trace-independent work issued");
    clock.readme(x, "Set up evaluation context");
    // 2 ----- execution trace (:97) and the assertions it must satisfy (:356-375)
    Buf trace(x, (uint64_t)R * T * ELEM);
    launch_trace(x, job, air.first_rows, air.segments, trace.p);
    // the asserted cells (:356-375) are compared when the evaluation root comes back: one round trip for both
    check_assertion_ranges(job);
    std::vector<uint64_t> asserted_at;
    for (uint32_t i = 0; i < job.nassertions; i++) asserted_at.push_back((uint64_t)job.assertions[i].reg * T + job.assertions[i].step);

    clock.mark("execution trace (host recurrence)");
    clock.readme(x, "Generated execution trace");
    // 3 ----- P(x) and its low-degree extension (:106-109)
    Buf pPolys(x, (uint64_t)R * T * ELEM), pEval(x, (uint64_t)R * N * ELEM);
    x.check(counted_interpolate_roots(x.c, trace.p, R, enc(exec_rou), T, pPolys.p), "gs_interpolate_roots(trace)");
    clock.readme(x, "Computed execution trace polynomials P(x)");
    x.check(counted_eval_polys_at_roots(x.c, pPolys.p, R, T, enc(omega), N, pEval.p), "gs_eval_polys_at_roots(P)");
    clock.readme(x, "Low-degree extended P(x) polynomials over evaluation domain");
    std::vector<const void *> pRows(R);
    for (uint32_t r = 0; r < R; r++) pRows[r] = pEval.at((uint64_t)r * N * ELEM);
    std::vector<const void *> eVectors(pRows);                    // [P_0.., S_0..] (lib/Stark.ts:113-114)
    for (uint32_t i = 0; i < air.nsecret; i++) eVectors.push_back(air.secret_traces[i]);
    const uint32_t V = (uint32_t)eVectors.size();

    // 4 ----- evaluation Merkle tree (:113-118)
    Tree eTree = commit_rows(x, alg, eVectors.data(), V, N, false);

    clock.mark("P(x), extension, evaluation tree issued");
    clock.readme(x, "Serialized evaluations of P(x) and S(x) polynomials + Built evaluation merkle tree (one fused call)");
    // 5 ----- composition polynomial (CompositionPolynomial.ts:29-146)
    const uint32_t dcount = plan.dcount, bcoef = plan.bcoef;
    // The coefficients come from the evaluation root (:121): it is read where the first of them is needed, with the asserted cells —
    // the work that needs neither (constraint evaluation, degree adjustment) is queued first and covers the round trip
    std::vector<F> coefficients;
    auto read_evaluation_root = [&] {
        Bytes got(asserted_at.size() * ELEM);
        const uint64_t one = 1;                        // record 1 of a node array (32-byte records) is the root
        DeferWindow win(x);
        x.check(A.gs_gather(x.c, trace.p, ELEM, asserted_at.data(), asserted_at.size(), got.data()), "gs_gather(asserted cells)");
        x.check(A.gs_gather(x.c, eTree.nodes.p, DIGEST, &one, 1, eTree.root.data()), "gs_gather(root)");
        win.end();
        check_asserted_cells(job, [&](uint32_t i) { return got.data() + i * ELEM; });
        trace.release();
        coefficients = plan.coefficients(eTree.root, V);
    };

    Buf cEval(x, N * ELEM);
    bool lc_fused = false;                     // cEval already holds L (LinearCombination folded into the composition kernel)
    if (fused) {
        // K over the evaluation domain (issued before the trace), the interpolant through the assertions (all on register 0: one row
        // of the boundary plan), then one kernel for :71-146 (what needs no coefficient first: the device is idle while the root travels)
        const Plan::Boundary bd = comp_tables ? std::move(fused_bd) : plan.boundary(E, true);
        read_evaluation_root();
        const bool q_adjusted = plan.groups[0].first < combination_degree;
        Bytes co(4 * ELEM, 0);
        store_elem(coefficients[0], co.data());
        if (q_adjusted) store_elem(coefficients[1], co.data() + ELEM);
        store_elem(coefficients[dcount], co.data() + 2 * ELEM);
        if (b_inc > 0) store_elem(coefficients[dcount + 1], co.data() + 3 * ELEM);
        // ... and, with one committed vector, LinearCombination.computeMany (:36-64) on top: the same prng stream continues
        lc_fused = lc_folds;
        Bytes lc = lc_folds ? pack(coefficients, dcount + bcoef, plan.lccount(V)) : Bytes();
        lc.resize(2 * ELEM, 0);                                    // (the kernel reads two; the second is 0 without a degree adjustment)
        const auto composition = comp_tables ? A.gs_mimc_composition_tables : A.gs_mimc_composition;      // (same arguments, same values)
        x.check(composition(x.c, pRows[0], N, T, enc(omega), kN.p, klen_n, co.data(), q_adjusted ? combination_degree - plan.groups[0].first : 0, b_inc,
                            bd.interpolants.data(), bd.at.data(), bd.per_row[0], lc_folds ? lc.data() : nullptr, cEval.p),
                comp_tables ? "gs_mimc_composition_tables" : "gs_mimc_composition");
    } else {
        // 5.1-5.3: the combined, degree-adjusted Q has degree < Nc, so its extension to the evaluation domain (:109-110) is what
        // the constraint expression gives there.  MiMC (one cheap constraint): evaluate it on all N points from the extension of P
        // already at hand — no interpolation + extension; AIR programs: on the composition domain as the reference does.
        const bool direct = air.kind == 0;
        const Coset qDomain = direct ? domain : Coset{Nc, comp_rou, 1, Nc / T, true};
        const uint64_t Nq = qDomain.n;
        Buf q(x, (uint64_t)air.nconstraints * Nq * ELEM);
        if (direct) {
            x.check(A.gs_mimc_constraints(x.c, pRows[0], N, N / T, kN.p, klen_n, q.p), "gs_mimc_constraints");
        } else {
            // P over the composition domain is every (N/Nc)-th element of the extension just computed (:76)
            // (the R rows are one contiguous R x N matrix and N / Nc divides N: ONE strided pick over the whole matrix gives R x Nc)
            // — read in place, with that stride: no plucked copy (R x Nc elements written and read again)
            x.check(A.gs_air_constraints_strided(x.c, air.e_code, air.e_ninstr, air.consts, air.nconsts, air.vm_regs, R, air.nconstraints, pEval.p, N, N / Nc,
                                                 Nc, Nc / T, air.static_tables, air.static_lens, air.nstatic, q.p), "gs_air_constraints_strided");
        }
        // 5.2 degree adjustment (:83-101) and 5.3 merge + extension (:103-111)
        std::vector<const void *> qa;
        for (uint32_t i = 0; i < air.nconstraints; i++) qa.push_back(q.at((uint64_t)i * Nq * ELEM));
        read_evaluation_root();
        Buf qe(x, N * ELEM), qc;
        if (!direct) qc = Buf(x, Nc * ELEM);
        merge_q(x, plan, coefficients, qa, Nq, [&](uint64_t e) { return coset_powers(x, qDomain, e); }, direct ? qe.p : qc.p);
        if (!direct) {
            Buf qcPoly(x, Nc * ELEM);
            x.check(counted_interpolate_roots(x.c, qc.p, 1, enc(comp_rou), Nc, qcPoly.p), "gs_interpolate_roots(Q)");
            x.check(counted_eval_polys_at_roots(x.c, qcPoly.p, 1, Nc, enc(omega), N, qe.p), "gs_eval_polys_at_roots(Q)");
        }
        // 5.4-5.7: in ONE pass with 6 on top (gs_composition_tail) when the assertions fit its per-register limits, else member by member
        std::vector<const void *> pv;                                      // the asserted registers' extensions
        for (auto &r : plan.regs) pv.push_back(pRows[r.reg]);
        if (tail) {
            composition_tail(x, plan, domain, coefficients, qe.p, tail_makes_z ? nullptr : zInverses.p, pv, eVectors, cEval.p);
            lc_fused = true;
        } else {
            member_sequence(x, plan, domain, device_boundary, coefficients, qe, zInverses, pv, psbPowers, cEval.p);
        }
    }
    zInverses.release();

    clock.readme(x, lc_fused ? "Computed composition polynomial C(x) + Combined P(x) and S(x) evaluations with C(x) evaluations (one kernel)"
                            : "Computed composition polynomial C(x)");
    // 6 ----- random linear combination (LinearCombination.ts:36-64)
    Buf lEval;
    if (lc_fused) {
        lEval = std::move(cEval);
    } else {
        lEval = Buf(x, N * ELEM);
        linear_combination(x, plan, coefficients, eVectors, psbPowers, cEval.p, N, lEval.p);
    }
    cEval.release();
    psbPowers.release();

    if (!lc_fused) clock.readme(x, "Combined P(x) and S(x) evaluations with C(x) evaluations");
    clock.mark("composition + LC issued (root read inside)");
    // 7 ----- low-degree proof (LowDegreeProver.ts:39-68, 176-221)
    check_fri_length(N);
    // transposeVector(v, 4) is never materialised: row r of it is v[r], v[r + rows], v[r + 2 rows], v[r + 3 rows], which the hashing,
    // folding and gathering below read in place
    Tree pTree0 = commit_rows4(x, alg, lEval.p, N / 4, N > 256);                                      // :45-46

    // layers (:176-221), the recursion unrolled.  No root is read back inside it: the point every layer folds at,
    // prng(root of the tree above) (:194), is derived on the device from the root where it lies, so all layers
    // are enqueued without a round trip.  The launch that produces a tree's root also POSTS it to the host and derives that point
    // (gs_merkle_commit_rows_seed): the host picks each root up as soon as its tree exists and derives the layer's query positions and
    // batch-proof plans while the device folds the layers below
    double waited_ms = 0;          // host time blocked on roots that had not arrived yet (the device was the slower side)
    auto await_root = [&](Tree &t) {
        const auto w0 = std::chrono::steady_clock::now();
        x.check(A.gs_readback_wait(x.c, t.ticket, t.root.data()), "gs_readback_wait(root)");
        waited_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    };
    std::vector<Fold> layers = fri_layers(x, alg, omega, N, 1, lEval.p, N, pTree0.point.p);
    if (layers.size() > 60) fail(GS_ERR_ARG, "too many FRI components");
    clock.mark("FRI layers issued");
    clock.readme(x, "Computed low-degree proof: %zu FRI layers folded and committed", layers.size());
    // Everything the proof reads back — the queried rows and their batch proofs of every tree, the remainder (:179-187: the natural-
    // order vector the last polyValues came from) — is requested in ONE deferral window; the requests are planned root by root as
    // the roots arrive, the window closes with the single synchronisation of the proof
    std::vector<Component> components(layers.size());
    Readbacks rb;
    DeferWindow win(x);
    // spot checks of the evaluation tree (lib/Stark.ts:146-152, 274-296) and of the linear combination (LowDegreeProver.ts:52-54,
    // 302-309): positions from the root of the first FRI tree
    await_root(pTree0);
    const std::vector<uint64_t> exe_positions = plan.exe_positions(pTree0.root), lc_positions = augmented_rows(exe_positions, N);
    MerkleProof lcProof;
    rb.prove_batch(x, pTree0, lc_positions, &lcProof);
    rb.gather_rows4(x, lEval.p, N / 4, lc_positions, &lcProof);
    const std::vector<uint64_t> aug = plan.evaluation_positions(exe_positions);
    MerkleProof evProof;
    rb.prove_batch(x, eTree, aug, &evProof);
    // the leaves of the evaluation tree are the committed vectors' elements side by side (lib/Stark.ts:284-296)
    std::vector<MerkleProof> cols(V);
    for (uint32_t r = 0; r < V; r++) rb.gather(x, eVectors[r], ELEM, aug, 1, V == 1 ? &evProof : &cols[r]);
    // queries of every layer (:209-219): its column (4 * rows values in natural order: rows are read strided, never transposed) under the
    // tree above, the folded column under its own
    const Tree *pTree = &pTree0;
    const void *column = lEval.p;       // the current layer's values (the remainder at the end)
    uint64_t len = N;
    for (size_t d = 0; d < layers.size(); d++) {
        Fold &L = layers[d];
        const uint64_t rows = len / 4;
        await_root(L.cTree);
        if (d + 1 == layers.size()) clock.mark_split("waiting for FRI roots (device busy)", waited_ms, "query plans while the device folds");
        const Plan::Queries q = plan.layer_queries(L.cTree.root, rows);
        Component &c = components[d];
        c.columnRoot = L.cTree.root;
        rb.prove_batch(x, L.cTree, q.rows, &c.columnProof);
        rb.gather_rows4(x, L.next.p, rows / 4, q.rows, &c.columnProof);
        rb.prove_batch(x, *pTree, q.positions, &c.polyProof);
        rb.gather_rows4(x, column, rows, q.positions, &c.polyProof);
        pTree = &L.cTree;
        column = L.next.p;
        len = rows;
    }
    if (layers.empty()) clock.mark_split("waiting for FRI roots (device busy)", waited_ms, "query plans while the device folds");
    clock.mark("last root here: the last layer's plan");
    std::vector<F> remainder(len);
    Bytes remainder_raw(len * ELEM);
    {
        std::vector<uint64_t> all(len);
        for (uint64_t i = 0; i < len; i++) all[i] = i;
        x.check(A.gs_gather(x.c, column, ELEM, all.data(), len, remainder_raw.data()), "gs_gather(remainder)");
    }
    win.end();
    clock.mark("remainder + answers fetched (one sync)");
    for (uint64_t i = 0; i < len; i++) remainder[i] = load_elem(remainder_raw.data() + ELEM * i);
    check_remainder(plan, remainder, (uint32_t)layers.size());
    clock.mark("remainder checked");
    clock.readme(x, "Computed low-degree proof: query answers + Computed %zu evaluation spot checks (one read-back), remainder verified", exe_positions.size());
    if (V > 1) {
        evProof.value_size = (uint64_t)V * ELEM;
        evProof.nvalues = (uint32_t)aug.size();
        evProof.values.resize(aug.size() * V * ELEM);
        for (size_t i = 0; i < aug.size(); i++)
            for (uint32_t r = 0; r < V; r++) memcpy(evProof.values.data() + (i * V + r) * ELEM, cols[r].values.data() + i * ELEM, ELEM);
    }

    clock.mark("query answers unpacked");
    write_proof(out, eTree.root, evProof, V, pTree0.root, lcProof, components, remainder, input_shapes);
    clock.mark("serialized");
    clock.readme(x, "Proof serialized");
}

// ---- one proof across several GPUs (same helpers, same coefficient streams, same wire format)
#include "prover_dist.h"

// ---- Stark.verify(): the CPU-side half of the acceptance loop, native
#include "verifier.h"

// ---- why a statement does not prove: the same job, no proof (include/gstark_diagnose.h)
#include "diagnose.h"
