// sponge_common.h — what the algebraic hash units (hades.hip, rescue.hip) share: everything around a permutation.  A unit brings its
// permutation, its parameter handle `H` (members `ctx` and `consts`, its one device block) and its launches.
//   rows    a workgroup's BLOCK rows of `arity` elements are one contiguous run of memory: it is copied into LDS with consecutive lanes
//           on consecutive elements, then every thread picks its row up from there; the digests leave the same way (GS_SPONGE_HASH_ROWS).
//   tree    heap layout: the inputs of ALL nodes of one level are the level below, contiguous, in rows of 2 * digest elements — a level
//           IS a hash launch (sponge_tree_levels).  What reads and writes nodes and knows no permutation is field_tree.hip.
// Every message starts with the caller's name (`who`): the texts are those of the entry points.
#pragma once
#include "common.h"

#include <initializer_list>
#include <mutex>
#include <unordered_map>

#define GS_SPONGE_WIDTHS(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8)        // the state widths a unit instantiates: switch (width) { GS_SPONGE_WIDTHS(X) }

// The body of a k_*_hash<W> kernel of BLOCK threads with the parameters `in`, `count`, `arity`, `digest` (1 or 2) and `out`: `count` rows of
// `arity` elements in, `digest` elements out each, one workgroup per BLOCK rows.  PERMUTE is the call that permutes the state `fe s[W]`;
// its constants are read at lane-independent indexes.  STAGE: elements of LDS per row (the widest arity the unit admits, at least 2 for
// the digests).  A macro and no function: the permutation is inlined straight into the __global__ function, which compiles to what it
// compiled to with the body written out in it (profiles/sponge_shared.md).
#define GS_SPONGE_HASH_ROWS(BLOCK, W, STAGE, PERMUTE)                                                                                \
    __shared__ fe stage[(BLOCK) * (STAGE)];                                    /* rows x arity in, then rows x digest out */         \
    const uint32_t t = threadIdx.x;                                                                                                  \
    const uint64_t first = (uint64_t)blockIdx.x * (BLOCK);                                                                           \
    const uint32_t rows = count - first < (BLOCK) ? (uint32_t)(count - first) : (BLOCK);                                             \
    const fe *__restrict__ src = in + first * arity;                                                                                 \
    for (uint32_t k = t; k < rows * arity; k += (BLOCK)) stage[k] = src[k];                                                          \
    __syncthreads();                                                                                                                 \
    fe s[W];                                                                                                                         \
    if (t < rows) {                                                                                                                  \
        _Pragma("unroll") for (int j = 0; j < W; j++) s[j] = j < (int)arity ? stage[t * arity + j] : fe_zero();                      \
        PERMUTE;                                                                                                                     \
    }                                                                                                                                \
    __syncthreads();                                                         /* every row has been picked up: the stage takes the digests */ \
    if (t < rows) {                                                                                                                  \
        stage[t * digest] = s[0];                                                                                                    \
        if (digest > 1) stage[t * digest + 1] = s[1];                                                                                \
    }                                                                                                                                \
    __syncthreads();                                                                                                                 \
    fe *__restrict__ dst = out + first * digest;                                                                                     \
    for (uint32_t k = t; k < rows * digest; k += (BLOCK)) dst[k] = stage[k]

template <class H>
static inline int sponge_check_handle(gs_ctx *c, const H *h, const char *who) {
    if (!c || !h) return GS_ERR_ARG;
    return h->ctx == c ? GS_OK : gs_fail(c, GS_ERR_ARG, "%s: the handle belongs to another context", who);
}

// a hash launch: rows of 1 .. max_arity inputs into a state of `width`, 1 or 2 elements out; `count` of them (a check of its own: a
// unit has checks of its own arguments to make between the two)
static inline int sponge_check_rows(gs_ctx *c, const char *who, uint32_t arity, uint32_t max_arity, uint32_t width, uint32_t digest) {
    if (arity < 1 || arity > max_arity) return gs_fail(c, GS_ERR_ARG, "%s: %u inputs do not fit a state of %u (1 .. %u)", who, arity, width, max_arity);
    return digest >= 1 && digest <= 2 ? GS_OK : gs_fail(c, GS_ERR_ARG, "%s: a digest of 1 or 2 elements, not %u", who, digest);
}
static inline int sponge_check_count(gs_ctx *c, const char *who, uint64_t count) {
    return count <= (1ull << 36) ? GS_OK : gs_fail(c, GS_ERR_ARG, "%s: at most 2^36 permutations per call", who);
}

// An absorb launch (include/gstark_absorb.h): `count` rows of `length` elements at in[k * row_stride + i * elem_stride], `rate` of them
// per permutation of a state of `width`, `digest` elements out each.  Every refusal has a message of its own; -> *blocks: the
// permutations of one row.  The caller has checked its handle, and returns GS_OK itself when count is 0 (nothing below looks at the
// pointers of an empty call).
#define GS_ABSORB_MAX_LENGTH (1u << 16)
static inline int sponge_check_absorb(gs_ctx *c, const char *who, uint32_t width, uint64_t count, uint32_t length, uint64_t row_stride, uint64_t elem_stride, uint32_t rate,
                                      uint32_t digest, const void *in, const void *out, uint64_t *blocks) {
    if (rate < 1 || rate >= width) return gs_fail(c, GS_ERR_ARG, "%s: a rate of %u does not leave a capacity in a state of %u (1 .. %u)", who, rate, width, width - 1);
    if (digest < 1 || digest > 2 || digest > rate) return gs_fail(c, GS_ERR_ARG, "%s: a digest of 1 or 2 elements and at most the rate (%u), not %u", who, rate, digest);
    if (length < 1 || length > GS_ABSORB_MAX_LENGTH) return gs_fail(c, GS_ERR_ARG, "%s: a row of %u elements (1 .. 65536)", who, length);
    if (fe_ge_p(fe_from_u64(length))) return gs_fail(c, GS_ERR_ARG, "%s: a row of %u elements: the length is below the modulus", who, length);
    const bool by_rows = elem_stride == 1 && row_stride >= length, by_columns = row_stride == 1 && elem_stride >= count;
    if (!by_rows && !by_columns)
        return gs_fail(c, GS_ERR_ARG, "%s: strides (%llu, %llu) are neither rows (elem_stride 1, row_stride >= length) nor columns (row_stride 1, elem_stride >= count)", who,
                       (unsigned long long)row_stride, (unsigned long long)elem_stride);
    *blocks = (length + rate - 1) / rate;
    if (count > (1ull << 36) / *blocks) return gs_fail(c, GS_ERR_ARG, "%s: at most 2^36 permutations per call", who);
    if (!count) return GS_OK;
    if (!in || !out) return gs_fail(c, GS_ERR_ARG, "%s: in and out are required", who);
    const unsigned __int128 read = ((unsigned __int128)(count - 1) * row_stride + (unsigned __int128)(length - 1) * elem_stride + 1) * GS_ELT;
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    if (b < a + read && a < b + count * digest * GS_ELT) return gs_fail(c, GS_ERR_ARG, "%s: out overlaps in", who);
    return GS_OK;
}

static inline int sponge_check_leaves(gs_ctx *c, const char *who, uint64_t n) {
    return n >= 2 && gs_is_pow2(n) && n <= (1ull << 36) ? GS_OK : gs_fail(c, GS_ERR_ARG, "%s: the number of leaves is a power of two, 2 .. 2^36", who);
}

// products of one x^alpha: the squarings and products fe_pow_u64 makes — none by one at the start, none after the top bit
static inline uint64_t sponge_pow_products(uint64_t alpha) {
    uint64_t n = 0;
    for (uint64_t e = alpha; e > 1; e >>= 1) n += 1 + (e & 1u);
    return n;
}

// the constants of a parameter set: ONE device block that holds the host parts one after the other
struct sponge_part { const void *host; uint64_t bytes; };
static inline int sponge_upload(gs_ctx *c, std::initializer_list<sponge_part> parts, void **out) {
    uint64_t total = 0, at = 0;
    for (const sponge_part &part : parts) total += part.bytes;
    int rc = gs_alloc(c, total, out);
    for (const sponge_part &part : parts) {
        if (!rc) rc = gs_push(c, (uint8_t *)*out + at, part.host, part.bytes);
        at += part.bytes;
    }
    if (rc && *out) gs_free(c, *out);
    return rc;
}

// A host array that one launch reads: up through the stream-ordered scratch, launch(its device copy), and the scratch goes back at
// once — the cache is stream-ordered, so the launch still reads it.
template <class Launch>
static inline int sponge_with_upload(gs_ctx *c, const void *host, uint64_t bytes, Launch launch) {
    void *dev = nullptr;
    int rc = gs_tmp_alloc(c, bytes, &dev);
    if (rc) return rc;
    if ((rc = gs_push(c, dev, host, bytes)) == GS_OK) rc = launch((const void *)dev);
    gs_tmp_free(c, dev);
    return rc;
}

// The live parameter handles of both units, each with the serial number it was created under: what outlives a handle and keeps its
// pointer (a sparse tree, field_tree.h) asks here before it dereferences it, so a destroyed hash is an error code and not a read of
// freed memory.  One registry per library: a function-local static of an inline function.
struct sponge_registry {
    std::mutex mutex;
    std::unordered_map<const void *, uint64_t> live;
    uint64_t next = 1;
};
inline sponge_registry &sponge_handles() {
    static sponge_registry registry;
    return registry;
}
static inline uint64_t sponge_register(const void *h) {
    sponge_registry &r = sponge_handles();
    std::lock_guard<std::mutex> lock(r.mutex);
    return r.live[h] = r.next++;
}
static inline void sponge_unregister(const void *h) {
    sponge_registry &r = sponge_handles();
    std::lock_guard<std::mutex> lock(r.mutex);
    r.live.erase(h);
}
// the serial of a live handle; 0: never created, or destroyed
static inline uint64_t sponge_serial(const void *h) {
    sponge_registry &r = sponge_handles();
    std::lock_guard<std::mutex> lock(r.mutex);
    const auto it = r.live.find(h);
    return it == r.live.end() ? 0 : it->second;
}

template <class H>
static inline int sponge_destroy(gs_ctx *c, H *h, const char *who) {
    if (!c || !h) return c ? GS_OK : GS_ERR_ARG;
    const int rc = sponge_check_handle(c, h, who);
    if (rc) return rc;
    sponge_unregister(h);
    gs_free(c, h->consts);                                                   // parked in the context's cache: launches already queued still read it in order
    delete h;
    return GS_OK;
}

// The levels of more than `top` nodes, from the widest down: level(below, cnt, here) hashes the cnt rows of 2 * digest elements at
// `below` into the cnt nodes at `here`; the stream orders the launches.  -> *rest: the nodes of the first level left to the caller
template <class Level>
static inline int sponge_tree_levels(fe *nodes, uint64_t n, uint32_t digest, uint64_t top, uint64_t *rest, Level level) {
    int rc = GS_OK;
    for (*rest = n / 2; *rest > top && !rc; *rest /= 2) rc = level((const fe *)(nodes + 2 * *rest * digest), *rest, nodes + *rest * digest);
    return rc;
}
