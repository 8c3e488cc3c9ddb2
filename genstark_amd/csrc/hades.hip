// hades.hip — Hades permutations (Poseidon hashes) and Poseidon Merkle trees (include/gstark_hades.h; examples/poseidon/utils.ts:19-49,
// 126-210 of the reference).  One thread runs one permutation with its state in registers; the width is a template argument (2 .. 8) so
// that every index into the state is a constant — rounds, alpha and the constants are run-time values.
//   constants   round constants ((rf + rp) x W) and the matrix (W x W) lie in ONE device block per parameter set (gs_hades_create) and
//               are read through `const fe *__restrict__` at indexes that do not depend on the lane: the compiler turns those reads
//               into scalar loads (through the scalar cache, into SGPRs), so the constants cost no VGPRs, no LDS and no barrier, and a
//               product by one of them is a product by a wave-uniform operand.  (Up to 568 elements: too many for kernel arguments.)
//   inputs      a workgroup's 256 rows pass through LDS both ways: the staged row kernel body of sponge_common.h.
//   tree        node i = digest(permute(node 2i || node 2i + 1)), heap layout.  A wide level IS a k_hades_hash launch over the level
//               below (the level loop of sponge_common.h) — there is no second copy of the kernel.  The levels of at most
//               GS_HADES_BLOCK nodes are one launch of one workgroup (k_hades_merkle_top): the level lives in LDS, a barrier
//               separates the levels.  Nothing here synchronises between workgroups.
//   updates,    gs_hades_merkle_update and gs_hades_sparse_create hand hades_node_hash — launch_hash over rows of two nodes — to the
//   sparse      drivers of field_tree.h, so an updated node is the node the tree build computes.
//   records     gs_hades_absorb (include/gstark_absorb.h): one thread absorbs one row of any length, a permutation per `rate` elements
//               (k_hades_absorb), the state in registers throughout; the row is read in place, by rows or by columns.
//   path roots  gs_hades_merkle_path_roots (tree_verify.h): one thread walks one path through all its levels in ONE launch
//               (k_hades_path_roots), the running node in registers; the sibling of a level is read straight from the path array.
#include "field_tree.h"
#include "tree_verify.h"
#include "../../include/gstark_hades.h"
#include "../../include/gstark_absorb.h"
#include "../../include/gstark_tree_update.h"
#include "../../include/gstark_tree_verify.h"
#include "../../include/gstark_sparse_tree.h"

#define GS_HADES_BLOCK 256

struct gs_hades {
    gs_ctx *ctx;
    uint32_t width, rf, rp;
    uint64_t alpha;
    fe *consts;              // device: (rf + rp) x width round constants, then width x width matrix rows
};

// s[FIRST .. W) to the power e (>= 1), the elements side by side (independent chains); the squarings and products fe_pow_u64 makes:
// none by one at the start, none after the top bit — x^5 is three products.  e is the same in every lane: scalar branches.
template <int W, int FIRST>
__device__ __forceinline__ void hades_sbox(fe (&s)[W], uint64_t e) {
    fe b[W];
#pragma unroll
    for (int j = FIRST; j < W; j++) b[j] = s[j];
#pragma unroll 1
    while (!(e & 1u)) {
#pragma unroll
        for (int j = FIRST; j < W; j++) b[j] = fe_mul(b[j], b[j]);
        e >>= 1;
    }
#pragma unroll
    for (int j = FIRST; j < W; j++) s[j] = b[j];
#pragma unroll 1
    for (e >>= 1; e; e >>= 1) {
#pragma unroll
        for (int j = FIRST; j < W; j++) b[j] = fe_mul(b[j], b[j]);
        if (e & 1u) {
#pragma unroll
            for (int j = FIRST; j < W; j++) s[j] = fe_mul(s[j], b[j]);
        }
    }
}

template <int W>
__device__ __forceinline__ void hades_permute(fe (&s)[W], const fe *__restrict__ consts, uint32_t rf, uint32_t rp, uint64_t alpha) {
    const uint32_t half = rf / 2, rounds = rf + rp;
    const fe *__restrict__ mds = consts + (uint64_t)rounds * W;
#pragma unroll 1
    for (uint32_t r = 0; r < rounds; r++) {
        const fe *__restrict__ ark = consts + (uint64_t)r * W;
#pragma unroll
        for (int j = 0; j < W; j++) s[j] = fe_add(s[j], ark[j]);
        if (r < half || r >= half + rp) hades_sbox<W, 0>(s, alpha);
        else hades_sbox<W, W - 1>(s, alpha);
        fe t[W];
#pragma unroll
        for (int i = 0; i < W; i++) {
            fe acc = fe_mul(mds[i * W], s[0]);
#pragma unroll
            for (int j = 1; j < W; j++) acc = fe_add(acc, fe_mul(mds[i * W + j], s[j]));
            t[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < W; i++) s[i] = t[i];
    }
}

// `count` permutations of rows of `arity` elements (1 <= arity < W), `digest` (1 or 2) elements out each; one workgroup per 256 rows
template <int W>
__global__ __launch_bounds__(GS_HADES_BLOCK) void k_hades_hash(const fe *__restrict__ in, uint64_t count, uint32_t arity, uint32_t digest,
                                                               const fe *__restrict__ consts, uint32_t rf, uint32_t rp, uint64_t alpha, fe *__restrict__ out) {
    GS_SPONGE_HASH_ROWS(GS_HADES_BLOCK, W, W - 1 > 2 ? W - 1 : 2, hades_permute<W>(s, consts, rf, rp, alpha));
}

// the top of a tree in one workgroup: reads nodes 2m .. 4m - 1 (m a power of two <= GS_HADES_BLOCK: the widest level computed here),
// writes nodes 1 .. 2m - 1 and the zero of node 0.  The level just computed stays in LDS for the next one.
template <int W>
__global__ __launch_bounds__(GS_HADES_BLOCK) void k_hades_merkle_top(fe *nodes,uint32_t m, uint32_t digest, const fe *__restrict__ consts,
                                                                     uint32_t rf, uint32_t rp, uint64_t alpha) {
    __shared__ fe level[2 * GS_HADES_BLOCK * 2];
    const uint32_t t = threadIdx.x;
    for (uint32_t k = t; k < 2 * m * digest; k += GS_HADES_BLOCK) level[k] = nodes[2 * m * digest + k];
    if (t < digest) nodes[t] = fe_zero();
    __syncthreads();
#pragma unroll 1
    for (uint32_t cnt = m; cnt >= 1; cnt >>= 1) {
        fe s[W];
        if (t < cnt) {
#pragma unroll
            for (int j = 0; j < W; j++) s[j] = j < 4 && j < (int)(2 * digest) ? level[t * 2 * digest + j] : fe_zero();
            hades_permute<W>(s, consts, rf, rp, alpha);
        }
        __syncthreads();                                                     // the level below has been read by everyone
        if (t < cnt) {
            level[t * digest] = s[0];
            nodes[(cnt + t) * digest] = s[0];
            if (digest > 1) { level[t * digest + 1] = s[1]; nodes[(cnt + t) * digest + 1] = s[1]; }
        }
        __syncthreads();
    }
}

// The root every path implies (tree_verify.h): thread k walks path k — paths[k] = the leaf, then `depth` siblings bottom-up, `digest`
// elements each — from leaves[k] when `leaves` is given, else from the path's own leaf.  On level l the state is (left, right, zeros),
// the running node on the right when bit l of idx[k] is 1, and the node above is the first `digest` elements of its permutation: what
// k_hades_hash computes for a row of a tree level.  No staging through LDS: a level costs one load of 16 .. 64 bytes per thread against
// the hundreds of field products of a permutation, a thread's siblings are consecutive in memory (the line one level fetches serves
// the next levels from the cache), and a workgroup's paths — 256 x 37 x 2 elements at the limits — do not fit the LDS at all.
// 2 * digest < W (the entry has checked it).
template <int W>
__global__ __launch_bounds__(GS_HADES_BLOCK) void k_hades_path_roots(const fe *__restrict__ paths, uint32_t depth, uint32_t digest, const uint64_t *__restrict__ idx,
                                                                     const fe *__restrict__ leaves, uint64_t count, const fe *__restrict__ consts, uint32_t rf,
                                                                     uint32_t rp, uint64_t alpha, fe *__restrict__ roots) {
    const uint64_t k = (uint64_t)blockIdx.x * GS_HADES_BLOCK + threadIdx.x;
    if (k >= count) return;                                                  // (nothing below crosses lanes)
    const fe *__restrict__ path = paths + k * (depth + 1) * digest;
    const fe *__restrict__ start = leaves ? leaves + k * digest : path;
    const uint64_t index = idx[k];
    fe v0 = start[0], v1 = digest > 1 ? start[1] : fe_zero();
#pragma unroll 1
    for (uint32_t l = 0; l < depth; l++) {
        const fe *__restrict__ sibling = path + (uint64_t)(l + 1) * digest;
        const fe u0 = sibling[0], u1 = digest > 1 ? sibling[1] : fe_zero();
        const bool right = (index >> l) & 1u;
        const fe a0 = right ? u0 : v0, a1 = right ? u1 : v1, b0 = right ? v0 : u0, b1 = right ? v1 : u1;      // left a, right b
        fe s[W];
#pragma unroll
        for (int j = 2; j < W; j++) s[j] = fe_zero();
        s[0] = a0;
        s[1] = digest > 1 ? a1 : b0;
        if constexpr (W > 4) {                                               // (nodes of two elements need a state of five)
            if (digest > 1) { s[2] = b0; s[3] = b1; }
        }
        hades_permute<W>(s, consts, rf, rp, alpha);
        v0 = s[0];
        v1 = s[1];
    }
    roots[k * digest] = v0;
    if (digest > 1) roots[k * digest + 1] = v1;
}

// Records of any length (include/gstark_absorb.h): thread k absorbs row k, `rate` elements per permutation, the state in registers from
// the first block to the digest.  state[rate] starts as the length; every index into the state is a constant (the comparisons with
// `rate` are the same in every lane).  Element i of the row is read at row[i * elem_stride] straight from memory, as k_hades_path_roots
// reads its siblings: a block is 16 .. 224 bytes per thread against the hundreds to thousands of products of its permutation.  In the
// columns layout (row_stride 1) consecutive lanes read consecutive elements; in the rows layout a thread's elements are consecutive
// and the line one block fetches serves the next blocks from the cache.  The next block is NOT loaded ahead of the permutation: the
// state and the S-box temporaries already set the register count.  A grid-stride loop: the grid is capped, nothing crosses lanes.
template <int W>
__global__ __launch_bounds__(GS_HADES_BLOCK) void k_hades_absorb(const fe *__restrict__ in, uint64_t count, uint32_t length, uint64_t row_stride, uint64_t elem_stride,
                                                                 uint32_t rate, uint32_t digest, const fe *__restrict__ consts, uint32_t rf, uint32_t rp, uint64_t alpha,
                                                                 fe *__restrict__ out) {
#pragma unroll 1
    for (uint64_t k = (uint64_t)blockIdx.x * GS_HADES_BLOCK + threadIdx.x; k < count; k += (uint64_t)gridDim.x * GS_HADES_BLOCK) {
        const fe *__restrict__ row = in + k * row_stride;
        fe s[W];
#pragma unroll
        for (int j = 0; j < W; j++) s[j] = j == (int)rate ? fe_make(length, 0, 0, 0) : fe_zero();
#pragma unroll 1
        for (uint32_t first = 0; first < length; first += rate) {
#pragma unroll
            for (int j = 0; j < W - 1; j++)
                if (j < (int)rate && first + j < length) s[j] = fe_add(s[j], row[(uint64_t)(first + j) * elem_stride]);
            hades_permute<W>(s, consts, rf, rp, alpha);
        }
        out[k * digest] = s[0];
        if (digest > 1) out[k * digest + 1] = s[1];
    }
}

namespace {

#define GS_HADES_ABSORB_GRID (1u << 22)      // workgroups of k_hades_absorb at most: 2^30 threads, the rows beyond them by the stride loop

int launch_absorb(gs_ctx *c, const gs_hades *h, const fe *in, uint64_t count, uint32_t length, uint64_t row_stride, uint64_t elem_stride, uint32_t rate, uint32_t digest,
                  fe *out) {
    uint64_t blocks = (count + GS_HADES_BLOCK - 1) / GS_HADES_BLOCK;
    if (blocks > GS_HADES_ABSORB_GRID) blocks = GS_HADES_ABSORB_GRID;
    switch (h->width) {
#define X(W)                                                                                                                                         \
    case W:                                                                                                                                          \
        hipLaunchKernelGGL(k_hades_absorb<W>, dim3((unsigned)blocks), dim3(GS_HADES_BLOCK), 0, c->stream, in, count, length, row_stride, elem_stride, rate, digest, \
                           (const fe *)h->consts, h->rf, h->rp, h->alpha, out);                                                                      \
        break;
        GS_SPONGE_WIDTHS(X)
#undef X
    }
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int launch_hash(gs_ctx *c, const gs_hades *h, const fe *in, uint64_t count, uint32_t arity, uint32_t digest, fe *out) {
    const uint64_t blocks = (count + GS_HADES_BLOCK - 1) / GS_HADES_BLOCK;
    switch (h->width) {
#define X(W)                                                                                                                                         \
    case W:                                                                                                                                          \
        hipLaunchKernelGGL(k_hades_hash<W>, dim3((unsigned)blocks), dim3(GS_HADES_BLOCK), 0, c->stream, in, count, arity, digest, (const fe *)h->consts, \
                           h->rf, h->rp, h->alpha, out);                                                                                             \
        break;
        GS_SPONGE_WIDTHS(X)
#undef X
    }
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int launch_top(gs_ctx *c, const gs_hades *h, fe *nodes, uint32_t m, uint32_t digest) {
    switch (h->width) {
#define X(W)                                                                                                                                             \
    case W:                                                                                                                                              \
        hipLaunchKernelGGL(k_hades_merkle_top<(W < 3 ? 3 : W)>, dim3(1), dim3(GS_HADES_BLOCK), 0, c->stream, nodes, m, digest, (const fe *)h->consts, h->rf, \
                           h->rp, h->alpha);                                                                                                             \
        break;
        GS_SPONGE_WIDTHS(X)                                                   // (a tree needs 2 * digest < width: width 2 never gets here)
#undef X
    }
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int launch_path_roots(gs_ctx *c, const gs_hades *h, const fe *paths, uint32_t depth, uint32_t digest, const uint64_t *idx, const fe *leaves, uint64_t count, fe *roots) {
    const uint64_t blocks = (count + GS_HADES_BLOCK - 1) / GS_HADES_BLOCK;
    switch (h->width) {
#define X(W)                                                                                                                                             \
    case W:                                                                                                                                              \
        hipLaunchKernelGGL(k_hades_path_roots<(W < 3 ? 3 : W)>, dim3((unsigned)blocks), dim3(GS_HADES_BLOCK), 0, c->stream, paths, depth, digest, idx, leaves, count, \
                           (const fe *)h->consts, h->rf, h->rp, h->alpha, roots);                                                                        \
        break;
        GS_SPONGE_WIDTHS(X)                                                   // (2 * digest < width: width 2 never gets here)
#undef X
    }
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

// products of one permutation: the S-boxes of rf full and rp partial rounds and the matrix of every round
uint64_t hades_products(const gs_hades *h) {
    const uint64_t w = h->width, per_pow = sponge_pow_products(h->alpha);
    return h->rf * (w * per_pow + w * w) + h->rp * (per_pow + w * w);
}

// the tree_node_hash of this unit (field_tree.h): `count` rows of two nodes into `count` nodes, as a wide level of the tree build
int hades_node_hash(gs_ctx *c, const void *handle, uint32_t digest, const fe *rows, uint64_t count, fe *out) {
    const gs_hades *h = (const gs_hades *)handle;
    gs_traffic(c, 3 * count * digest * GS_ELT, count * hades_products(h), "k_hades_hash<%u>", h->width);
    return launch_hash(c, h, rows, count, 2 * digest, digest, out);
}

// a tree's nodes have 1 or 2 elements, and two of them enter one permutation beside its capacity
int hades_check_nodes(gs_ctx *c, const gs_hades *h, const char *who, uint32_t digest) {
    if (digest >= 1 && digest <= 2 && 2 * digest < h->width) return GS_OK;
    return gs_fail(c, GS_ERR_ARG, "%s: nodes of %u elements (1 or 2): two of them do not fit a state of %u beside its capacity", who, digest, h->width);
}

}  // namespace

extern "C" {

uint32_t gs_hades_merkle_top(void) { return GS_HADES_BLOCK; }

int gs_hades_create(gs_ctx *c, uint32_t width, uint32_t rf, uint32_t rp, uint64_t alpha, const uint8_t *rc_host, const uint8_t *mds_host, gs_hades **out) {
    if (!c || !out) return GS_ERR_ARG;
    *out = nullptr;
    if (!rc_host || !mds_host) return gs_fail(c, GS_ERR_ARG, "hades_create: round constants and matrix are required");
    if (width < 2 || width > 8) return gs_fail(c, GS_ERR_ARG, "hades_create: width %u is outside 2 .. 8", width);
    if (rf < 2 || (rf & 1u) || rf > (1u << 16) || rp > (1u << 16))
        return gs_fail(c, GS_ERR_ARG, "hades_create: %u full rounds (even, 2 .. 65536) and %u partial rounds (at most 65536)", rf, rp);
    if (alpha < 2) return gs_fail(c, GS_ERR_ARG, "hades_create: alpha is at least 2");
    const uint64_t nrc = (uint64_t)(rf + rp) * width, nmds = (uint64_t)width * width;
    void *p = nullptr;
    const int rc = sponge_upload(c, {{rc_host, nrc * GS_ELT}, {mds_host, nmds * GS_ELT}}, &p);
    if (rc) return rc;
    *out = new gs_hades{c, width, rf, rp, alpha, (fe *)p};
    sponge_register(*out);
    return GS_OK;
}

int gs_hades_destroy(gs_ctx *c, gs_hades *h) { return sponge_destroy(c, h, "hades_destroy"); }

int gs_hades_hash(gs_ctx *c, const gs_hades *h, const void *in, uint64_t count, uint32_t arity, uint32_t digest, void *out) {
    int rc;
    if ((rc = sponge_check_handle(c, h, "hades_hash")) || (rc = sponge_check_rows(c, "hades_hash", arity, h->width - 1, h->width, digest)) ||
        (rc = sponge_check_count(c, "hades_hash", count)))
        return rc;
    if (!count) return GS_OK;
    if (!in || !out) return GS_ERR_ARG;
    gs_traffic(c, count * (arity + digest) * GS_ELT, count * hades_products(h), "k_hades_hash<%u>", h->width);
    return launch_hash(c, h, (const fe *)in, count, arity, digest, (fe *)out);
}

int gs_hades_absorb(gs_ctx *c, const gs_hades *h, const void *in, uint64_t count, uint32_t length, uint64_t row_stride, uint64_t elem_stride, uint32_t rate, uint32_t digest,
                    void *out) {
    int rc;
    uint64_t blocks = 0;
    if ((rc = sponge_check_handle(c, h, "hades_absorb")) ||
        (rc = sponge_check_absorb(c, "hades_absorb", h->width, count, length, row_stride, elem_stride, rate, digest, in, out, &blocks)) || !count)
        return rc;
    gs_traffic(c, count * (length + digest) * GS_ELT, count * blocks * hades_products(h), "k_hades_absorb<%u>", h->width);
    return launch_absorb(c, h, (const fe *)in, count, length, row_stride, elem_stride, rate, digest, (fe *)out);
}

int gs_hades_merkle(gs_ctx *c, const gs_hades *h, const void *leaves, uint64_t n, uint32_t digest, void *nodes_out) {
    int rc;
    if ((rc = sponge_check_handle(c, h, "hades_merkle")) || (rc = sponge_check_leaves(c, "hades_merkle", n)) || (rc = hades_check_nodes(c, h, "hades_merkle", digest))) return rc;
    if (!leaves || !nodes_out) return GS_ERR_ARG;
    fe *nodes = (fe *)nodes_out;
    if (leaves != (const void *)(nodes + n * digest))
        GS_HIP(c, hipMemcpyAsync(nodes + n * digest, leaves, n * digest * GS_ELT, hipMemcpyDeviceToDevice, c->stream));
    uint64_t cnt;
    rc = sponge_tree_levels(nodes, n, digest, GS_HADES_BLOCK, &cnt, [&](const fe *below, uint64_t count, fe *level) {      // hades_node_hash under the build's own label
        gs_traffic(c, 3 * count * digest * GS_ELT, count * hades_products(h), "k_hades_merkle_level<%u>", h->width);
        return launch_hash(c, h, below, count, 2 * digest, digest, level);
    });
    if (rc) return rc;
    gs_traffic(c, (4 * cnt - 1) * digest * GS_ELT, (2 * cnt - 1) * hades_products(h), "k_hades_merkle_top<%u>", h->width);
    return launch_top(c, h, nodes, (uint32_t)cnt, digest);
}

int gs_hades_merkle_update(gs_ctx *c, const gs_hades *h, void *nodes, uint64_t n, uint32_t digest, const uint64_t *indexes_host, const void *leaves, uint64_t count,
                           void *before_out, void *roots_out) {
    int rc;
    if ((rc = sponge_check_handle(c, h, "hades_merkle_update")) || (rc = hades_check_nodes(c, h, "hades_merkle_update", digest))) return rc;
    if ((rc = tree_update_check(c, "hades_merkle_update", n, count, indexes_host, nodes, leaves, before_out, roots_out)) || !count) return rc;
    return tree_update_run(c, (fe *)nodes, n, digest, indexes_host, (const fe *)leaves, count, (fe *)before_out, (fe *)roots_out, {hades_node_hash, h});
}

int gs_hades_sparse_create(gs_ctx *c, const gs_hades *h, uint32_t depth, uint32_t digest, const void *empty_leaf_host, uint64_t slots_hint, gs_sparse **tree) {
    int rc;
    if (c && h && !sponge_serial(h)) return gs_fail(c, GS_ERR_ARG, "hades_sparse_create: the hash has been destroyed");
    if ((rc = sponge_check_handle(c, h, "hades_sparse_create")) || (rc = hades_check_nodes(c, h, "hades_sparse_create", digest))) return rc;
    return sparse_tree_create(c, "hades_sparse_create", {hades_node_hash, h}, depth, digest, empty_leaf_host, slots_hint, tree);
}

int gs_hades_merkle_path_roots(gs_ctx *c, const gs_hades *h, const void *paths, uint32_t depth, uint32_t digest, const uint64_t *indexes_host, const void *leaves,
                               uint64_t count, void *roots_out) {
    int rc;
    if ((rc = sponge_check_handle(c, h, "hades_merkle_path_roots")) || (rc = hades_check_nodes(c, h, "hades_merkle_path_roots", digest))) return rc;
    if ((rc = tree_verify_check(c, "hades_merkle_path_roots", depth, count, indexes_host, paths, roots_out)) || !count) return rc;
    return tree_verify_run(c, indexes_host, count, [&](const uint64_t *idx) {
        gs_traffic(c, tree_verify_bytes(depth, digest, leaves != nullptr, count), count * depth * hades_products(h), "k_hades_path_roots<%u>", h->width);
        return launch_path_roots(c, h, (const fe *)paths, depth, digest, idx, (const fe *)leaves, count, (fe *)roots_out);
    });
}

}  // extern "C"
