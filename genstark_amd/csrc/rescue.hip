// rescue.hip — Rescue permutations and Rescue Merkle trees (include/gstark_rescue.h; examples/rescue/utils.ts:19-124, 232-273 of the
// reference).  The width is a template argument so that the state stays in registers; rounds, both exponents and the constants are
// run-time values.
//   constants   keys ((2 rounds + 3) x W), the matrix (W x W) and the exponent schedule lie in ONE device block per parameter set
//               (gs_rescue_create).  Form 1 reads them at indexes that do not depend on the lane (scalar loads, as in hades.hip).
//   inverse     x^inv_exponent is almost all of the cost: the exponent has as many bits as the field.  gs_rescue_create turns it into a
//   S-box       left-to-right sliding-window schedule once, on the host: word 0 names the odd power the chain starts from, every later
//               word is (squarings << 8 | table index), index 0xff = no product.  The table holds x^1, x^3, .. x^(2 size - 1) (one
//               squaring and size - 1 products); the window (1 .. 4 bits) is the one with the fewest products in all.  Every branch of
//               the chain depends on the schedule alone: the same in every lane.  In the 128-bit flavour the chain runs on lazy
//               five-limb values (gf128_lazy.h: lz_unpack once, lz_sqr / lz_mul_v, lz_pack once); every other flavour uses fe_mul.
//   form 1      one thread per permutation (k_rescue_hash<W>): a workgroup's rows pass through LDS both ways (the staged row kernel
//               body of sponge_common.h).  The W chains of a state run one after the other through ONE copy of the chain: the
//               state is rotated by one element per pass, so every index into it is a constant.
//   form 2      one lane per state element (k_rescue_spread<G>): a permutation is an aligned group of G = 2, 4 or 8 lanes (the width
//               rounded up; surplus lanes carry zeros), every lane runs ONE chain, and for the matrix step a lane fetches the group's
//               elements with cross-lane reads and computes its own row.  A permutation's latency is one chain per half round instead of
//               W: this is the form of narrow launches, where the machine is empty and latency is all there is.
//   tree        node i = element 0 of modifiedSponge(node 2i, node 2i + 1), heap layout: every level is one hash launch over the level
//               below, ordered by the stream (the level loop of sponge_common.h, down to the root).  Workgroups are one wave in both forms, so a narrow level spreads over many CUs.
//               Nothing here synchronises between workgroups.
//   updates,    gs_rescue_merkle_update and gs_rescue_sparse_create hand rescue_node_hash — what a level of the tree build runs:
//   sparse      launch_hash with the form pick_form chooses — to the drivers of field_tree.h: an updated node is the node the build computes.
//   records     gs_rescue_absorb (include/gstark_absorb.h): a row of any length, a permutation per `rate` elements, in form 2 only
//               (k_rescue_absorb<G>: a group of G lanes per row, the state in the lanes' registers from the first block to the digest).
//   path roots  gs_rescue_merkle_path_roots (tree_verify.h): a path is a dependent chain of permutations, so it is walked in form 2
//               only (k_rescue_path_roots<G>: a group of G lanes per path, every level in ONE launch); the entry's cap is form 2's limit.
#include "field_tree.h"
#include "tree_verify.h"
#include "../../include/gstark_rescue.h"
#include "../../include/gstark_absorb.h"
#include "../../include/gstark_tree_update.h"
#include "../../include/gstark_sparse_tree.h"
#include "../../include/gstark_tree_verify.h"
#if defined(GS_FIELD_128)
#include "gf128_lazy.h"
#endif

#define GS_RESCUE_BLOCK 64
#define GS_RESCUE_TABLE 8                    // odd powers x^1 .. x^15: a window of at most 4 bits
#define GS_RESCUE_NO_PRODUCT 0xffu
#define GS_RESCUE_SPREAD_LIMIT (1ull << 20)  // form 0: form 2 up to this many permutations — measured: form 2 is the faster one at every
                                             // count from 1 to 2^20 (by 4x up to 2^14, by 2 % at 2^20), no crossover found (profiles/rescue.md)
#define GS_RESCUE_SPREAD_MAX (1ull << 24)    // form 2: the grid is count * G / 64 workgroups
static_assert(GS_TREE_VERIFY_MAX <= GS_RESCUE_SPREAD_LIMIT, "the path walk exists in form 2 only: its cap is the count up to which form 2 is the faster one");

struct gs_rescue {
    gs_ctx *ctx;
    uint32_t width, rounds;
    uint64_t alpha;
    uint32_t nops, table;                    // words of the schedule, entries of the table of odd powers
    uint64_t inv_products, alpha_products;   // squarings + products of one S-box of either kind
    fe *consts;                              // device: keys, matrix rows, then the schedule (uint32 words)
    const uint32_t *sched;                   // = (uint32_t *)(consts + (2 rounds + 3 + width) * width)
};

// the values a chain of squarings and products runs on
struct rescue_chain_fe {
    typedef fe T;
    static __device__ __forceinline__ T from(const fe &x) { return x; }
    static __device__ __forceinline__ fe to(const T &x) { return x; }
    static __device__ __forceinline__ T sqr(const T &x) { return fe_mul(x, x); }
    static __device__ __forceinline__ T mul(const T &x, const T &y) { return fe_mul(x, y); }
};
#if defined(GS_FIELD_128) && !defined(GS_RESCUE_CANONICAL_CHAIN)
struct rescue_chain_lz {                     // near-normalised lazy values in, near-normalised out: the chain never leaves the form
    typedef lz T;
    static __device__ __forceinline__ T from(const fe &x) { return lz_unpack(x); }
    static __device__ __forceinline__ fe to(const T &x) { return lz_pack(x); }
    static __device__ __forceinline__ T sqr(const T &x) { return lz_sqr(x, lzk_make()); }
    static __device__ __forceinline__ T mul(const T &x, const T &y) { return lz_mul_v(x, y, lzk_make()); }
};
typedef rescue_chain_lz rescue_chain;
#else
typedef rescue_chain_fe rescue_chain;
#endif

template <class C>
__device__ __forceinline__ typename C::T rescue_pick(const typename C::T (&t)[GS_RESCUE_TABLE], uint32_t k) {
    switch (k) {                             // k is the same in every lane
    case 1: return t[1];
    case 2: return t[2];
    case 3: return t[3];
    case 4: return t[4];
    case 5: return t[5];
    case 6: return t[6];
    case 7: return t[7];
    default: return t[0];
    }
}

// x^inv_exponent by the schedule of gs_rescue_create (0 -> 0: the chain starts from a power of x and only squares and multiplies)
template <class C>
__device__ __forceinline__ fe rescue_inv_sbox(const fe &x, const uint32_t *__restrict__ sched, uint32_t nops, uint32_t table) {
    typename C::T t[GS_RESCUE_TABLE];
    t[0] = C::from(x);
#pragma unroll
    for (int i = 1; i < GS_RESCUE_TABLE; i++) t[i] = t[0];
    if (table > 1) {
        const typename C::T x2 = C::sqr(t[0]);
#pragma unroll
        for (int i = 1; i < GS_RESCUE_TABLE; i++)
            if (i < (int)table) t[i] = C::mul(t[i - 1], x2);
    }
    typename C::T acc = rescue_pick<C>(t, sched[0] & 0xffu);
#pragma unroll 1
    for (uint32_t op = 1; op < nops; op++) {
        const uint32_t u = sched[op];
#pragma unroll 1
        for (uint32_t q = u >> 8; q; q--) acc = C::sqr(acc);
        if ((u & 0xffu) != GS_RESCUE_NO_PRODUCT) acc = C::mul(acc, rescue_pick<C>(t, u & 0xffu));
    }
    return C::to(acc);
}

// half rounds of one sponge: how many, the first key row, and whether the first one is the inverse S-box
__device__ __forceinline__ void rescue_shape(uint32_t rounds, uint32_t modified, uint32_t &halves, uint32_t &key, uint32_t &inverse) {
    halves = modified ? 2 * (rounds - 1) : 2 * rounds;
    key = modified ? 2 : 1;
    inverse = modified ? 0 : 1;
}

template <int W>
__device__ __forceinline__ void rescue_permute(fe (&s)[W], const fe *__restrict__ consts, uint32_t rounds, uint32_t modified, uint64_t alpha,
                                               const uint32_t *__restrict__ sched, uint32_t nops, uint32_t table) {
    const fe *__restrict__ mds = consts + (uint64_t)(2 * rounds + 3) * W;
    uint32_t halves, key, inverse;
    rescue_shape(rounds, modified, halves, key, inverse);
    if (!modified) {
#pragma unroll
        for (int j = 0; j < W; j++) s[j] = fe_add(s[j], consts[j]);
    }
#pragma unroll 1
    for (uint32_t h = 0; h < halves; h++, key++, inverse ^= 1u) {
#pragma unroll 1
        for (int pass = 0; pass < W; pass++) {                              // one chain at a time; the state turns by one element
            const fe y = inverse ? rescue_inv_sbox<rescue_chain>(s[0], sched, nops, table) : fe_pow_u64(s[0], alpha);
#pragma unroll
            for (int j = 0; j + 1 < W; j++) s[j] = s[j + 1];
            s[W - 1] = y;
        }
        const fe *__restrict__ k = consts + (uint64_t)key * W;
        fe t[W];
#pragma unroll
        for (int i = 0; i < W; i++) t[i] = s[i];
#pragma unroll 1
        for (int i = 0; i < W; i++) {                                       // row i lands in t[W - 1]; t turns like the state
            const fe *__restrict__ row = mds + i * W;
            fe acc = fe_mul(row[0], s[0]);
#pragma unroll
            for (int j = 1; j < W; j++) acc = fe_add(acc, fe_mul(row[j], s[j]));
            acc = fe_add(acc, k[i]);
#pragma unroll
            for (int j = 0; j + 1 < W; j++) t[j] = t[j + 1];
            t[W - 1] = acc;
        }
#pragma unroll
        for (int i = 0; i < W; i++) s[i] = t[i];
    }
}

// form 1: `count` permutations of rows of `arity` elements (1 <= arity <= W), `digest` (1 or 2) elements out each; one workgroup (one
// wave) per 64 rows
template <int W>
__global__ __launch_bounds__(GS_RESCUE_BLOCK) void k_rescue_hash(const fe *__restrict__ in, uint64_t count, uint32_t arity, uint32_t digest, uint32_t modified,
                                                                 const fe *__restrict__ consts, uint32_t rounds, uint64_t alpha,
                                                                 const uint32_t *__restrict__ sched, uint32_t nops, uint32_t table, fe *__restrict__ out) {
    GS_SPONGE_HASH_ROWS(GS_RESCUE_BLOCK, W, W, rescue_permute<W>(s, consts, rounds, modified, alpha, sched, nops, table));
}

__device__ __forceinline__ fe rescue_lane_read(const fe &a, int lane) {
    fe r;
#pragma unroll
    for (int i = 0; i < GF_LIMBS; i++) fe_set_limb(r, i, (uint32_t)__shfl((int)fe_limb(a, i), lane, 64));
    return r;
}

// form 2: lane j of an aligned group of G lanes holds element j of one permutation (j >= width: a zero that nothing reads with a
// non-zero coefficient); 64 / G permutations per workgroup.  Every lane stays active to the end — the cross-lane reads need the
// whole wave —, only the loads and stores are guarded.
template <int G>
__global__ __launch_bounds__(GS_RESCUE_BLOCK) void k_rescue_spread(const fe *__restrict__ in, uint64_t count, uint32_t width, uint32_t arity, uint32_t digest,
                                                                   uint32_t modified, const fe *__restrict__ consts, uint32_t rounds, uint64_t alpha,
                                                                   const uint32_t *__restrict__ sched, uint32_t nops, uint32_t table, fe *__restrict__ out) {
    const uint32_t lane = threadIdx.x, j = lane % G, base = lane - j;
    const uint64_t perm = (uint64_t)blockIdx.x * (GS_RESCUE_BLOCK / G) + lane / G;
    const bool live = perm < count && j < width;
    const uint32_t col = j < width ? j : 0;                                 // a surplus lane reads keys that exist and multiplies them by nothing
    const fe *__restrict__ mds = consts + (uint64_t)(2 * rounds + 3) * width;
    fe row[G];
#pragma unroll
    for (int k = 0; k < G; k++) row[k] = (j < width && k < (int)width) ? mds[j * width + k] : fe_zero();
    fe x = (live && j < arity) ? in[perm * arity + j] : fe_zero();
    uint32_t halves, key, inverse;
    rescue_shape(rounds, modified, halves, key, inverse);
    if (!modified) x = fe_add(x, consts[col]);
#pragma unroll 1
    for (uint32_t h = 0; h < halves; h++, key++, inverse ^= 1u) {
        x = inverse ? rescue_inv_sbox<rescue_chain>(x, sched, nops, table) : fe_pow_u64(x, alpha);
        fe acc = consts[(uint64_t)key * width + col];
#pragma unroll
        for (int k = 0; k < G; k++) acc = fe_add(acc, fe_mul(row[k], rescue_lane_read(x, (int)(base + k))));
        x = j < width ? acc : fe_zero();
    }
    if (live && j < digest) out[perm * digest + j] = x;
}

// The root every path implies (tree_verify.h), in form 2: an aligned group of G lanes walks one path, lane j holding element j of the
// state.  paths[k] = the leaf, then `depth` siblings bottom-up, one element each; the walk starts from leaves[k] when `leaves` is given.
// Between two levels lane 0 holds the running node (element 0 of the modified sponge) and lane 1 loads the sibling; the two swap
// values when bit l of idx[k] is 1 (the running node enters on the right), every other lane carries zero: the state (left, right,
// zeros) of a tree level's row.  Every lane stays active to the end — the cross-lane reads need the whole wave —, only the loads and
// the final store are guarded.
template <int G>
__global__ __launch_bounds__(GS_RESCUE_BLOCK) void k_rescue_path_roots(const fe *__restrict__ paths, uint32_t depth, const uint64_t *__restrict__ idx,
                                                                       const fe *__restrict__ leaves, uint64_t count, uint32_t width, const fe *__restrict__ consts,
                                                                       uint32_t rounds, uint64_t alpha, const uint32_t *__restrict__ sched, uint32_t nops, uint32_t table,
                                                                       fe *__restrict__ roots) {
    const uint32_t lane = threadIdx.x, j = lane % G, base = lane - j;
    const uint64_t k = (uint64_t)blockIdx.x * (GS_RESCUE_BLOCK / G) + lane / G;
    const bool live = k < count;
    const uint32_t col = j < width ? j : 0;                                 // a surplus lane reads keys that exist and multiplies them by nothing
    const fe *__restrict__ mds = consts + (uint64_t)(2 * rounds + 3) * width;
    fe row[G];
#pragma unroll
    for (int i = 0; i < G; i++) row[i] = (j < width && i < (int)width) ? mds[j * width + i] : fe_zero();
    const fe *__restrict__ path = paths + (live ? k : 0) * (depth + 1);
    const uint64_t index = live ? idx[k] : 0;
    fe x = (live && j == 0) ? (leaves ? leaves[k] : path[0]) : fe_zero();
    uint32_t halves, first_key, first_inverse;
    rescue_shape(rounds, 1, halves, first_key, first_inverse);
#pragma unroll 1
    for (uint32_t l = 0; l < depth; l++) {
        const fe mine = j == 0 ? x : ((live && j == 1) ? path[l + 1] : fe_zero());      // lane 0: the running node, lane 1: the sibling
        const fe other = rescue_lane_read(mine, (int)(base + (j ^ 1u)));
        x = j < 2 ? (((index >> l) & 1u) ? other : mine) : fe_zero();
        uint32_t key = first_key, inverse = first_inverse;
#pragma unroll 1
        for (uint32_t h = 0; h < halves; h++, key++, inverse ^= 1u) {
            x = inverse ? rescue_inv_sbox<rescue_chain>(x, sched, nops, table) : fe_pow_u64(x, alpha);
            fe acc = consts[(uint64_t)key * width + col];
#pragma unroll
            for (int i = 0; i < G; i++) acc = fe_add(acc, fe_mul(row[i], rescue_lane_read(x, (int)(base + i))));
            x = j < width ? acc : fe_zero();
        }
    }
    if (live && j == 0) roots[k] = x;
}

// Records of any length (include/gstark_absorb.h), in form 2 as the path walk: an aligned group of G lanes absorbs one row, lane j
// holding element j of the state from the first block to the digest.  Lane `rate` starts as the length, every other lane as zero; for
// every block lane j < rate adds its element of the block (none past the end of the row), then the group permutes as k_rescue_spread
// does.  Every lane stays active to the end — the cross-lane reads need the whole wave —, only the loads and the store are guarded.
// A grid-stride loop whose trip count is that of the whole wave (a workgroup is one wave): the grid is capped.
template <int G>
__global__ __launch_bounds__(GS_RESCUE_BLOCK) void k_rescue_absorb(const fe *__restrict__ in, uint64_t count, uint32_t length, uint64_t row_stride, uint64_t elem_stride,
                                                                   uint32_t rate, uint32_t digest, uint32_t modified, uint32_t width, const fe *__restrict__ consts,
                                                                   uint32_t rounds, uint64_t alpha, const uint32_t *__restrict__ sched, uint32_t nops, uint32_t table,
                                                                   fe *__restrict__ out) {
    const uint32_t lane = threadIdx.x, j = lane % G, base = lane - j;
    const uint32_t col = j < width ? j : 0;                                 // a surplus lane reads keys that exist and multiplies them by nothing
    const fe *__restrict__ mds = consts + (uint64_t)(2 * rounds + 3) * width;
    fe row[G];
#pragma unroll
    for (int i = 0; i < G; i++) row[i] = (j < width && i < (int)width) ? mds[j * width + i] : fe_zero();
    uint32_t halves, first_key, first_inverse;
    rescue_shape(rounds, modified, halves, first_key, first_inverse);
#pragma unroll 1
    for (uint64_t first_row = (uint64_t)blockIdx.x * (GS_RESCUE_BLOCK / G); first_row < count; first_row += (uint64_t)gridDim.x * (GS_RESCUE_BLOCK / G)) {
        const uint64_t k = first_row + lane / G;
        const bool live = k < count;
        const fe *__restrict__ mine = in + (live ? k : 0) * row_stride;
        fe x = j == rate ? fe_make(length, 0, 0, 0) : fe_zero();
#pragma unroll 1
        for (uint32_t first = 0; first < length; first += rate) {
            if (live && j < rate && first + j < length) x = fe_add(x, mine[(uint64_t)(first + j) * elem_stride]);
            if (!modified) x = fe_add(x, consts[col]);
            uint32_t key = first_key, inverse = first_inverse;
#pragma unroll 1
            for (uint32_t h = 0; h < halves; h++, key++, inverse ^= 1u) {
                x = inverse ? rescue_inv_sbox<rescue_chain>(x, sched, nops, table) : fe_pow_u64(x, alpha);
                fe acc = consts[(uint64_t)key * width + col];
#pragma unroll
                for (int i = 0; i < G; i++) acc = fe_add(acc, fe_mul(row[i], rescue_lane_read(x, (int)(base + i))));
                x = j < width ? acc : fe_zero();
            }
        }
        if (live && j < digest) out[k * digest + j] = x;
    }
}

namespace {

uint32_t spread_group(const gs_rescue *h) { return h->width <= 2 ? 2u : (h->width <= 4 ? 4u : 8u); }

int launch_path_roots(gs_ctx *c, const gs_rescue *h, const fe *paths, uint32_t depth, const uint64_t *idx, const fe *leaves, uint64_t count, fe *roots) {
    const uint32_t g = spread_group(h);                                      // (width 3 .. 8: 4 or 8)
    const uint64_t per = GS_RESCUE_BLOCK / g, blocks = (count + per - 1) / per;
#define X(G)                                                                                                                                          \
    hipLaunchKernelGGL(k_rescue_path_roots<G>, dim3((unsigned)blocks), dim3(GS_RESCUE_BLOCK), 0, c->stream, paths, depth, idx, leaves, count, h->width, \
                       (const fe *)h->consts, h->rounds, h->alpha, h->sched, h->nops, h->table, roots)
    if (g == 4) X(4);
    else X(8);
#undef X
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

#define GS_RESCUE_ABSORB_GRID (1u << 24)     // workgroups of k_rescue_absorb at most: 2^30 lanes, the rows beyond them by the stride loop

int launch_absorb(gs_ctx *c, const gs_rescue *h, const fe *in, uint64_t count, uint32_t length, uint64_t row_stride, uint64_t elem_stride, uint32_t rate, uint32_t digest,
                  uint32_t modified, fe *out) {
    const uint32_t g = spread_group(h);
    const uint64_t per = GS_RESCUE_BLOCK / g;
    uint64_t blocks = (count + per - 1) / per;
    if (blocks > GS_RESCUE_ABSORB_GRID) blocks = GS_RESCUE_ABSORB_GRID;
#define X(G)                                                                                                                                          \
    hipLaunchKernelGGL(k_rescue_absorb<G>, dim3((unsigned)blocks), dim3(GS_RESCUE_BLOCK), 0, c->stream, in, count, length, row_stride, elem_stride, rate, digest, \
                       modified, h->width, (const fe *)h->consts, h->rounds, h->alpha, h->sched, h->nops, h->table, out)
    if (g == 2) X(2);
    else if (g == 4) X(4);
    else X(8);
#undef X
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int launch_hash(gs_ctx *c, const gs_rescue *h, const fe *in, uint64_t count, uint32_t arity, uint32_t digest, uint32_t modified, uint32_t form, fe *out) {
    if (form == 2) {
        const uint32_t g = h->width <= 2 ? 2 : (h->width <= 4 ? 4 : 8);
        const uint64_t per = GS_RESCUE_BLOCK / g, blocks = (count + per - 1) / per;
#define X(G)                                                                                                                                          \
    hipLaunchKernelGGL(k_rescue_spread<G>, dim3((unsigned)blocks), dim3(GS_RESCUE_BLOCK), 0, c->stream, in, count, h->width, arity, digest, modified, \
                       (const fe *)h->consts, h->rounds, h->alpha, h->sched, h->nops, h->table, out)
        if (g == 2) X(2);
        else if (g == 4) X(4);
        else X(8);
#undef X
    } else {
        const uint64_t blocks = (count + GS_RESCUE_BLOCK - 1) / GS_RESCUE_BLOCK;
        switch (h->width) {
#define X(W)                                                                                                                                         \
    case W:                                                                                                                                          \
        hipLaunchKernelGGL(k_rescue_hash<W>, dim3((unsigned)blocks), dim3(GS_RESCUE_BLOCK), 0, c->stream, in, count, arity, digest, modified,       \
                           (const fe *)h->consts, h->rounds, h->alpha, h->sched, h->nops, h->table, out);                                           \
        break;
            GS_SPONGE_WIDTHS(X)
#undef X
        }
    }
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

// products of one permutation: the S-boxes and the matrix of every half round
uint64_t rescue_products(const gs_rescue *h, uint32_t modified) {
    const uint64_t w = h->width, pairs = modified ? h->rounds - 1 : h->rounds;
    return pairs * (w * (h->inv_products + h->alpha_products) + 2 * w * w);
}

uint32_t pick_form(uint64_t count, uint32_t form) { return form ? form : (count <= GS_RESCUE_SPREAD_LIMIT ? 2u : 1u); }

void traffic(gs_ctx *c, const gs_rescue *h, uint64_t count, uint32_t arity, uint32_t digest, uint32_t modified, uint32_t form) {
    if (form == 2) gs_traffic(c, count * (arity + digest) * GS_ELT, count * rescue_products(h, modified), "k_rescue_spread<%u>", h->width <= 2 ? 2u : (h->width <= 4 ? 4u : 8u));
    else gs_traffic(c, count * (arity + digest) * GS_ELT, count * rescue_products(h, modified), "k_rescue_hash<%u>", h->width);
}

// the tree_node_hash of this unit (field_tree.h) and a level of its tree build: `count` rows of two nodes (of one element) into `count` nodes
int rescue_node_hash(gs_ctx *c, const void *handle, uint32_t, const fe *rows, uint64_t count, fe *out) {
    const gs_rescue *h = (const gs_rescue *)handle;
    const uint32_t form = pick_form(count, 0);
    traffic(c, h, count, 2, 1, 1, form);
    return launch_hash(c, h, rows, count, 2, 1, 1, form, out);
}

int rescue_check_nodes(gs_ctx *c, const gs_rescue *h, const char *who) {
    return h->width >= 3 ? GS_OK : gs_fail(c, GS_ERR_ARG, "%s: two nodes do not fit a state of %u beside its capacity (width 3 .. 8)", who, h->width);
}

// the sliding-window schedule of exponent `bits` (most significant first at bits[nb - 1]) for a window of `w` bits: the words, the
// table size it needs, and what it costs in squarings + products (table included)
uint64_t window_schedule(const std::vector<uint8_t> &bits, int w, std::vector<uint32_t> &ops, uint32_t &table) {
    ops.clear();
    uint32_t top = 0, pending = 0;
    uint64_t cost = 0;
    for (int i = (int)bits.size() - 1; i >= 0;) {
        if (!bits[i]) { pending++; i--; continue; }
        int l = i - w + 1 < 0 ? 0 : i - w + 1;
        while (!bits[l]) l++;                                                // the window ends in a one: its value is odd
        uint32_t v = 0;
        for (int b = i; b >= l; b--) v = 2 * v + bits[b];
        const uint32_t idx = (v - 1) / 2;
        if (idx > top) top = idx;
        if (ops.empty()) ops.push_back(idx);
        else {
            ops.push_back((pending + (uint32_t)(i - l + 1)) << 8 | idx);
            cost += pending + (i - l + 1) + 1;
        }
        pending = 0;
        i = l - 1;
    }
    if (pending) { ops.push_back(pending << 8 | GS_RESCUE_NO_PRODUCT); cost += pending; }
    table = top + 1;
    return cost + (table > 1 ? table : 0);                                   // x^2 and table - 1 products
}

}  // namespace

extern "C" {

uint64_t gs_rescue_spread_limit(void) { return GS_RESCUE_SPREAD_LIMIT; }

int gs_rescue_create(gs_ctx *c, uint32_t width, uint32_t rounds, uint64_t alpha, const uint8_t *inv_exponent, const uint8_t *mds_host, const uint8_t *keys_host,
                     gs_rescue **out) {
    if (!c || !out) return GS_ERR_ARG;
    *out = nullptr;
    if (!inv_exponent || !mds_host || !keys_host) return gs_fail(c, GS_ERR_ARG, "rescue_create: the exponent, the matrix and the keys are required");
    if (width < 2 || width > 8) return gs_fail(c, GS_ERR_ARG, "rescue_create: width %u is outside 2 .. 8", width);
    if (rounds < 1 || rounds > (1u << 16)) return gs_fail(c, GS_ERR_ARG, "rescue_create: %u rounds (1 .. 65536)", rounds);
    if (alpha < 2) return gs_fail(c, GS_ERR_ARG, "rescue_create: alpha is at least 2");
    const fe e = fe_from_bytes(inv_exponent);
    if (fe_ge_p(e) || fe_is_zero(e) || fe_is_zero(fe_add(e, fe_one())))
        return gs_fail(c, GS_ERR_ARG, "rescue_create: the inverse exponent is a canonical element in 1 .. p - 2");
    std::vector<uint8_t> bits;
    for (int i = 0; i < GF_LIMBS * 32; i++) bits.push_back((fe_limb(e, i / 32) >> (i % 32)) & 1u);
    while (!bits.back()) bits.pop_back();
    std::vector<uint32_t> ops, best;
    uint32_t table = 0, best_table = 0;
    uint64_t best_cost = ~0ull;
    for (int w = 1; (1 << (w - 1)) <= GS_RESCUE_TABLE; w++) {               // fewest products; the narrower window on a tie
        const uint64_t cost = window_schedule(bits, w, ops, table);
        if (cost < best_cost) { best_cost = cost; best = ops; best_table = table; }
    }
    const uint64_t nkeys = (uint64_t)(2 * rounds + 3) * width, nmds = (uint64_t)width * width;
    void *p = nullptr;
    const int rc = sponge_upload(c, {{keys_host, nkeys * GS_ELT}, {mds_host, nmds * GS_ELT}, {best.data(), best.size() * 4}}, &p);
    if (rc) return rc;
    fe *consts = (fe *)p;
    *out = new gs_rescue{c, width, rounds, alpha, (uint32_t)best.size(), best_table, best_cost, sponge_pow_products(alpha), consts, (const uint32_t *)(consts + nkeys + nmds)};
    sponge_register(*out);
    return GS_OK;
}

int gs_rescue_destroy(gs_ctx *c, gs_rescue *h) { return sponge_destroy(c, h, "rescue_destroy"); }

int gs_rescue_hash(gs_ctx *c, const gs_rescue *h, const void *in, uint64_t count, uint32_t arity, uint32_t digest, uint32_t modified, uint32_t form, void *out) {
    int rc;
    if ((rc = sponge_check_handle(c, h, "rescue_hash")) || (rc = sponge_check_rows(c, "rescue_hash", arity, h->width, h->width, digest))) return rc;
    if (modified > 1) return gs_fail(c, GS_ERR_ARG, "rescue_hash: modified is 0 (sponge) or 1 (modifiedSponge), not %u", modified);
    if (form > 2) return gs_fail(c, GS_ERR_ARG, "rescue_hash: form is 0 (chosen here), 1 (a thread per permutation) or 2 (a lane per element), not %u", form);
    if ((rc = sponge_check_count(c, "rescue_hash", count))) return rc;
    if (form == 2 && count > GS_RESCUE_SPREAD_MAX) return gs_fail(c, GS_ERR_ARG, "rescue_hash: form 2 serves at most 2^24 permutations per call");
    if (!count) return GS_OK;
    if (!in || !out) return GS_ERR_ARG;
    form = pick_form(count, form);
    traffic(c, h, count, arity, digest, modified, form);
    return launch_hash(c, h, (const fe *)in, count, arity, digest, modified, form, (fe *)out);
}

int gs_rescue_absorb(gs_ctx *c, const gs_rescue *h, const void *in, uint64_t count, uint32_t length, uint64_t row_stride, uint64_t elem_stride, uint32_t rate,
                     uint32_t digest, uint32_t modified, void *out) {
    int rc;
    uint64_t blocks = 0;
    if ((rc = sponge_check_handle(c, h, "rescue_absorb"))) return rc;
    if (modified > 1) return gs_fail(c, GS_ERR_ARG, "rescue_absorb: modified is 0 (sponge) or 1 (modifiedSponge), not %u", modified);
    if ((rc = sponge_check_absorb(c, "rescue_absorb", h->width, count, length, row_stride, elem_stride, rate, digest, in, out, &blocks)) || !count) return rc;
    gs_traffic(c, count * (length + digest) * GS_ELT, count * blocks * rescue_products(h, modified), "k_rescue_absorb<%u>", spread_group(h));
    return launch_absorb(c, h, (const fe *)in, count, length, row_stride, elem_stride, rate, digest, modified, (fe *)out);
}

int gs_rescue_merkle(gs_ctx *c, const gs_rescue *h, const void *leaves, uint64_t n, void *nodes_out) {
    int rc;
    if ((rc = sponge_check_handle(c, h, "rescue_merkle")) || (rc = sponge_check_leaves(c, "rescue_merkle", n)) || (rc = rescue_check_nodes(c, h, "rescue_merkle"))) return rc;
    if (!leaves || !nodes_out) return GS_ERR_ARG;
    fe *nodes = (fe *)nodes_out;
    if (leaves != (const void *)(nodes + n)) GS_HIP(c, hipMemcpyAsync(nodes + n, leaves, n * GS_ELT, hipMemcpyDeviceToDevice, c->stream));
    GS_HIP(c, hipMemsetAsync(nodes, 0, GS_ELT, c->stream));
    uint64_t rest;
    return sponge_tree_levels(nodes, n, 1, 0, &rest, [&](const fe *below, uint64_t count, fe *level) { return rescue_node_hash(c, h, 1, below, count, level); });
}

int gs_rescue_merkle_update(gs_ctx *c, const gs_rescue *h, void *nodes, uint64_t n, const uint64_t *indexes_host, const void *leaves, uint64_t count, void *before_out,
                            void *roots_out) {
    int rc;
    if ((rc = sponge_check_handle(c, h, "rescue_merkle_update")) || (rc = rescue_check_nodes(c, h, "rescue_merkle_update"))) return rc;
    if ((rc = tree_update_check(c, "rescue_merkle_update", n, count, indexes_host, nodes, leaves, before_out, roots_out)) || !count) return rc;
    return tree_update_run(c, (fe *)nodes, n, 1, indexes_host, (const fe *)leaves, count, (fe *)before_out, (fe *)roots_out, {rescue_node_hash, h});
}

int gs_rescue_sparse_create(gs_ctx *c, const gs_rescue *h, uint32_t depth, const void *empty_leaf_host, uint64_t slots_hint, gs_sparse **tree) {
    int rc;
    if (c && h && !sponge_serial(h)) return gs_fail(c, GS_ERR_ARG, "rescue_sparse_create: the hash has been destroyed");
    if ((rc = sponge_check_handle(c, h, "rescue_sparse_create")) || (rc = rescue_check_nodes(c, h, "rescue_sparse_create"))) return rc;
    return sparse_tree_create(c, "rescue_sparse_create", {rescue_node_hash, h}, depth, 1, empty_leaf_host, slots_hint, tree);
}

int gs_rescue_merkle_path_roots(gs_ctx *c, const gs_rescue *h, const void *paths, uint32_t depth, const uint64_t *indexes_host, const void *leaves, uint64_t count,
                                void *roots_out) {
    int rc;
    if ((rc = sponge_check_handle(c, h, "rescue_merkle_path_roots")) || (rc = rescue_check_nodes(c, h, "rescue_merkle_path_roots"))) return rc;
    if ((rc = tree_verify_check(c, "rescue_merkle_path_roots", depth, count, indexes_host, paths, roots_out)) || !count) return rc;
    return tree_verify_run(c, indexes_host, count, [&](const uint64_t *idx) {
        gs_traffic(c, tree_verify_bytes(depth, 1, leaves != nullptr, count), count * depth * rescue_products(h, 1), "k_rescue_path_roots<%u>", spread_group(h));
        return launch_path_roots(c, h, (const fe *)paths, depth, idx, (const fe *)leaves, count, (fe *)roots_out);
    });
}

}  // extern "C"
