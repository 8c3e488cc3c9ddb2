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
//   paths       k_hades_paths / gs_hades_merkle_paths read nothing but a node array: family-neutral (sponge_common.h), defined here.
//   updates     gs_hades_merkle_update: the shared driver of tree_update.h over launch_hash, so an updated node is the node the tree
//               build computes.  Its two kernels (k_tree_update_gather / _commit) know no permutation either and are defined here too.
//   sparse      gs_hades_sparse_create: the shared driver of sparse_tree.h over launch_hash.  Its three kernels (k_sparse_gather / _commit /
//               _paths) read nodes at slots of a store, know no permutation and are defined here, with the family-neutral entries
//               gs_sparse_* (include/gstark_sparse_tree.h).
//   path roots  gs_hades_merkle_path_roots (tree_verify.h): one thread walks one path through all its levels in ONE launch
//               (k_hades_path_roots), the running node in registers; the sibling of a level is read straight from the path array.
#include "sponge_common.h"
#include "tree_update.h"
#include "sparse_tree.h"
#include "tree_verify.h"
#include "../../include/gstark_hades.h"
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

// out[path][level][e]: the leaf (level 0), then the sibling on every level from the leaves up — of any tree in the heap layout
__global__ __launch_bounds__(256) void k_hades_paths(const fe *__restrict__ nodes, uint64_t n, uint32_t depth, uint32_t digest, const uint64_t *__restrict__ idx,
                                                     uint64_t total, fe *__restrict__ out) {
    const uint64_t per_path = (uint64_t)(depth + 1) * digest;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t path = t / per_path, e = t % digest;
        const uint32_t l = (uint32_t)((t % per_path) / digest);
        const uint64_t leaf = n + idx[path];
        const uint64_t node = l ? ((leaf >> (l - 1)) ^ 1) : leaf;
        out[t] = nodes[node * digest + e];
    }
}

// one level of a batch of updates (tree_update.h), of any tree in the heap layout: element e of update j's version ver_l[j] and of its
// sibling's value — the version of the update the plan names, or what the node array holds — land side by side in rows[j] in
// left/right order; the sibling is before[j][level + 1], and on level 0 the old leaf (the previous update of the same leaf, or the
// node array) is before[j][0].  Reads of the node array only: the commit writes it, after the last level.
__global__ __launch_bounds__(256) void k_tree_update_gather(const fe *__restrict__ nodes, uint64_t n, uint32_t digest, uint32_t depth, uint32_t level, uint64_t total,
                                                            const uint64_t *__restrict__ idx, const int32_t *__restrict__ same, const int32_t *__restrict__ pred,
                                                            const fe *__restrict__ ver_l, fe *__restrict__ rows, fe *__restrict__ before) {
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = t / digest, e = t % digest;
        const uint64_t node = (n + idx[j]) >> level;
        const int32_t p = pred[j];                                           // (the caller has moved `pred` to this level's row)
        const fe sibling = p >= 0 ? ver_l[(uint64_t)p * digest + e] : nodes[(node ^ 1) * digest + e];
        const uint64_t right = node & 1;
        rows[j * 2 * digest + (right ? digest : 0) + e] = ver_l[t];
        rows[j * 2 * digest + (right ? 0 : digest) + e] = sibling;
        before[(j * (depth + 1) + level + 1) * digest + e] = sibling;
        if (level == 0) {
            const int32_t s = same[j];
            before[j * (depth + 1) * digest + e] = s >= 0 ? ver_l[(uint64_t)s * digest + e] : nodes[node * digest + e];
        }
    }
}

// after the last level: the version of every node's latest toucher into the node array; item t = (level, update, element)
__global__ __launch_bounds__(256) void k_tree_update_commit(fe *__restrict__ nodes, uint64_t n, uint32_t digest, uint32_t depth, uint64_t count, uint64_t total,
                                                            const uint64_t *__restrict__ idx, const uint8_t *__restrict__ last, const fe *__restrict__ leaves,
                                                            const fe *__restrict__ mid, const fe *__restrict__ roots) {
    const uint64_t per_level = count * digest;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = (uint32_t)(t / per_level);
        const uint64_t at = t % per_level, j = at / digest, e = at % digest;
        if (!last[l * count + j]) continue;
        const fe *__restrict__ ver = l == 0 ? leaves : (l == depth ? roots : mid + (uint64_t)(l - 1) * per_level);
        nodes[((n + idx[j]) >> l) * digest + e] = ver[at];
    }
}

int tree_update_gather(gs_ctx *c, const fe *nodes, uint64_t n, uint32_t digest, uint32_t depth, uint32_t level, uint64_t count, const tree_update_device_plan &plan,
                       const fe *ver_l, fe *rows, fe *before) {
    const uint64_t total = count * digest;
    gs_traffic(c, (5 * total + (level ? 0 : 2 * total)) * GS_ELT + count * 12, 0, "k_tree_update_gather");
    hipLaunchKernelGGL(k_tree_update_gather, dim3(gs_grid(total)), dim3(256), 0, c->stream, nodes, n, digest, depth, level, total, plan.idx, plan.same,
                       plan.pred + (uint64_t)level * count, ver_l, rows, before);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int tree_update_commit(gs_ctx *c, fe *nodes, uint64_t n, uint32_t digest, uint32_t depth, uint64_t count, const tree_update_device_plan &plan, const fe *leaves,
                       const fe *mid, const fe *roots) {
    const uint64_t total = (uint64_t)(depth + 1) * count * digest;
    gs_traffic(c, 2 * total * GS_ELT + (uint64_t)(depth + 1) * count, 0, "k_tree_update_commit");
    hipLaunchKernelGGL(k_tree_update_commit, dim3(gs_grid(total)), dim3(256), 0, c->stream, nodes, n, digest, depth, count, total, plan.idx, plan.last, leaves, mid, roots);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

// ---- sparse trees (sparse_tree.h): the dense update and path kernels above with every read of the node array replaced by a read at a
// slot of the node store, or of empties[level] where the host found no slot (GS_SPARSE_EMPTY).  Slots have been checked against the
// store on the host.  One thread per element, grid-stride, 64-bit indexes, plain loads and stores; no ordering but the stream's.
__global__ __launch_bounds__(256) void k_sparse_gather(const fe *__restrict__ store, const fe *__restrict__ empties, uint32_t digest, uint32_t depth, uint32_t level,
                                                       uint64_t total, const uint64_t *__restrict__ idx, const int32_t *__restrict__ same, const int32_t *__restrict__ pred,
                                                       const uint32_t *__restrict__ sib, const uint32_t *__restrict__ old, const fe *__restrict__ ver_l,
                                                       fe *__restrict__ rows, fe *__restrict__ before) {
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = t / digest, e = t % digest;
        const int32_t p = pred[j];                                           // (the caller has moved `pred` and `sib` to this level's row)
        const uint32_t s = sib[j];
        const fe sibling = p >= 0 ? ver_l[(uint64_t)p * digest + e] : (s != GS_SPARSE_EMPTY ? store[(uint64_t)s * digest + e] : empties[(uint64_t)level * digest + e]);
        const uint64_t right = (idx[j] >> level) & 1;
        rows[j * 2 * digest + (right ? digest : 0) + e] = ver_l[t];
        rows[j * 2 * digest + (right ? 0 : digest) + e] = sibling;
        before[(j * (depth + 1) + level + 1) * digest + e] = sibling;
        if (level == 0) {
            const int32_t q = same[j];
            const uint32_t o = old[j];
            before[j * (depth + 1) * digest + e] = q >= 0 ? ver_l[(uint64_t)q * digest + e] : (o != GS_SPARSE_EMPTY ? store[(uint64_t)o * digest + e] : empties[e]);
        }
    }
}

// after the last level: the version of every node's latest toucher into its slot; item t = (level, update, element)
__global__ __launch_bounds__(256) void k_sparse_commit(fe *__restrict__ store, uint32_t digest, uint32_t depth, uint64_t count, uint64_t total,
                                                       const uint32_t *__restrict__ write, const fe *__restrict__ leaves, const fe *__restrict__ mid,
                                                       const fe *__restrict__ roots) {
    const uint64_t per_level = count * digest;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = (uint32_t)(t / per_level);
        const uint64_t at = t % per_level, j = at / digest, e = at % digest;
        const uint32_t w = write[(uint64_t)l * count + j];
        if (w == GS_SPARSE_EMPTY) continue;
        const fe *__restrict__ ver = l == 0 ? leaves : (l == depth ? roots : mid + (uint64_t)(l - 1) * per_level);
        store[(uint64_t)w * digest + e] = ver[at];
    }
}

// out[path][place][e]: the leaf (place 0), then the sibling on every level from the leaves up, by slot
__global__ __launch_bounds__(256) void k_sparse_paths(const fe *__restrict__ store, const fe *__restrict__ empties, uint32_t depth, uint32_t digest,
                                                      const uint32_t *__restrict__ slots, uint64_t total, fe *__restrict__ out) {
    const uint64_t per_path = (uint64_t)(depth + 1) * digest;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t path = t / per_path, e = t % digest;
        const uint32_t place = (uint32_t)((t % per_path) / digest);
        const uint32_t s = slots[path * (depth + 1) + place];
        out[t] = s != GS_SPARSE_EMPTY ? store[(uint64_t)s * digest + e] : empties[(uint64_t)(place ? place - 1 : 0) * digest + e];
    }
}

int sparse_tree_gather(gs_ctx *c, const fe *store, const fe *empties, uint32_t digest, uint32_t depth, uint32_t level, uint64_t count, const uint64_t *idx,
                       const int32_t *same, const int32_t *pred, const uint32_t *sib, const uint32_t *old, const fe *ver_l, fe *rows, fe *before) {
    const uint64_t total = count * digest;
    gs_traffic(c, (5 * total + (level ? 0 : 2 * total)) * GS_ELT + count * 16 + (level ? 0 : count * 8), 0, "k_sparse_gather");
    hipLaunchKernelGGL(k_sparse_gather, dim3(gs_grid(total)), dim3(256), 0, c->stream, store, empties, digest, depth, level, total, idx, same, pred, sib, old, ver_l, rows,
                       before);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int sparse_tree_commit(gs_ctx *c, fe *store, uint32_t digest, uint32_t depth, uint64_t count, const uint32_t *write, const fe *leaves, const fe *mid, const fe *roots) {
    const uint64_t total = (uint64_t)(depth + 1) * count * digest;
    gs_traffic(c, 2 * total * GS_ELT + (uint64_t)(depth + 1) * count * 4, 0, "k_sparse_commit");
    hipLaunchKernelGGL(k_sparse_commit, dim3(gs_grid(total)), dim3(256), 0, c->stream, store, digest, depth, count, total, write, leaves, mid, roots);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int sparse_tree_path_gather(gs_ctx *c, const fe *store, const fe *empties, uint32_t digest, uint32_t depth, uint64_t count, const uint32_t *slots, fe *out) {
    const uint64_t total = count * (depth + 1) * digest;
    gs_traffic(c, 2 * total * GS_ELT + count * (depth + 1) * 4, 0, "k_sparse_paths");
    hipLaunchKernelGGL(k_sparse_paths, dim3(gs_grid(total)), dim3(256), 0, c->stream, store, empties, depth, digest, slots, total, out);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

namespace {

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

int gs_hades_merkle(gs_ctx *c, const gs_hades *h, const void *leaves, uint64_t n, uint32_t digest, void *nodes_out) {
    int rc;
    if ((rc = sponge_check_handle(c, h, "hades_merkle")) || (rc = sponge_check_leaves(c, "hades_merkle", n))) return rc;
    if (digest < 1 || digest > 2 || 2 * digest >= h->width)
        return gs_fail(c, GS_ERR_ARG, "hades_merkle: nodes of %u elements (1 or 2): two of them do not fit a state of %u beside its capacity", digest, h->width);
    if (!leaves || !nodes_out) return GS_ERR_ARG;
    fe *nodes = (fe *)nodes_out;
    if (leaves != (const void *)(nodes + n * digest))
        GS_HIP(c, hipMemcpyAsync(nodes + n * digest, leaves, n * digest * GS_ELT, hipMemcpyDeviceToDevice, c->stream));
    uint64_t cnt;
    rc = sponge_tree_levels(nodes, n, digest, GS_HADES_BLOCK, &cnt, [&](const fe *below, uint64_t count, fe *level) {
        gs_traffic(c, 3 * count * digest * GS_ELT, count * hades_products(h), "k_hades_merkle_level<%u>", h->width);
        return launch_hash(c, h, below, count, 2 * digest, digest, level);
    });
    if (rc) return rc;
    gs_traffic(c, (4 * cnt - 1) * digest * GS_ELT, (2 * cnt - 1) * hades_products(h), "k_hades_merkle_top<%u>", h->width);
    return launch_top(c, h, nodes, (uint32_t)cnt, digest);
}

int gs_hades_merkle_paths(gs_ctx *c, const void *nodes, uint64_t n, uint32_t digest, const uint64_t *indexes_host, uint64_t count, void *out) {
    if (!c) return GS_ERR_ARG;
    int rc = sponge_check_leaves(c, "hades_merkle_paths", n);
    if (rc) return rc;
    if (digest < 1 || digest > 2) return gs_fail(c, GS_ERR_ARG, "hades_merkle_paths: nodes of 1 or 2 elements, not %u", digest);
    if (count > (1ull << 24)) return gs_fail(c, GS_ERR_ARG, "hades_merkle_paths: at most 2^24 paths per call");
    if (!count) return GS_OK;
    if (!nodes || !indexes_host || !out) return GS_ERR_ARG;
    for (uint64_t k = 0; k < count; k++)
        if (indexes_host[k] >= n)
            return gs_fail(c, GS_ERR_ARG, "hades_merkle_paths: index %llu is outside of the %llu leaves", (unsigned long long)indexes_host[k], (unsigned long long)n);
    const uint32_t depth = (uint32_t)gs_log2(n);
    const uint64_t total = count * (depth + 1) * digest;
    void *d_idx = nullptr;
    if ((rc = gs_tmp_alloc(c, count * 8, &d_idx))) return rc;
    if ((rc = gs_push(c, d_idx, indexes_host, count * 8)) == GS_OK) {
        hipLaunchKernelGGL(k_hades_paths, dim3(gs_grid(total)), dim3(256), 0, c->stream, (const fe *)nodes, n, depth, digest, (const uint64_t *)d_idx, total, (fe *)out);
        if (hipGetLastError() != hipSuccess) rc = gs_fail(c, GS_ERR_DEVICE, "hades_merkle_paths: launch failed");
    }
    gs_tmp_free(c, d_idx);                                                   // (stream-ordered cache: the launch above still reads it)
    return rc;
}

int gs_hades_merkle_update(gs_ctx *c, const gs_hades *h, void *nodes, uint64_t n, uint32_t digest, const uint64_t *indexes_host, const void *leaves, uint64_t count,
                           void *before_out, void *roots_out) {
    int rc;
    if ((rc = sponge_check_handle(c, h, "hades_merkle_update"))) return rc;
    if (digest < 1 || digest > 2 || 2 * digest >= h->width)
        return gs_fail(c, GS_ERR_ARG, "hades_merkle_update: nodes of %u elements (1 or 2): two of them do not fit a state of %u beside its capacity", digest, h->width);
    if ((rc = tree_update_check(c, "hades_merkle_update", n, count, indexes_host, nodes, leaves, before_out, roots_out)) || !count) return rc;
    return tree_update_run(c, (fe *)nodes, n, digest, indexes_host, (const fe *)leaves, count, (fe *)before_out, (fe *)roots_out, [&](const fe *rows, uint64_t cnt, fe *out) {
        gs_traffic(c, 3 * cnt * digest * GS_ELT, cnt * hades_products(h), "k_hades_hash<%u>", h->width);
        return launch_hash(c, h, rows, cnt, 2 * digest, digest, out);
    });
}

int gs_hades_sparse_create(gs_ctx *c, const gs_hades *h, uint32_t depth, uint32_t digest, const void *empty_leaf_host, uint64_t slots_hint, gs_sparse **tree) {
    int rc;
    if (c && h && !sponge_serial(h)) return gs_fail(c, GS_ERR_ARG, "hades_sparse_create: the hash has been destroyed");
    if ((rc = sponge_check_handle(c, h, "hades_sparse_create"))) return rc;
    if (digest < 1 || digest > 2 || 2 * digest >= h->width)
        return gs_fail(c, GS_ERR_ARG, "hades_sparse_create: nodes of %u elements (1 or 2): two of them do not fit a state of %u beside its capacity", digest, h->width);
    return sparse_tree_create(c, "hades_sparse_create", h, depth, digest, empty_leaf_host, slots_hint, [c, h, digest](const fe *rows, uint64_t cnt, fe *out) {
        gs_traffic(c, 3 * cnt * digest * GS_ELT, cnt * hades_products(h), "k_hades_hash<%u>", h->width);
        return launch_hash(c, h, rows, cnt, 2 * digest, digest, out);
    }, tree);
}

// ---- the family-neutral entries of include/gstark_sparse_tree.h: the tree carries its unit's launch
int gs_sparse_update(gs_ctx *c, gs_sparse *t, const uint64_t *indexes_host, const void *leaves, uint64_t count, void *before_out, void *roots_out) {
    int rc;
    if ((rc = sparse_tree_check_handle(c, t, "sparse_update")) || (rc = sparse_tree_check_indexes(c, t, "sparse_update", indexes_host, count, "updates")) || !count) return rc;
    if (!leaves || !before_out || !roots_out) return GS_ERR_ARG;
    return sparse_tree_update_run(c, t, indexes_host, (const fe *)leaves, count, (fe *)before_out, (fe *)roots_out);
}

int gs_sparse_paths(gs_ctx *c, const gs_sparse *t, const uint64_t *indexes_host, uint64_t count, void *out) {
    int rc;
    if ((rc = sparse_tree_check_handle(c, t, "sparse_paths")) || (rc = sparse_tree_check_indexes(c, t, "sparse_paths", indexes_host, count, "paths")) || !count) return rc;
    if (!out) return GS_ERR_ARG;
    return sparse_tree_paths_run(c, t, indexes_host, count, (fe *)out);
}

int gs_sparse_root(gs_ctx *c, const gs_sparse *t, void *root_out) {
    const int rc = sparse_tree_check_handle(c, t, "sparse_root");
    if (rc) return rc;
    if (!root_out) return GS_ERR_ARG;
    const uint32_t slot = sparse_plan_root(t->index);
    if (slot != GS_SPARSE_EMPTY && slot >= t->index.slots) return gs_fail(c, GS_ERR_ARG, "sparse_root: the slot of the root lies outside of the node store");
    const fe *src = slot != GS_SPARSE_EMPTY ? t->store + (uint64_t)slot * t->digest : t->empties + (uint64_t)t->depth * t->digest;
    GS_HIP(c, hipMemcpyAsync(root_out, src, t->digest * GS_ELT, hipMemcpyDeviceToDevice, c->stream));
    return GS_OK;
}

int gs_sparse_empties(gs_ctx *c, const gs_sparse *t, void *out) {
    const int rc = sparse_tree_check_handle(c, t, "sparse_empties");
    if (rc) return rc;
    if (!out) return GS_ERR_ARG;
    GS_HIP(c, hipMemcpyAsync(out, t->empties, (uint64_t)(t->depth + 1) * t->digest * GS_ELT, hipMemcpyDeviceToDevice, c->stream));
    return GS_OK;
}

uint64_t gs_sparse_stored(const gs_sparse *t, uint32_t level) { return t && level <= t->depth ? t->index.level[level].used : 0; }

int gs_sparse_destroy(gs_ctx *c, gs_sparse *t) {
    if (!c || !t) return c ? GS_OK : GS_ERR_ARG;
    if (t->ctx != c) return gs_fail(c, GS_ERR_ARG, "sparse_destroy: the tree belongs to another context");      // (its hash may be gone already)
    gs_free(c, t->store);                                                    // parked in the context's cache: launches already queued still read them in order
    gs_free(c, t->empties);
    delete t;
    return GS_OK;
}

int gs_hades_merkle_path_roots(gs_ctx *c, const gs_hades *h, const void *paths, uint32_t depth, uint32_t digest, const uint64_t *indexes_host, const void *leaves,
                               uint64_t count, void *roots_out) {
    int rc;
    if ((rc = sponge_check_handle(c, h, "hades_merkle_path_roots"))) return rc;
    if (digest < 1 || digest > 2 || 2 * digest >= h->width)
        return gs_fail(c, GS_ERR_ARG, "hades_merkle_path_roots: nodes of %u elements (1 or 2): two of them do not fit a state of %u beside its capacity", digest, h->width);
    if ((rc = tree_verify_check(c, "hades_merkle_path_roots", depth, count, indexes_host, paths, roots_out)) || !count) return rc;
    return tree_verify_run(c, indexes_host, count, [&](const uint64_t *idx) {
        gs_traffic(c, tree_verify_bytes(depth, digest, leaves != nullptr, count), count * depth * hades_products(h), "k_hades_path_roots<%u>", h->width);
        return launch_path_roots(c, h, (const fe *)paths, depth, digest, idx, (const fe *)leaves, count, (fe *)roots_out);
    });
}

}  // extern "C"
