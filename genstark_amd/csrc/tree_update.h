// tree_update.h — a batch of leaf updates applied to a heap-layout tree on the device, with every update's witness
// (include/gstark_tree_update.h): the driver the algebraic hash units share, as they share sponge_tree_levels.  A unit brings "hash
// these rows": its own launch, so a node computed here is bit for bit the node its tree build computes.
//   plan      tree_update_plan.h, on the host: per (level, update) whose version of the sibling node the update sees.
//   versions  ver[l][j] = the value of node (n + indexes[j]) >> l just after update j.  ver[0] is the new leaves (the caller's array),
//             ver[depth] the roots (the caller's array), the levels between lie level-major in one scratch block: a level's hash
//             launch writes one contiguous run.
//   a level   the gather writes, per update, its version and its sibling's value side by side in left/right order (a row of
//             2 * digest elements) and the sibling into the witness; the unit's launch hashes the rows into ver[l + 1].  No update
//             waits for another: a level is `count` independent permutations.
//   commit    NO level writes the node array: an update further on may still have to read what a node held at the call (its
//             predecessor is -1).  After the last level every node's latest toucher stores its version; one writer per node.
// The two kernels read nothing but arrays and the plan — they know no permutation, like k_hades_paths — and are defined once, beside
// it in hades.hip.  Everything is enqueued on the context's stream; the scratch is stream-ordered (gs_tmp_alloc).
#pragma once
#include "sponge_common.h"
#include "tree_update_plan.h"

// what the kernels read of a plan, on the device
struct tree_update_device_plan {
    const uint64_t *idx;                     // count
    const int32_t *same;                     // count
    const int32_t *pred;                     // depth x count
    const uint8_t *last;                     // (depth + 1) x count
};

// level l of the batch: rows[j] = (left, right) of update j's node pair, before[j][l + 1] = the sibling (and before[j][0] = the old leaf
// on level 0); ver_l = ver[l]
int tree_update_gather(gs_ctx *c, const fe *nodes, uint64_t n, uint32_t digest, uint32_t depth, uint32_t level, uint64_t count, const tree_update_device_plan &plan,
                       const fe *ver_l, fe *rows, fe *before);
// nodes[(n + idx[j]) >> l] = ver[l][j] wherever last[l][j]: ver[0] = leaves, ver[1 .. depth - 1] = mid, ver[depth] = roots
int tree_update_commit(gs_ctx *c, fe *nodes, uint64_t n, uint32_t digest, uint32_t depth, uint64_t count, const tree_update_device_plan &plan, const fe *leaves,
                       const fe *mid, const fe *roots);

// the arguments every unit's entry shares (the unit has checked its handle and that `digest` fits its state)
static inline int tree_update_check(gs_ctx *c, const char *who, uint64_t n, uint64_t count, const uint64_t *indexes_host, const void *nodes, const void *leaves,
                                    const void *before, const void *roots) {
    const int rc = sponge_check_leaves(c, who, n);
    if (rc) return rc;
    if (count > GS_TREE_UPDATE_MAX) return gs_fail(c, GS_ERR_ARG, "%s: at most 2^20 updates per call", who);
    if (!count) return GS_OK;
    if (!nodes || !indexes_host || !leaves || !before || !roots) return GS_ERR_ARG;
    for (uint64_t j = 0; j < count; j++)
        if (indexes_host[j] >= n)
            return gs_fail(c, GS_ERR_ARG, "%s: index %llu is outside of the %llu leaves", who, (unsigned long long)indexes_host[j], (unsigned long long)n);
    return GS_OK;
}

// hash(rows, count, out): `count` rows of 2 * digest elements at `rows` into `count` nodes of `digest` elements at `out`, enqueued on
// the context's stream.  count >= 1 and the arguments have passed tree_update_check.
template <class Hash>
static inline int tree_update_run(gs_ctx *c, fe *nodes, uint64_t n, uint32_t digest, const uint64_t *indexes_host, const fe *leaves, uint64_t count, fe *before,
                                  fe *roots, Hash hash) {
    tree_update_plan plan;
    tree_update_plan_build(n, indexes_host, count, plan);
    const uint32_t depth = plan.depth;
    const uint64_t level_elems = count * digest;
    // one scratch block: the plan, the rows of one level (reused: the stream orders the levels), the versions of levels 1 .. depth - 1
    const uint64_t idx_bytes = count * 8, same_bytes = count * 4, pred_bytes = plan.pred.size() * 4, last_bytes = plan.last.size();
    const uint64_t fe_off = (idx_bytes + same_bytes + pred_bytes + last_bytes + 31) & ~31ull;     // elements start on a multiple of 32 bytes
    const uint64_t total = fe_off + (2 * level_elems + (uint64_t)(depth - 1) * level_elems) * GS_ELT;
    void *block = nullptr;
    int rc = gs_tmp_alloc(c, total, &block);
    if (rc) return rc;
    uint8_t *at = (uint8_t *)block;
    tree_update_device_plan dev;
    dev.idx = (const uint64_t *)at;
    dev.same = (const int32_t *)(at + idx_bytes);
    dev.pred = (const int32_t *)(at + idx_bytes + same_bytes);
    dev.last = at + idx_bytes + same_bytes + pred_bytes;
    fe *rows = (fe *)(at + fe_off), *mid = rows + 2 * level_elems;
    const struct { const void *dst, *src; uint64_t bytes; } parts[] = {
        {dev.idx, indexes_host, idx_bytes}, {dev.same, plan.same.data(), same_bytes}, {dev.pred, plan.pred.data(), pred_bytes}, {dev.last, plan.last.data(), last_bytes}};
    for (const auto &part : parts)
        if (!rc) rc = gs_push(c, (void *)part.dst, part.src, part.bytes);
    for (uint32_t l = 0; l < depth && !rc; l++) {
        const fe *ver_l = l ? mid + (uint64_t)(l - 1) * level_elems : leaves;
        fe *ver_up = l + 1 == depth ? roots : mid + (uint64_t)l * level_elems;
        if ((rc = tree_update_gather(c, nodes, n, digest, depth, l, count, dev, ver_l, rows, before))) break;
        rc = hash((const fe *)rows, count, ver_up);
    }
    if (!rc) rc = tree_update_commit(c, nodes, n, digest, depth, count, dev, leaves, mid, roots);
    gs_tmp_free(c, block);                                                   // (stream-ordered cache: the launches above still read it)
    return rc;
}
