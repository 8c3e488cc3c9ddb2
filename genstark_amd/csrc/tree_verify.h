// tree_verify.h — the roots a batch of authentication paths implies (include/gstark_tree_verify.h): what the entries of the algebraic
// hash units share.  A unit brings its kernel: ONE launch walks every level of every path with the running node in registers, the
// unit's own permutation inlined into it, so a node computed here is the node its tree build computes.
//   check     the arguments after the unit's own (its handle, and that two nodes fit its state): depth, count, the arrays, the indexes.
//   run       the indexes go up through the stream-ordered scratch (sponge_with_upload) and the unit's launch reads them there.
// There is no body macro: the two walks have no body in common — hades.hip walks a path per thread, rescue.hip a path per group of lanes.
// Nothing here is host work beyond the argument check: no plan, no sort, nothing in proportion to the depth.
#pragma once
#include "sponge_common.h"

#define GS_TREE_VERIFY_MAX (1ull << 20)      // paths per call
#define GS_TREE_VERIFY_DEPTH 36              // the deepest tree sponge_check_leaves admits

static inline int tree_verify_check(gs_ctx *c, const char *who, uint32_t depth, uint64_t count, const uint64_t *indexes_host, const void *paths, const void *roots) {
    if (depth < 1 || depth > GS_TREE_VERIFY_DEPTH) return gs_fail(c, GS_ERR_ARG, "%s: a depth of %u levels is outside 1 .. %d", who, depth, GS_TREE_VERIFY_DEPTH);
    if (count > GS_TREE_VERIFY_MAX) return gs_fail(c, GS_ERR_ARG, "%s: at most 2^20 paths per call", who);
    if (!count) return GS_OK;
    if (!paths || !indexes_host || !roots) return gs_fail(c, GS_ERR_ARG, "%s: the paths, their indexes and the array of the roots are required", who);
    for (uint64_t k = 0; k < count; k++)
        if (indexes_host[k] >> depth)
            return gs_fail(c, GS_ERR_ARG, "%s: index %llu is outside of the %llu leaves", who, (unsigned long long)indexes_host[k], 1ull << depth);
    return GS_OK;
}

// launch(idx): the unit's kernel over `count` paths with the indexes at `idx` on the device, enqueued on the context's stream.
// count >= 1 and the arguments have passed tree_verify_check.
template <class Launch>
static inline int tree_verify_run(gs_ctx *c, const uint64_t *indexes_host, uint64_t count, Launch launch) {
    return sponge_with_upload(c, indexes_host, count * 8, [&](const void *idx) { return launch((const uint64_t *)idx); });
}

// what a call HAS to move: the paths, the replacing leaves where given, the indexes, the roots
static inline uint64_t tree_verify_bytes(uint32_t depth, uint32_t digest, bool leaves, uint64_t count) {
    return count * (((uint64_t)depth + 2 + (leaves ? 1 : 0)) * digest * GS_ELT + 8);
}
