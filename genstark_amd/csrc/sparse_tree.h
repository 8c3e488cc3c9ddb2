// sparse_tree.h — a sparse Merkle tree of fixed depth kept on the device (include/gstark_sparse_tree.h): the driver the algebraic hash
// units share, as they share tree_update.h.  A unit brings "hash these rows": its own launch, so a node computed here is bit for bit the
// node its dense tree build computes.
//   store     slots x digest elements on the device, append-only: a node keeps its slot for life.  It grows by doubling with ONE device
//             copy on the context's stream, and never past GS_SPARSE_MAX_SLOTS = 2^31 slots.
//   index     sparse_tree_plan.h, on the host: per level the slot of every stored node.  A stored leaf costs up to `depth` stored nodes
//             and as many index entries.
//   empties   (depth + 1) x digest elements on the device: empties[0] the empty leaf, empties[l + 1] = node(empties[l], empties[l]),
//             one row per level through the unit's launch.
//   a batch   as in tree_update.h — versions ver[l][j], per level a gather and the unit's hash launch, one commit after the last level —
//             with every read of the node array replaced by a read at a slot, or of empties[l] where the plan found no slot.  The
//             index changes only after every launch has been enqueued without error; before the upload every slot is checked against
//             the slots the store holds (O(count x depth)): a bad slot is an error code, never an access.
// The three kernels read nothing but arrays and slots — they know no permutation — and are defined once, beside the dense ones, in
// hades.hip, with the family-neutral entries (gs_sparse_update, _paths, _root, _empties, _stored, _destroy).  Everything is enqueued on
// the context's stream; nothing is read back.
#pragma once
#include <functional>

#include "sparse_tree_plan.h"
#include "sponge_common.h"

struct gs_sparse {
    gs_ctx *ctx;
    uint32_t depth, digest;
    std::function<int(const fe *rows, uint64_t count, fe *out)> hash;      // the unit's launch over its hash handle (which outlives the tree)
    const void *hash_handle;                 // that handle and the serial it was created under (sponge_common.h): checked, never dereferenced here
    uint64_t hash_serial;
    fe *store;
    uint64_t capacity;                       // slots the store holds
    fe *empties;
    sparse_tree_index index;
};

// level l of the batch: rows[j] = (left, right) of update j's node pair, before[j][l + 1] = the sibling (and before[j][0] = the old leaf on
// level 0); ver_l = ver[l].  pred and sib: row l of the plan's; the kernels are in hades.hip
int sparse_tree_gather(gs_ctx *c, const fe *store, const fe *empties, uint32_t digest, uint32_t depth, uint32_t level, uint64_t count, const uint64_t *idx,
                       const int32_t *same, const int32_t *pred, const uint32_t *sib, const uint32_t *old, const fe *ver_l, fe *rows, fe *before);
// store[write[l][j]] = ver[l][j] wherever write[l][j] is a slot: ver[0] = leaves, ver[1 .. depth - 1] = mid, ver[depth] = roots
int sparse_tree_commit(gs_ctx *c, fe *store, uint32_t digest, uint32_t depth, uint64_t count, const uint32_t *write, const fe *leaves, const fe *mid, const fe *roots);
// out[k][l] = store[slots[k][l]], or the empty node of that place: empties[0] for the leaf, empties[l - 1] for the sibling on level l - 1
int sparse_tree_path_gather(gs_ctx *c, const fe *store, const fe *empties, uint32_t digest, uint32_t depth, uint64_t count, const uint32_t *slots, fe *out);

static inline int sparse_tree_check_handle(gs_ctx *c, const gs_sparse *t, const char *who) {
    if (!c || !t) return GS_ERR_ARG;
    if (t->ctx != c) return gs_fail(c, GS_ERR_ARG, "%s: the tree belongs to another context", who);
    // the closure holds the hash handle's pointer: a call after gs_*_destroy of the hash would read freed memory and launch over freed constants
    return sponge_serial(t->hash_handle) == t->hash_serial ? GS_OK : gs_fail(c, GS_ERR_ARG, "%s: the tree's hash has been destroyed", who);
}

// the store holds at least `slots` slots: doubling, one device copy of what is in use
static inline int sparse_tree_reserve(gs_ctx *c, gs_sparse *t, uint64_t slots, const char *who) {
    if (slots <= t->capacity) return GS_OK;
    if (slots > GS_SPARSE_MAX_SLOTS) return gs_fail(c, GS_ERR_ARG, "%s: the node store does not grow past 2^31 slots", who);
    uint64_t capacity = t->capacity;
    while (capacity < slots) capacity *= 2;
    if (capacity > GS_SPARSE_MAX_SLOTS) capacity = GS_SPARSE_MAX_SLOTS;
    void *grown = nullptr;
    const int rc = gs_alloc(c, capacity * t->digest * GS_ELT, &grown);
    if (rc) return rc;
    if (t->index.slots) {
        const hipError_t e = hipMemcpyAsync(grown, t->store, t->index.slots * t->digest * GS_ELT, hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) {
            gs_free(c, grown);
            return gs_fail(c, GS_ERR_DEVICE, "%s: the copy into the grown store: %s", who, hipGetErrorString(e));
        }
    }
    gs_free(c, t->store);                                                    // (stream-ordered cache: the copy above still reads it)
    t->store = (fe *)grown;
    t->capacity = capacity;
    return GS_OK;
}

// hash(rows, count, out) as in tree_update_run; empty_host: `digest` canonical elements, or null for zeros.  The unit has checked its
// handle `h` (a live one) and that two nodes of `digest` elements fit its state.
template <class Hash>
static inline int sparse_tree_create(gs_ctx *c, const char *who, const void *h, uint32_t depth, uint32_t digest, const void *empty_host, uint64_t slots_hint, Hash hash, gs_sparse **out) {
    if (!out) return GS_ERR_ARG;
    *out = nullptr;
    if (depth < 1 || depth > GS_SPARSE_MAX_DEPTH) return gs_fail(c, GS_ERR_ARG, "%s: a depth of 1 .. 36, not %u", who, depth);
    if (slots_hint < 1 || slots_hint > GS_SPARSE_MAX_SLOTS) return gs_fail(c, GS_ERR_ARG, "%s: slots_hint is 1 .. 2^31", who);
    void *store = nullptr, *empties = nullptr, *row = nullptr;
    int rc = gs_alloc(c, slots_hint * digest * GS_ELT, &store);
    if (!rc) rc = gs_alloc(c, (uint64_t)(depth + 1) * digest * GS_ELT, &empties);
    if (!rc) rc = gs_tmp_alloc(c, 2 * digest * GS_ELT, &row);
    fe *e = (fe *)empties;
    if (!rc) {
        if (empty_host) rc = gs_push(c, e, empty_host, digest * GS_ELT);
        else if (hipMemsetAsync(e, 0, digest * GS_ELT, c->stream) != hipSuccess) rc = gs_fail(c, GS_ERR_DEVICE, "%s: hipMemsetAsync failed", who);
    }
    for (uint32_t l = 0; l < depth && !rc; l++) {                            // the stream orders the copies and the launches: `row` is reused
        for (int side = 0; side < 2 && !rc; side++)
            if (hipMemcpyAsync((fe *)row + side * digest, e + (uint64_t)l * digest, digest * GS_ELT, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
                rc = gs_fail(c, GS_ERR_DEVICE, "%s: hipMemcpyAsync failed", who);
        if (!rc) rc = hash((const fe *)row, 1, e + (uint64_t)(l + 1) * digest);
    }
    if (row) gs_tmp_free(c, row);
    if (rc) {
        if (store) gs_free(c, store);
        if (empties) gs_free(c, empties);
        return rc;
    }
    *out = new gs_sparse{c, depth, digest, hash, h, sponge_serial(h), (fe *)store, slots_hint, e, sparse_tree_index(depth)};
    return GS_OK;
}

// indexes below 2^depth, the count within the cap: what update and paths share
static inline int sparse_tree_check_indexes(gs_ctx *c, const gs_sparse *t, const char *who, const uint64_t *indexes_host, uint64_t count, const char *what) {
    if (count > GS_TREE_UPDATE_MAX) return gs_fail(c, GS_ERR_ARG, "%s: at most 2^20 %s per call", who, what);
    if (!count) return GS_OK;
    if (!indexes_host) return GS_ERR_ARG;
    for (uint64_t j = 0; j < count; j++)
        if (indexes_host[j] >> t->depth)
            return gs_fail(c, GS_ERR_ARG, "%s: index %llu is outside of the 2^%u leaves", who, (unsigned long long)indexes_host[j], t->depth);
    return GS_OK;
}

// count >= 1 and the arguments have passed sparse_tree_check_indexes
static inline int sparse_tree_update_run(gs_ctx *c, gs_sparse *t, const uint64_t *indexes_host, const fe *leaves, uint64_t count, fe *before, fe *roots) {
    const char *who = "sparse_update";
    sparse_update_plan plan;
    if (!sparse_plan_update(t->index, indexes_host, count, plan)) return gs_fail(c, GS_ERR_ARG, "%s: the node store does not grow past 2^31 slots", who);
    if (!sparse_plan_update_in_bounds(plan)) return gs_fail(c, GS_ERR_ARG, "%s: a slot of the plan lies outside of the node store", who);
    int rc = sparse_tree_reserve(c, t, plan.slots_after, who);
    if (rc) return rc;
    const uint32_t depth = t->depth, digest = t->digest;
    const uint64_t level_elems = count * digest;
    // one scratch block: the plan, the rows of one level (reused: the stream orders the levels), the versions of levels 1 .. depth - 1
    const struct { const void *src; uint64_t bytes; } parts[] = {{indexes_host, count * 8},          {plan.plan.same.data(), count * 4}, {plan.plan.pred.data(), plan.plan.pred.size() * 4},
                                                                 {plan.sib.data(), plan.sib.size() * 4}, {plan.old.data(), count * 4},       {plan.write.data(), plan.write.size() * 4}};
    uint64_t off[7] = {0};
    for (int k = 0; k < 6; k++) off[k + 1] = off[k] + parts[k].bytes;      // (every part is a multiple of 4 bytes, the first of 8)
    const uint64_t fe_off = (off[6] + 31) & ~31ull;                          // elements start on a multiple of 32 bytes
    void *block = nullptr;
    if ((rc = gs_tmp_alloc(c, fe_off + (2 * level_elems + (uint64_t)(depth - 1) * level_elems) * GS_ELT, &block))) return rc;
    uint8_t *at = (uint8_t *)block;
    for (int k = 0; k < 6 && !rc; k++) rc = gs_push(c, at + off[k], parts[k].src, parts[k].bytes);
    const uint64_t *d_idx = (const uint64_t *)at;
    const int32_t *d_same = (const int32_t *)(at + off[1]), *d_pred = (const int32_t *)(at + off[2]);
    const uint32_t *d_sib = (const uint32_t *)(at + off[3]), *d_old = (const uint32_t *)(at + off[4]), *d_write = (const uint32_t *)(at + off[5]);
    fe *rows = (fe *)(at + fe_off), *mid = rows + 2 * level_elems;
    for (uint32_t l = 0; l < depth && !rc; l++) {
        const fe *ver_l = l ? mid + (uint64_t)(l - 1) * level_elems : leaves;
        fe *ver_up = l + 1 == depth ? roots : mid + (uint64_t)l * level_elems;
        if ((rc = sparse_tree_gather(c, t->store, t->empties, digest, depth, l, count, d_idx, d_same, d_pred + (uint64_t)l * count, d_sib + (uint64_t)l * count, d_old, ver_l,
                                     rows, before)))
            break;
        rc = t->hash((const fe *)rows, count, ver_up);
    }
    if (!rc) rc = sparse_tree_commit(c, t->store, digest, depth, count, d_write, leaves, mid, roots);
    gs_tmp_free(c, block);                                                   // (stream-ordered cache: the launches above still read it)
    if (!rc) sparse_plan_commit(t->index, plan);
    return rc;
}

static inline int sparse_tree_paths_run(gs_ctx *c, const gs_sparse *t, const uint64_t *indexes_host, uint64_t count, fe *out) {
    std::vector<uint32_t> slots;
    sparse_plan_paths(t->index, indexes_host, count, slots);
    if (!sparse_plan_slots_below(slots, t->index.slots)) return gs_fail(c, GS_ERR_ARG, "sparse_paths: a slot of the plan lies outside of the node store");
    void *d_slots = nullptr;
    int rc = gs_tmp_alloc(c, slots.size() * 4, &d_slots);
    if (rc) return rc;
    if ((rc = gs_push(c, d_slots, slots.data(), slots.size() * 4)) == GS_OK)
        rc = sparse_tree_path_gather(c, t->store, t->empties, t->digest, t->depth, count, (const uint32_t *)d_slots, out);
    gs_tmp_free(c, d_slots);                                                 // (stream-ordered cache: the launch above still reads it)
    return rc;
}
