// field_tree.hip — everything that reads and writes the nodes of a Merkle tree of field elements and knows no permutation
// (field_tree.h): it serves the Poseidon trees of hades.hip and the Rescue trees of rescue.hip alike.
//   paths    k_tree_paths behind gs_hades_merkle_paths — the name the entry was first exported with — reads nothing but a node array
//            in the heap layout.
//   updates  k_tree_update_gather / _commit and the driver of a batch (tree_update_run); the unit's hash launch comes in as a
//            tree_node_hash, so an updated node is the node the unit's tree build computes.
//   sparse   k_sparse_gather / _commit / _paths: the same with every read of the node array replaced by a read at a slot of a store;
//            a tree carries the tree_node_hash of the unit that created it (gs_hades_sparse_create, gs_rescue_sparse_create), every
//            other entry of include/gstark_sparse_tree.h is here.
// One thread per element, grid-stride, 64-bit indexes, plain loads and stores; no ordering but the stream's.
#include "field_tree.h"
#include "../../include/gstark_hades.h"
#include "../../include/gstark_sparse_tree.h"

// out[path][level][e]: the leaf (level 0), then the sibling on every level from the leaves up — of any tree in the heap layout
__global__ __launch_bounds__(256) void k_tree_paths(const fe *__restrict__ nodes, uint64_t n, uint32_t depth, uint32_t digest, const uint64_t *__restrict__ idx,
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

// one level of a batch of updates, of any tree in the heap layout: element e of update j's version ver_l[j] and of its sibling's
// value — the version of the update the plan names, or what the node array holds — land side by side in rows[j] in left/right order;
// the sibling is before[j][level + 1], and on level 0 the old leaf (the previous update of the same leaf, or the node array) is
// before[j][0].  Reads of the node array only: the commit writes it, after the last level.
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

// ---- sparse trees: the three kernels above with every read of the node array replaced by a read at a slot of the node store, or of
// empties[level] where the host found no slot (GS_SPARSE_EMPTY).  Slots have been checked against the store on the host.
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

namespace {

// level l of a batch: rows[j] = (left, right) of update j's node pair, before[j][l + 1] = the sibling (and before[j][0] = the old leaf
// on level 0); ver_l = ver[l]; pred (and sib): the plan's whole array, row l is read
int tree_update_gather(gs_ctx *c, const fe *nodes, uint64_t n, uint32_t digest, uint32_t depth, uint32_t level, uint64_t count, const uint64_t *idx, const int32_t *same,
                       const int32_t *pred, const fe *ver_l, fe *rows, fe *before) {
    const uint64_t total = count * digest;
    gs_traffic(c, (5 * total + (level ? 0 : 2 * total)) * GS_ELT + count * 12, 0, "k_tree_update_gather");
    hipLaunchKernelGGL(k_tree_update_gather, dim3(gs_grid(total)), dim3(256), 0, c->stream, nodes, n, digest, depth, level, total, idx, same, pred + (uint64_t)level * count,
                       ver_l, rows, before);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int sparse_tree_gather(gs_ctx *c, const fe *store, const fe *empties, uint32_t digest, uint32_t depth, uint32_t level, uint64_t count, const uint64_t *idx,
                       const int32_t *same, const int32_t *pred, const uint32_t *sib, const uint32_t *old, const fe *ver_l, fe *rows, fe *before) {
    const uint64_t total = count * digest;
    gs_traffic(c, (5 * total + (level ? 0 : 2 * total)) * GS_ELT + count * 16 + (level ? 0 : count * 8), 0, "k_sparse_gather");
    hipLaunchKernelGGL(k_sparse_gather, dim3(gs_grid(total)), dim3(256), 0, c->stream, store, empties, digest, depth, level, total, idx, same,
                       pred + (uint64_t)level * count, sib + (uint64_t)level * count, old, ver_l, rows, before);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

// nodes[(n + idx[j]) >> l] = ver[l][j] wherever last[l][j]: ver[0] = leaves, ver[1 .. depth - 1] = mid, ver[depth] = roots
int tree_update_commit(gs_ctx *c, fe *nodes, uint64_t n, uint32_t digest, uint32_t depth, uint64_t count, const uint64_t *idx, const uint8_t *last, const fe *leaves,
                       const fe *mid, const fe *roots) {
    const uint64_t total = (uint64_t)(depth + 1) * count * digest;
    gs_traffic(c, 2 * total * GS_ELT + (uint64_t)(depth + 1) * count, 0, "k_tree_update_commit");
    hipLaunchKernelGGL(k_tree_update_commit, dim3(gs_grid(total)), dim3(256), 0, c->stream, nodes, n, digest, depth, count, total, idx, last, leaves, mid, roots);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

// store[write[l][j]] = ver[l][j] wherever write[l][j] is a slot
int sparse_tree_commit(gs_ctx *c, fe *store, uint32_t digest, uint32_t depth, uint64_t count, const uint32_t *write, const fe *leaves, const fe *mid, const fe *roots) {
    const uint64_t total = (uint64_t)(depth + 1) * count * digest;
    gs_traffic(c, 2 * total * GS_ELT + (uint64_t)(depth + 1) * count * 4, 0, "k_sparse_commit");
    hipLaunchKernelGGL(k_sparse_commit, dim3(gs_grid(total)), dim3(256), 0, c->stream, store, digest, depth, count, total, write, leaves, mid, roots);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

// out[k][l] = store[slots[k][l]], or the empty node of that place: empties[0] for the leaf, empties[l - 1] for the sibling on level l - 1
int sparse_tree_path_gather(gs_ctx *c, const fe *store, const fe *empties, uint32_t digest, uint32_t depth, uint64_t count, const uint32_t *slots, fe *out) {
    const uint64_t total = count * (depth + 1) * digest;
    gs_traffic(c, 2 * total * GS_ELT + count * (depth + 1) * 4, 0, "k_sparse_paths");
    hipLaunchKernelGGL(k_sparse_paths, dim3(gs_grid(total)), dim3(256), 0, c->stream, store, empties, depth, digest, slots, total, out);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

// A batch of `count` updates over `depth` levels, dense or sparse.  One scratch block holds the host parts of the plan one after the
// other, then — from a multiple of 32 bytes — the rows of one level (reused: the stream orders the levels) and the versions of levels
// 1 .. depth - 1.  gather(parts, l, ver_l, rows) enqueues level l's gather and commit(parts, mid) the commit, parts[k] being the device
// copy of part k.  Nothing after a failed enqueue is enqueued; the block is freed on every path.
#define GS_TREE_BATCH_PARTS 6
template <class Gather, class Commit>
int tree_batch_run(gs_ctx *c, std::initializer_list<sponge_part> parts, uint64_t count, uint32_t digest, uint32_t depth, const fe *leaves, fe *roots, Gather gather,
                   const tree_node_hash &hash, Commit commit) {
    const uint64_t level_elems = count * digest;
    uint64_t off[GS_TREE_BATCH_PARTS + 1] = {0};
    int k = 0;
    for (const sponge_part &part : parts) { off[k + 1] = off[k] + part.bytes; k++; }      // (the 8-byte items come first, single bytes last: every part is aligned)
    const uint64_t fe_off = (off[k] + 31) & ~31ull;
    void *block = nullptr;
    int rc = gs_tmp_alloc(c, fe_off + (2 * level_elems + (uint64_t)(depth - 1) * level_elems) * GS_ELT, &block);
    if (rc) return rc;
    uint8_t *at = (uint8_t *)block;
    const void *dev[GS_TREE_BATCH_PARTS];
    k = 0;
    for (const sponge_part &part : parts) {
        dev[k] = at + off[k];
        if (!rc) rc = gs_push(c, at + off[k], part.host, part.bytes);
        k++;
    }
    fe *rows = (fe *)(at + fe_off), *mid = rows + 2 * level_elems;
    for (uint32_t l = 0; l < depth && !rc; l++) {
        const fe *ver_l = l ? mid + (uint64_t)(l - 1) * level_elems : leaves;
        fe *ver_up = l + 1 == depth ? roots : mid + (uint64_t)l * level_elems;
        if ((rc = gather(dev, l, ver_l, rows))) break;
        rc = hash.run(c, hash.handle, digest, rows, count, ver_up);
    }
    if (!rc) rc = commit(dev, (const fe *)mid);
    gs_tmp_free(c, block);                                                   // (stream-ordered cache: the launches above still read it)
    return rc;
}

int sparse_tree_check_handle(gs_ctx *c, const gs_sparse *t, const char *who) {
    if (!c || !t) return GS_ERR_ARG;
    if (t->ctx != c) return gs_fail(c, GS_ERR_ARG, "%s: the tree belongs to another context", who);
    // the tree holds the hash handle's pointer: a call after gs_*_destroy of the hash would read freed memory and launch over freed constants
    return sponge_serial(t->hash.handle) == t->hash_serial ? GS_OK : gs_fail(c, GS_ERR_ARG, "%s: the tree's hash has been destroyed", who);
}

// the store holds at least `slots` slots: doubling, one device copy of what is in use
int sparse_tree_reserve(gs_ctx *c, gs_sparse *t, uint64_t slots, const char *who) {
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

// indexes below 2^depth, the count within the cap: what update and paths share
int sparse_tree_check_indexes(gs_ctx *c, const gs_sparse *t, const char *who, const uint64_t *indexes_host, uint64_t count, const char *what) {
    if (count > GS_TREE_UPDATE_MAX) return gs_fail(c, GS_ERR_ARG, "%s: at most 2^20 %s per call", who, what);
    if (!count) return GS_OK;
    if (!indexes_host) return GS_ERR_ARG;
    for (uint64_t j = 0; j < count; j++)
        if (indexes_host[j] >> t->depth)
            return gs_fail(c, GS_ERR_ARG, "%s: index %llu is outside of the 2^%u leaves", who, (unsigned long long)indexes_host[j], t->depth);
    return GS_OK;
}

// count >= 1 and the arguments have passed sparse_tree_check_indexes
int sparse_tree_update_run(gs_ctx *c, gs_sparse *t, const uint64_t *indexes_host, const fe *leaves, uint64_t count, fe *before, fe *roots) {
    const char *who = "sparse_update";
    sparse_update_plan plan;
    if (!sparse_plan_update(t->index, indexes_host, count, plan)) return gs_fail(c, GS_ERR_ARG, "%s: the node store does not grow past 2^31 slots", who);
    if (!sparse_plan_update_in_bounds(plan)) return gs_fail(c, GS_ERR_ARG, "%s: a slot of the plan lies outside of the node store", who);
    int rc = sparse_tree_reserve(c, t, plan.slots_after, who);
    if (rc) return rc;
    const uint32_t depth = t->depth, digest = t->digest;
    rc = tree_batch_run(
        c, {{indexes_host, count * 8},          {plan.plan.same.data(), count * 4}, {plan.plan.pred.data(), plan.plan.pred.size() * 4},
            {plan.sib.data(), plan.sib.size() * 4}, {plan.old.data(), count * 4},       {plan.write.data(), plan.write.size() * 4}},
        count, digest, depth, leaves, roots,
        [&](const void *const *d, uint32_t l, const fe *ver_l, fe *rows) {
            return sparse_tree_gather(c, t->store, t->empties, digest, depth, l, count, (const uint64_t *)d[0], (const int32_t *)d[1], (const int32_t *)d[2],
                                      (const uint32_t *)d[3], (const uint32_t *)d[4], ver_l, rows, before);
        },
        t->hash, [&](const void *const *d, const fe *mid) { return sparse_tree_commit(c, t->store, digest, depth, count, (const uint32_t *)d[5], leaves, mid, roots); });
    if (!rc) sparse_plan_commit(t->index, plan);
    return rc;
}

}  // namespace

int tree_update_check(gs_ctx *c, const char *who, uint64_t n, uint64_t count, const uint64_t *indexes_host, const void *nodes, const void *leaves, const void *before,
                      const void *roots) {
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

int tree_update_run(gs_ctx *c, fe *nodes, uint64_t n, uint32_t digest, const uint64_t *indexes_host, const fe *leaves, uint64_t count, fe *before, fe *roots,
                    const tree_node_hash &hash) {
    tree_update_plan plan;
    tree_update_plan_build(n, indexes_host, count, plan);
    const uint32_t depth = plan.depth;
    return tree_batch_run(
        c, {{indexes_host, count * 8}, {plan.same.data(), count * 4}, {plan.pred.data(), plan.pred.size() * 4}, {plan.last.data(), plan.last.size()}}, count, digest, depth,
        leaves, roots,
        [&](const void *const *d, uint32_t l, const fe *ver_l, fe *rows) {
            return tree_update_gather(c, nodes, n, digest, depth, l, count, (const uint64_t *)d[0], (const int32_t *)d[1], (const int32_t *)d[2], ver_l, rows, before);
        },
        hash, [&](const void *const *d, const fe *mid) { return tree_update_commit(c, nodes, n, digest, depth, count, (const uint64_t *)d[0], (const uint8_t *)d[3], leaves, mid, roots); });
}

int sparse_tree_create(gs_ctx *c, const char *who, const tree_node_hash &hash, uint32_t depth, uint32_t digest, const void *empty_host, uint64_t slots_hint, gs_sparse **out) {
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
        if (!rc) rc = hash.run(c, hash.handle, digest, (const fe *)row, 1, e + (uint64_t)(l + 1) * digest);
    }
    if (row) gs_tmp_free(c, row);
    if (rc) {
        if (store) gs_free(c, store);
        if (empties) gs_free(c, empties);
        return rc;
    }
    *out = new gs_sparse{c, depth, digest, hash, sponge_serial(hash.handle), (fe *)store, slots_hint, e, sparse_tree_index(depth)};
    return GS_OK;
}

extern "C" {

int gs_hades_merkle_paths(gs_ctx *c, const void *nodes, uint64_t n, uint32_t digest, const uint64_t *indexes_host, uint64_t count, void *out) {
    if (!c) return GS_ERR_ARG;
    const int rc = sponge_check_leaves(c, "hades_merkle_paths", n);
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
    return sponge_with_upload(c, indexes_host, count * 8, [&](const void *idx) {
        hipLaunchKernelGGL(k_tree_paths, dim3(gs_grid(total)), dim3(256), 0, c->stream, (const fe *)nodes, n, depth, digest, (const uint64_t *)idx, total, (fe *)out);
        return hipGetLastError() == hipSuccess ? (int)GS_OK : gs_fail(c, GS_ERR_DEVICE, "hades_merkle_paths: launch failed");      // (the entry's own text, not GS_LAUNCH_CHECK's)
    });
}

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
    std::vector<uint32_t> slots;
    sparse_plan_paths(t->index, indexes_host, count, slots);
    if (!sparse_plan_slots_below(slots, t->index.slots)) return gs_fail(c, GS_ERR_ARG, "sparse_paths: a slot of the plan lies outside of the node store");
    return sponge_with_upload(c, slots.data(), slots.size() * 4,
                              [&](const void *d_slots) { return sparse_tree_path_gather(c, t->store, t->empties, t->digest, t->depth, count, (const uint32_t *)d_slots, (fe *)out); });
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

}  // extern "C"
