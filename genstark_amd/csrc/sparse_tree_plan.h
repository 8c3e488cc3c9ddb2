// sparse_tree_plan.h — where the nodes of a sparse Merkle tree of fixed depth live: the host index of a device node store and the slots
// a batch of updates or of paths reads and writes (sparse_tree.h is the device side; DESIGN.md "Sparse trees" has the argument).
// Plain C++, no HIP: it is tested on its own (tests/host_harness/sparse_tree_plan_host.cpp).
//   The tree IS the dense heap tree of 2^depth leaves (depth 1 .. 36) whose leaves all hold one `empty` value until they are set.  A
//   node whose whole subtree is empty is not stored: it is empties[level].  A stored node has a SLOT in an append-only store and keeps it
//   for life; per level 0 .. depth the index maps the node's number on that level (leaf index >> level) to its slot.  A stored leaf costs
//   up to `depth` stored nodes (its ancestors below the root, shared with its neighbours) and as many index entries.
//   tree_update_plan_build says, per (level, update), whose version of the sibling is read (`pred`), the previous update of the same
//   leaf (`same`) and the latest toucher of every node (`last`).  Here every read the plan leaves to the node array, and every write of
//   a latest toucher, is resolved to a slot:
//     sib[l][j]    where pred[l][j] == -1: the slot of the sibling of update j's node on level l, or GS_SPARSE_EMPTY
//     old[j]       where same[j] == -1: the slot of the leaf as it stood at the call, or GS_SPARSE_EMPTY
//     write[l][j]  where last[l][j]: the slot the version is committed to — the node's own, or a fresh one; GS_SPARSE_EMPTY elsewhere
//   Fresh slots are handed out level by level from the leaves up and in update order inside a level: the order depends on nothing but
//   the call.  The index itself is NOT changed by the resolution: sparse_plan_commit inserts the fresh nodes once every launch of the
//   call has been enqueued, so a refused or failed call leaves the tree as it was.
#pragma once
#include <cstdint>
#include <vector>

#include "tree_update_plan.h"

#define GS_SPARSE_EMPTY 0xffffffffu           // "no slot": the node is empties[level]
#define GS_SPARSE_MAX_DEPTH 36u
#define GS_SPARSE_MAX_SLOTS (1ull << 31)      // slots of a store: slot numbers fit 32 bits with GS_SPARSE_EMPTY to spare

// node number -> slot: open addressing, linear probing, no deletion (nothing is ever pruned); grows at half full.  Key and slot share
// an entry, so a probe of a large map is one cache miss, and prefetch() lets a loop over a batch have several of them in flight
struct sparse_level_map {
    struct entry { uint64_t key; uint32_t slot; };      // key: node + 1; 0: free
    std::vector<entry> table;
    uint64_t used = 0;

    static uint64_t mix(uint64_t x) {
        x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
        x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
        return x ^ (x >> 33);
    }
    void prefetch(uint64_t node) const {
        if (!table.empty()) __builtin_prefetch(&table[mix(node) & (table.size() - 1)]);
    }
    uint32_t find(uint64_t node) const {
        if (table.empty()) return GS_SPARSE_EMPTY;
        const uint64_t mask = table.size() - 1;
        for (uint64_t at = mix(node) & mask;; at = (at + 1) & mask) {
            if (table[at].key == node + 1) return table[at].slot;
            if (!table[at].key) return GS_SPARSE_EMPTY;
        }
    }
    void place(uint64_t node, uint32_t slot) {
        const uint64_t mask = table.size() - 1;
        uint64_t at = mix(node) & mask;
        while (table[at].key) at = (at + 1) & mask;
        table[at] = {node + 1, slot};
    }
    void insert(uint64_t node, uint32_t slot) {     // the node is not in the map
        if (2 * (used + 1) > table.size()) {
            std::vector<entry> old(table.empty() ? 16 : 2 * table.size(), entry{0, 0});
            old.swap(table);
            for (const entry &e : old)
                if (e.key) place(e.key - 1, e.slot);
        }
        place(node, slot);
        used++;
    }
};

#define GS_SPARSE_PREFETCH 16                 // probes in flight: the batch is walked this many updates ahead of its lookups

struct sparse_tree_index {
    uint32_t depth = 0;
    uint64_t slots = 0;                       // slots handed out so far: the next fresh one
    std::vector<sparse_level_map> level;      // depth + 1 maps; level[depth] holds at most node 0, the root
    explicit sparse_tree_index(uint32_t d = 0) : depth(d), level(d + 1) {}
};

struct sparse_fresh { uint32_t level; uint32_t slot; uint64_t node; };

struct sparse_update_plan {
    tree_update_plan plan;
    std::vector<uint32_t> sib;                // depth x count, level-major
    std::vector<uint32_t> old;                // count
    std::vector<uint32_t> write;              // (depth + 1) x count, level-major
    std::vector<sparse_fresh> fresh;          // the nodes this call stores for the first time, in slot order
    uint64_t slots_after = 0;                 // what the store must hold before the first launch
};

// indexes[j] < 2^depth, count <= GS_TREE_UPDATE_MAX (the caller has checked both).  false: the store would pass GS_SPARSE_MAX_SLOTS
static inline bool sparse_plan_update(const sparse_tree_index &index, const uint64_t *indexes, uint64_t count, sparse_update_plan &out) {
    const uint32_t depth = index.depth;
    tree_update_plan_build(1ull << depth, indexes, count, out.plan);
    out.sib.assign((uint64_t)depth * count, GS_SPARSE_EMPTY);
    out.old.assign(count, GS_SPARSE_EMPTY);
    out.write.assign((uint64_t)(depth + 1) * count, GS_SPARSE_EMPTY);
    out.fresh.clear();
    uint64_t next = index.slots;
    for (uint64_t j = 0; j < count; j++)
        if (out.plan.same[j] < 0) out.old[j] = index.level[0].find(indexes[j]);
    for (uint32_t l = 0; l <= depth; l++) {
        const sparse_level_map &map = index.level[l];
        for (uint64_t j = 0; j < count; j++) {
            if (j + GS_SPARSE_PREFETCH < count) {
                map.prefetch(indexes[j + GS_SPARSE_PREFETCH] >> l);
                map.prefetch((indexes[j + GS_SPARSE_PREFETCH] >> l) ^ 1);
            }
            const uint64_t at = (uint64_t)l * count + j, node = indexes[j] >> l;
            if (l < depth && out.plan.pred[at] < 0) out.sib[at] = map.find(node ^ 1);
            if (!out.plan.last[at]) continue;
            uint32_t slot = map.find(node);
            if (slot == GS_SPARSE_EMPTY) {
                if (next >= GS_SPARSE_MAX_SLOTS) return false;
                slot = (uint32_t)next++;
                out.fresh.push_back({l, slot, node});
            }
            out.write[at] = slot;
        }
    }
    out.slots_after = next;
    return true;
}

// every slot the kernels of the call will read or write lies inside a store of `slots` slots
static inline bool sparse_plan_slots_below(const std::vector<uint32_t> &slots_of, uint64_t slots) {
    for (const uint32_t s : slots_of)
        if (s != GS_SPARSE_EMPTY && s >= slots) return false;
    return true;
}
static inline bool sparse_plan_update_in_bounds(const sparse_update_plan &p) {
    return sparse_plan_slots_below(p.sib, p.slots_after) && sparse_plan_slots_below(p.old, p.slots_after) && sparse_plan_slots_below(p.write, p.slots_after);
}

// after the last launch of the call has been enqueued: the fresh nodes enter the index
static inline void sparse_plan_commit(sparse_tree_index &index, const sparse_update_plan &p) {
    for (const sparse_fresh &f : p.fresh) index.level[f.level].insert(f.node, f.slot);
    index.slots = p.slots_after;
}

// out[k][0] = the slot of leaf indexes[k], out[k][l + 1] = the slot of its sibling on level l: (depth + 1) x count, path-major
static inline void sparse_plan_paths(const sparse_tree_index &index, const uint64_t *indexes, uint64_t count, std::vector<uint32_t> &out) {
    const uint32_t depth = index.depth, per = depth + 1;
    out.assign((uint64_t)per * count, GS_SPARSE_EMPTY);
    for (uint32_t l = 0; l < depth; l++) {                                   // level by level: one map at a time, its probes prefetched
        const sparse_level_map &map = index.level[l];
        for (uint64_t k = 0; k < count; k++) {
            if (k + GS_SPARSE_PREFETCH < count) {
                map.prefetch((indexes[k + GS_SPARSE_PREFETCH] >> l) ^ 1);
                if (!l) map.prefetch(indexes[k + GS_SPARSE_PREFETCH]);
            }
            if (!l) out[k * per] = map.find(indexes[k]);
            out[k * per + l + 1] = map.find((indexes[k] >> l) ^ 1);
        }
    }
}

// the slot of the root, or GS_SPARSE_EMPTY while nothing is stored
static inline uint32_t sparse_plan_root(const sparse_tree_index &index) { return index.level[index.depth].find(0); }
