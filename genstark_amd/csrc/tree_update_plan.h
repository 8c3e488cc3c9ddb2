// tree_update_plan.h — who reads whom when a batch of leaf updates is applied to a heap-layout Merkle tree level by level
// (tree_update.h is the device side; DESIGN.md "Batched tree updates" has the argument).  Plain C++, no HIP: it is tested on its own
// (tests/host_harness/tree_update_plan_host.cpp).
//   Update j sets leaf indexes[j]; anc(j, l) = (n + indexes[j]) >> l is the node it passes on level l.  Per (level, update) the plan
//   names the update whose version of the SIBLING node update j sees: the latest i < j with anc(i, l) == anc(j, l) ^ 1, or -1 where
//   the sibling still holds what the node array holds.  `same` is the previous update of the same leaf (its new leaf is this one's old
//   leaf), `last` flags the latest update that passes a node: the one whose version the node array ends with.
//   The work is O(count * depth) and no allocation depends on n: the updates are sorted by leaf once (stable, so call order survives
//   inside a leaf), and on every level the lists of two sibling nodes — each ascending in update number — are merged into their
//   parent's list.  While merging, an element's predecessor is the last element taken from the OTHER list; the merged list's tail is
//   the node's latest toucher.
#pragma once
#include <cstdint>
#include <vector>

struct tree_update_plan {
    uint32_t depth = 0;                      // log2 n
    uint64_t count = 0;
    std::vector<int32_t> pred;               // depth x count, level-major: the update whose version of the sibling is read, -1: the node array
    std::vector<int32_t> same;               // count: the previous update of the same leaf, -1: none
    std::vector<uint8_t> last;               // (depth + 1) x count, level-major: 1 where the update is the latest one through its node
};

#define GS_TREE_UPDATE_MAX (1ull << 20)     // updates per plan: update numbers fit an int32_t with room to spare

// n: a power of two >= 2; indexes[j] < n; count <= GS_TREE_UPDATE_MAX (the caller has checked all three)
static inline void tree_update_plan_build(uint64_t n, const uint64_t *indexes, uint64_t count, tree_update_plan &plan) {
    uint32_t depth = 0;
    while ((1ull << depth) < n) depth++;
    plan.depth = depth;
    plan.count = count;
    plan.pred.assign((uint64_t)depth * count, -1);
    plan.same.assign(count, -1);
    plan.last.assign((uint64_t)(depth + 1) * count, 0);
    if (!count) return;

    // update numbers by leaf, call order inside a leaf: a stable radix sort, one pass per 8 bits of the index
    std::vector<int32_t> order(count), other(count);
    for (uint64_t j = 0; j < count; j++) order[j] = (int32_t)j;
    for (uint32_t shift = 0; shift < depth; shift += 8) {
        uint64_t at[257] = {0};
        for (uint64_t k = 0; k < count; k++) at[((indexes[order[k]] >> shift) & 0xff) + 1]++;
        for (int b = 0; b < 256; b++) at[b + 1] += at[b];
        for (uint64_t k = 0; k < count; k++) other[at[(indexes[order[k]] >> shift) & 0xff]++] = order[k];
        order.swap(other);
    }

    // `order` holds one ascending list per touched node of the level, the nodes ascending; start[g] .. start[g + 1] is list g
    std::vector<uint64_t> start, next_start;
    for (uint64_t k = 0; k < count; k++) {
        if (k && indexes[order[k]] == indexes[order[k - 1]]) plan.same[order[k]] = order[k - 1];
        else start.push_back(k);
    }
    start.push_back(count);

    for (uint32_t l = 0; l < depth; l++) {
        int32_t *pred = plan.pred.data() + (uint64_t)l * count;
        uint8_t *last = plan.last.data() + (uint64_t)l * count;
        next_start.clear();
        const uint64_t groups = start.size() - 1;
        for (uint64_t g = 0; g < groups;) {
            const uint64_t lo = start[g], mid = start[g + 1];
            const uint64_t node = (n + indexes[order[lo]]) >> l;
            last[order[mid - 1]] = 1;
            next_start.push_back(lo);
            const bool pair = !(node & 1) && g + 1 < groups && ((n + indexes[order[mid]]) >> l) == node + 1;
            if (!pair) {                                                     // the sibling is untouched: every pred stays -1
                for (uint64_t k = lo; k < mid; k++) other[k] = order[k];
                g += 1;
                continue;
            }
            const uint64_t hi = start[g + 2];
            last[order[hi - 1]] = 1;
            uint64_t x = lo, y = mid, out = lo;
            int32_t last_left = -1, last_right = -1;
            while (x < mid || y < hi) {
                if (y == hi || (x < mid && order[x] < order[y])) {
                    pred[order[x]] = last_right;
                    last_left = order[x];
                    other[out++] = order[x++];
                } else {
                    pred[order[y]] = last_left;
                    last_right = order[y];
                    other[out++] = order[y++];
                }
            }
            g += 2;
        }
        next_start.push_back(count);
        order.swap(other);
        start.swap(next_start);
    }
    plan.last[(uint64_t)depth * count + order[count - 1]] = 1;              // the root: one list, every update, the last one wins
}
