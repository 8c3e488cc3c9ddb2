// sparse_tree_plan_host.cpp — genstark_amd/csrc/sparse_tree_plan.h on its own (tests/test_sparse_tree.py compiles this with
// -fsanitize=address,undefined and runs it).  A tree is a sequence of calls; per call
//   1. the slot resolution is held against a brute-force model, a std::map per level from node number to slot: every read the plan leaves
//      to the store (pred == -1, same == -1) names the model's slot or GS_SPARSE_EMPTY, every latest toucher writes the model's slot or a
//      fresh one, fresh slots are handed out exactly once, in the order the header states, and every slot is below the slot count;
//   2. the scheme the device runs with that plan — versions, siblings by predecessor / slot / empties, commit by slot — is run on a store
//      of 64-bit values under a mixing function that stands for the hash, against updates applied one at a time to a map model of the
//      dense tree of 2^depth leaves with `empty` at every index never set; then the paths of touched and untouched indexes, and the root.
// Depths 1, 2, 5 and 36; batches: repeated indexes, sibling pairs in both orders, the same leaf many times, indexes with bits 32 .. 35
// set, siblings created later in the batch, and several calls in a row so that slots carry over; and the refusal to pass 2^31 slots.  Prints "sparse tree plan: <calls> calls ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "../../genstark_amd/csrc/sparse_tree_plan.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                      // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

static uint64_t node_hash(uint64_t left, uint64_t right) {
    uint64_t x = left * 0xff51afd7ed558ccdull + (right ^ 0xc4ceb9fe1a85ec53ull) * 0x9fb21c651e98df25ull;
    x ^= x >> 29;
    return x * 0xbf58476d1ce4e5b9ull + left + 3 * right;
}

#define FAIL(...)                                  \
    do {                                           \
        std::fprintf(stderr, __VA_ARGS__);         \
        std::fprintf(stderr, " (depth = %u, k = %llu)\n", d, (unsigned long long)k); \
        std::exit(1);                              \
    } while (0)

struct Tree {
    uint32_t d;
    sparse_tree_index index;
    std::vector<std::map<uint64_t, uint32_t>> slot_of;       // the brute-force index
    std::vector<std::map<uint64_t, uint64_t>> value;         // the dense tree's nodes that differ from empties, per level
    std::vector<uint64_t> empties, store;
    std::set<uint32_t> handed;

    explicit Tree(uint32_t depth, uint64_t empty) : d(depth), index(depth), slot_of(depth + 1), value(depth + 1), empties(depth + 1) {
        empties[0] = empty;
        for (uint32_t l = 0; l < depth; l++) empties[l + 1] = node_hash(empties[l], empties[l]);
    }
    uint64_t get(uint32_t l, uint64_t node) const {
        auto it = value[l].find(node);
        return it == value[l].end() ? empties[l] : it->second;
    }
    uint64_t read(uint32_t l, uint32_t slot) const { return slot == GS_SPARSE_EMPTY ? empties[l] : store[slot]; }

    void update(const std::vector<uint64_t> &idx) {
        const uint64_t k = idx.size();
        sparse_update_plan p;
        if (!sparse_plan_update(index, idx.data(), k, p)) FAIL("the plan refuses");
        if (!sparse_plan_update_in_bounds(p)) FAIL("a slot out of bounds");
        if (p.sib.size() != d * k || p.old.size() != k || p.write.size() != (d + 1) * k) FAIL("plan sizes");

        // 1. the resolution against the maps
        uint64_t next = index.slots;
        size_t fresh_at = 0;
        for (uint32_t l = 0; l <= d; l++)
            for (uint64_t j = 0; j < k; j++) {
                const uint64_t at = l * k + j, node = idx[j] >> l;
                if (l < d) {
                    auto it = slot_of[l].find(node ^ 1);
                    const uint32_t want = p.plan.pred[at] >= 0 || it == slot_of[l].end() ? GS_SPARSE_EMPTY : it->second;
                    if (p.sib[at] != want) FAIL("sib[%u][%llu] = %u, not %u", l, (unsigned long long)j, p.sib[at], want);
                }
                if (l == 0) {
                    auto it = slot_of[0].find(node);
                    const uint32_t want = p.plan.same[j] >= 0 || it == slot_of[0].end() ? GS_SPARSE_EMPTY : it->second;
                    if (p.old[j] != want) FAIL("old[%llu] = %u, not %u", (unsigned long long)j, p.old[j], want);
                }
                if (!p.plan.last[at]) {
                    if (p.write[at] != GS_SPARSE_EMPTY) FAIL("write[%u][%llu] set for an update that is not the last", l, (unsigned long long)j);
                    continue;
                }
                auto it = slot_of[l].find(node);
                if (it != slot_of[l].end()) {
                    if (p.write[at] != it->second) FAIL("write[%u][%llu] = %u, not the node's slot %u", l, (unsigned long long)j, p.write[at], it->second);
                } else {
                    if (p.write[at] != next) FAIL("write[%u][%llu] = %u, not the fresh slot %llu", l, (unsigned long long)j, p.write[at], (unsigned long long)next);
                    if (fresh_at >= p.fresh.size() || p.fresh[fresh_at].level != l || p.fresh[fresh_at].node != node || p.fresh[fresh_at].slot != next) FAIL("fresh list");
                    if (!handed.insert((uint32_t)next).second) FAIL("slot %llu handed out twice", (unsigned long long)next);
                    slot_of[l][node] = (uint32_t)next++;
                    fresh_at++;
                }
                if (p.write[at] >= p.slots_after) FAIL("write slot beyond the store");
            }
        if (fresh_at != p.fresh.size() || next != p.slots_after) FAIL("fresh count");

        // 2. the device scheme against one update at a time
        std::vector<uint64_t> leaves(k), seq_before(k * (d + 1)), seq_roots(k);
        for (uint64_t j = 0; j < k; j++) leaves[j] = (j % 7 == 3) ? get(0, idx[j]) : ((j % 11 == 5) ? empties[0] : rnd());
        for (uint64_t j = 0; j < k; j++) {
            seq_before[j * (d + 1)] = get(0, idx[j]);
            for (uint32_t l = 0; l < d; l++) seq_before[j * (d + 1) + l + 1] = get(l, (idx[j] >> l) ^ 1);
            value[0][idx[j]] = leaves[j];
            for (uint32_t l = 0; l < d; l++) {
                const uint64_t node = idx[j] >> l;
                value[l + 1][node >> 1] = node_hash(get(l, node & ~1ull), get(l, node | 1));
            }
            seq_roots[j] = get(d, 0);
        }
        store.resize(p.slots_after, 0xDEADBEEFull);                          // "grown": fresh slots hold nothing yet
        std::vector<uint64_t> ver((d + 1) * k), before(k * (d + 1));
        for (uint64_t j = 0; j < k; j++) {
            ver[j] = leaves[j];
            before[j * (d + 1)] = p.plan.same[j] >= 0 ? leaves[p.plan.same[j]] : read(0, p.old[j]);
        }
        for (uint32_t l = 0; l < d; l++)
            for (uint64_t j = 0; j < k; j++) {
                const int32_t pr = p.plan.pred[l * k + j];
                const uint64_t sibling = pr >= 0 ? ver[l * k + pr] : read(l, p.sib[l * k + j]), mine = ver[l * k + j];
                before[j * (d + 1) + l + 1] = sibling;
                ver[(l + 1) * k + j] = ((idx[j] >> l) & 1) ? node_hash(sibling, mine) : node_hash(mine, sibling);
            }
        for (uint64_t at = 0; at < (d + 1) * k; at++)
            if (p.write[at] != GS_SPARSE_EMPTY) store[p.write[at]] = ver[at];
        sparse_plan_commit(index, p);
        if (before != seq_before) FAIL("witnesses differ");
        for (uint64_t j = 0; j < k; j++)
            if (ver[d * k + j] != seq_roots[j]) FAIL("root %llu differs", (unsigned long long)j);
        if (index.slots != next) FAIL("slot count after the commit");
        for (uint32_t l = 0; l <= d; l++) {
            if (index.level[l].used != slot_of[l].size()) FAIL("stored nodes on level %u", l);
            for (const auto &kv : slot_of[l]) {
                if (index.level[l].find(kv.first) != kv.second) FAIL("index entry on level %u", l);
                if (store[kv.second] != get(l, kv.first)) FAIL("stored value on level %u", l);
            }
        }
        paths(idx);
    }

    void paths(std::vector<uint64_t> idx) {
        const uint64_t mask = (1ull << d) - 1;
        for (int extra = 0; extra < 8; extra++) idx.push_back(rnd() & mask);        // mostly never set
        idx.push_back(0);
        idx.push_back(mask);
        const uint64_t k = idx.size();
        std::vector<uint32_t> slots;
        sparse_plan_paths(index, idx.data(), k, slots);
        if (slots.size() != k * (d + 1) || !sparse_plan_slots_below(slots, index.slots)) FAIL("path slots");
        for (uint64_t j = 0; j < k; j++) {
            if (read(0, slots[j * (d + 1)]) != get(0, idx[j])) FAIL("leaf of path %llu", (unsigned long long)j);
            for (uint32_t l = 0; l < d; l++)
                if (read(l, slots[j * (d + 1) + l + 1]) != get(l, (idx[j] >> l) ^ 1)) FAIL("sibling %u of path %llu", l, (unsigned long long)j);
        }
        if (read(d, sparse_plan_root(index)) != get(d, 0)) FAIL("root");
    }
};

int main() {
    unsigned calls = 0;
    const uint32_t depths[] = {1, 2, 5, 36};
    for (const uint32_t d : depths) {
        const uint64_t mask = (1ull << d) - 1;
        for (int variant = 0; variant < 3; variant++) {
            Tree tree(d, variant ? rnd() : 0);
            std::vector<uint64_t> idx;
            tree.paths(idx), calls++;                                        // nothing stored: every path is empties
            // a sibling pair, the right one first, then both again in the other order, in one batch
            const uint64_t pair = rnd() & mask & ~1ull;
            idx = {pair | 1, pair, pair, pair | 1};
            tree.update(idx), calls++;
            // the same leaf many times
            idx.assign(37, rnd() & mask);
            tree.update(idx), calls++;
            // all new, with siblings created later in the batch: 2i before 2i + 1 and the reverse
            idx.clear();
            for (int i = 0; i < 20; i++) {
                const uint64_t a = rnd() & mask & ~1ull;
                idx.push_back(i & 1 ? a : a | 1);
                idx.push_back(rnd() & mask);
                idx.push_back(i & 1 ? a | 1 : a);
            }
            tree.update(idx), calls++;
            // all repeated: the batch before, shuffled by reversal, twice
            std::vector<uint64_t> again(idx.rbegin(), idx.rend());
            again.insert(again.end(), idx.begin(), idx.end());
            tree.update(again), calls++;
            // the ends of the key space and, at depth 36, indexes with bits 32 .. 35 set
            idx = {0, mask, mask - 1, 1};
            if (d == 36) {
                for (int b = 32; b < 36; b++) { idx.push_back(1ull << b); idx.push_back((1ull << b) | 1); idx.push_back((1ull << b) - 1); }
                idx.push_back(0xF00000005ull);
                idx.push_back(0xF00000004ull);
                idx.push_back(0xFFFFFFFFull);
                idx.push_back(0x100000000ull);
            }
            tree.update(idx), calls++;
            // random calls in a row: the whole key space, and windows of 2, 4 and 64 leaves (heavy collisions), slots carrying over
            for (int trial = 0; trial < 24; trial++) {
                const uint64_t k = 1 + rnd() % 300, spans[4] = {0, 2, 4, 64};
                uint64_t span = spans[trial % 4];
                if (!span || span > mask + 1) span = mask + 1;
                const uint64_t base = (rnd() & mask) / span * span;
                idx.clear();
                for (uint64_t j = 0; j < k; j++) idx.push_back(base + rnd() % span);
                tree.update(idx), calls++;
            }
            // one update alone
            idx.assign(1, rnd() & mask);
            tree.update(idx), calls++;
        }
    }
    {   // the store does not grow past 2^31 slots: a call that needs one slot more is refused and changes nothing; one that fits exactly is served
        const uint32_t d = 5;
        const uint64_t k = 1, idx[1] = {9};
        sparse_tree_index index(d);
        sparse_update_plan p;
        index.slots = GS_SPARSE_MAX_SLOTS - d;                                // a new leaf needs d + 1 fresh slots
        if (sparse_plan_update(index, idx, k, p)) FAIL("a plan past 2^31 slots was not refused");
        if (index.slots != GS_SPARSE_MAX_SLOTS - d || index.level[0].used) FAIL("a refused plan changed the index");
        index.slots = GS_SPARSE_MAX_SLOTS - d - 1;
        if (!sparse_plan_update(index, idx, k, p) || p.slots_after != GS_SPARSE_MAX_SLOTS || !sparse_plan_update_in_bounds(p)) FAIL("a plan that fills the store exactly");
        if (p.write[d * k] != GS_SPARSE_MAX_SLOTS - 1) FAIL("the last slot");
        calls += 2;
    }
    std::printf("sparse tree plan: %u calls ok\n", calls);
    return 0;
}
