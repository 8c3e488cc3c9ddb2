// tree_update_plan_host.cpp — genstark_amd/csrc/tree_update_plan.h on its own (tests/test_tree_update.py compiles this with
// -fsanitize=address,undefined and runs it).  Every batch is checked twice:
//   1. the plan against its definition, by brute force in O(k^2) per level: the predecessor is the latest earlier update through the
//      sibling node, `same` the latest earlier update of the same leaf, `last` set where no later update passes the node;
//   2. the level-by-level scheme that the device runs with that plan (versions, siblings by predecessor, commit of the flagged
//      versions) against updates applied one at a time, on a tree of 64-bit values under a mixing function that stands for the hash.
// Batches: random ones for n in 2 .. 2^10 and k in 1 .. 300 (indexes from the whole tree, from a window of 2 and of 4 leaves), and
// the fixed patterns: all indexes equal, two sibling leaves alternating, every leaf once (in order and reversed), the two halves of the
// tree interleaved.  Prints "tree update plan: <batches> batches ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../genstark_amd/csrc/tree_update_plan.h"

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
        std::fprintf(stderr, " (n = %llu, k = %llu)\n", (unsigned long long)n, (unsigned long long)k); \
        std::exit(1);                              \
    } while (0)

static void check(uint64_t n, const std::vector<uint64_t> &idx) {
    const uint64_t k = idx.size();
    tree_update_plan plan;
    tree_update_plan_build(n, idx.data(), k, plan);
    uint32_t d = 0;
    while ((1ull << d) < n) d++;
    if (plan.depth != d || plan.count != k || plan.pred.size() != d * k || plan.same.size() != k || plan.last.size() != (d + 1) * k) FAIL("plan sizes");

    // 1. the definition, by brute force
    for (uint64_t j = 0; j < k; j++) {
        int32_t same = -1;
        for (uint64_t i = 0; i < j; i++)
            if (idx[i] == idx[j]) same = (int32_t)i;
        if (plan.same[j] != same) FAIL("same[%llu] = %d, not %d", (unsigned long long)j, plan.same[j], same);
        for (uint32_t l = 0; l <= d; l++) {
            const uint64_t a = (n + idx[j]) >> l;
            bool last = true;
            for (uint64_t i = j + 1; i < k; i++)
                if (((n + idx[i]) >> l) == a) last = false;
            if (plan.last[l * k + j] != (last ? 1 : 0)) FAIL("last[%u][%llu] = %d", l, (unsigned long long)j, plan.last[l * k + j]);
            if (l == d) break;
            int32_t pred = -1;
            for (uint64_t i = 0; i < j; i++)
                if (((n + idx[i]) >> l) == (a ^ 1)) pred = (int32_t)i;
            if (plan.pred[l * k + j] != pred) FAIL("pred[%u][%llu] = %d, not %d", l, (unsigned long long)j, plan.pred[l * k + j], pred);
        }
    }

    // 2. the scheme against one update at a time
    std::vector<uint64_t> nodes(2 * n), leaves(k);
    for (uint64_t i = n; i < 2 * n; i++) nodes[i] = rnd();
    for (uint64_t i = n - 1; i >= 1; i--) nodes[i] = node_hash(nodes[2 * i], nodes[2 * i + 1]);
    for (uint64_t j = 0; j < k; j++) leaves[j] = (j % 7 == 3) ? nodes[n + idx[j]] : rnd();       // some updates change nothing
    std::vector<uint64_t> seq(nodes), seq_before(k * (d + 1)), seq_roots(k);
    for (uint64_t j = 0; j < k; j++) {
        uint64_t a = n + idx[j];
        seq_before[j * (d + 1)] = seq[a];
        for (uint32_t l = 0; l < d; l++) seq_before[j * (d + 1) + l + 1] = seq[(a >> l) ^ 1];
        seq[a] = leaves[j];
        for (a >>= 1; a >= 1; a >>= 1) seq[a] = node_hash(seq[2 * a], seq[2 * a + 1]);
        seq_roots[j] = seq[1];
    }
    std::vector<uint64_t> ver((d + 1) * k), before(k * (d + 1));
    for (uint64_t j = 0; j < k; j++) {
        ver[j] = leaves[j];
        before[j * (d + 1)] = plan.same[j] >= 0 ? leaves[plan.same[j]] : nodes[n + idx[j]];
    }
    for (uint32_t l = 0; l < d; l++)
        for (uint64_t j = 0; j < k; j++) {
            const uint64_t a = (n + idx[j]) >> l;
            const int32_t p = plan.pred[l * k + j];
            const uint64_t sibling = p >= 0 ? ver[l * k + p] : nodes[a ^ 1], mine = ver[l * k + j];
            before[j * (d + 1) + l + 1] = sibling;
            ver[(l + 1) * k + j] = (a & 1) ? node_hash(sibling, mine) : node_hash(mine, sibling);
        }
    for (uint32_t l = 0; l <= d; l++)
        for (uint64_t j = 0; j < k; j++)
            if (plan.last[l * k + j]) nodes[(n + idx[j]) >> l] = ver[l * k + j];
    if (nodes != seq) FAIL("final nodes differ");
    if (before != seq_before) FAIL("witnesses differ");
    for (uint64_t j = 0; j < k; j++)
        if (ver[d * k + j] != seq_roots[j]) FAIL("root %llu differs", (unsigned long long)j);
}

int main() {
    unsigned batches = 0;
    for (uint32_t d = 1; d <= 10; d++) {
        const uint64_t n = 1ull << d;
        std::vector<uint64_t> idx;
        // all indexes equal
        idx.assign(37, n - 1);
        check(n, idx), batches++;
        idx.assign(1, 0);
        check(n, idx), batches++;
        // only two sibling leaves, alternating
        idx.clear();
        for (uint64_t j = 0; j < 41; j++) idx.push_back((n / 2 & ~1ull) + (j & 1));
        check(n, idx), batches++;
        // every leaf once, in order and reversed
        idx.clear();
        for (uint64_t i = 0; i < n; i++) idx.push_back(i);
        check(n, idx), batches++;
        idx.clear();
        for (uint64_t i = 0; i < n; i++) idx.push_back(n - 1 - i);
        check(n, idx), batches++;
        // the left and right halves of the tree interleaved
        idx.clear();
        for (uint64_t i = 0; i < n / 2; i++) { idx.push_back(i); idx.push_back(n / 2 + i); }
        check(n, idx), batches++;
        // random batches: the whole tree, and windows of 2 and 4 leaves (heavy collisions)
        for (int trial = 0; trial < 30; trial++) {
            const uint64_t k = 1 + rnd() % 300, spans[3] = {n, 2, n < 4 ? n : 4};
            const uint64_t span = spans[trial % 3], base = (rnd() % (n / span)) * span;
            idx.clear();
            for (uint64_t j = 0; j < k; j++) idx.push_back(base + rnd() % span);
            check(n, idx), batches++;
        }
    }
    std::printf("tree update plan: %u batches ok\n", batches);
    return 0;
}
