// The host plan of gs_curve_msm (genstark_amd/csrc/msm_plan.h) on its own: for every (count, bits, window) of the lists below the
// plan either refuses, naming the argument, or its windows cover the scalar's bits, its grids and index maps reach every pair and every
// bucket exactly once, its level counts fold every segment into its first element, its workspace regions lie apart below the cap, and
// the longest chain of additions one thread runs stays within 2^12 — none of which may depend on the scalars' values.
// Built with -fsanitize=address,undefined by tests/test_msm.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "../../genstark_amd/csrc/msm_plan.h"

#define CHECK(cond)                                                                                                           \
    do {                                                                                                                      \
        if (!(cond)) {                                                                                                        \
            std::printf("FAILED %s (line %d): count %llu bits %u window %u\n", #cond, __LINE__, (unsigned long long)g_count, g_bits, g_window); \
            std::exit(1);                                                                                                     \
        }                                                                                                                     \
    } while (0)

static uint64_t g_count;
static uint32_t g_bits, g_window;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 32);
}

// after `levels` levels, element 0 of a segment of m holds every element exactly once
static void check_levels(uint64_t m, uint32_t levels) {
    std::vector<uint64_t> weight(m, 1);
    uint64_t stride = 1;
    for (uint32_t l = 0; l < levels; l++, stride *= MSM_RADIX)
        for (uint64_t r = 0; r < m; r += MSM_RADIX * stride)
            for (uint64_t j = 1; j < MSM_RADIX && r + j * stride < m; j++) { weight[r] += weight[r + j * stride]; weight[r + j * stride] = 0; }
    CHECK(m == 0 || weight[0] == m);
}

static void check_digits(const msm_plan &p, uint32_t stride) {
    for (int trial = 0; trial < 8; trial++) {
        uint32_t words[8];
        for (uint32_t &w : words) w = trial == 0 ? 0xffffffffu : rnd();
        uint32_t rebuilt[9] = {0};
        for (uint32_t w = 0; w < p.windows; w++) {
            const uint32_t d = msm_digit(words, stride, p.bits, p.windows, w);
            CHECK(d < p.buckets);
            const uint32_t lo = msm_window_lo(p.bits, p.windows, w), width = msm_window_lo(p.bits, p.windows, w + 1) - lo;
            CHECK(width >= 1 && width <= p.c && d < (1u << width));
            const uint64_t v = (uint64_t)d << (lo & 31);
            rebuilt[lo >> 5] |= (uint32_t)v;
            rebuilt[(lo >> 5) + 1] |= (uint32_t)(v >> 32);
        }
        for (uint32_t b = 0; b < 256; b++) {
            const uint32_t want = b < p.bits ? (words[b >> 5] >> (b & 31)) & 1u : 0u;
            CHECK(((rebuilt[b >> 5] >> (b & 31)) & 1u) == want);
        }
        CHECK(rebuilt[8] == 0);
    }
}

static std::set<std::pair<uint32_t, uint32_t>> chunk_maps_seen;

static void check_plan(const msm_plan &p, uint32_t stride) {
    CHECK(p.chain_thread >= 1 && p.chain_thread <= MSM_CHAIN_CAP && p.chain_total >= p.chain_thread);
    CHECK(p.workspace <= MSM_WORKSPACE_CAP && p.workspace > 0);
    const uint64_t jac_bytes = 3ull * p.elt_bytes;
    if (p.route == MSM_ROUTE_MULTIPLY_THEN_SUM) {
        const uint64_t first = (p.count + MSM_BLOCK_SUM - 1) / MSM_BLOCK_SUM, second = (first + MSM_BLOCK_SUM - 1) / MSM_BLOCK_SUM;
        CHECK(p.grid_tree == first && p.tree_levels >= 1);
        uint64_t left = p.count;                                             // every launch folds MSM_BLOCK_SUM to one; the last leaves one
        for (uint32_t l = 0; l < p.tree_levels; l++) left = (left + MSM_BLOCK_SUM - 1) / MSM_BLOCK_SUM;
        CHECK(left == 1 && (p.tree_levels == 1 || first > 1));
        CHECK(p.off_scalars % 256 == 0 && p.off_products % 256 == 0 && p.off_flags % 256 == 0 && p.off_partial % 256 == 0 && p.off_partial_b % 256 == 0);
        CHECK(p.off_scalars + (stride == 32 ? 0 : p.count * 32) <= p.off_products && p.off_products + p.count * 2 * p.elt_bytes <= p.off_flags);
        CHECK(p.off_flags + p.count <= p.off_partial && p.off_partial + first * jac_bytes <= p.off_partial_b && p.off_partial_b + second * jac_bytes <= p.workspace);
        CHECK(p.chain_thread == 2 * p.bits);
        return;
    }
    CHECK(p.route == MSM_ROUTE_BUCKETS);
    // the windows cover the bits, the last one not empty
    CHECK(p.c >= 1 && p.c <= MSM_MAX_WINDOW && (g_window == 0 || p.c == g_window));
    CHECK((uint64_t)p.windows * p.c >= p.bits && (uint64_t)(p.windows - 1) * p.c < p.bits);
    CHECK(msm_window_lo(p.bits, p.windows, 0) == 0 && msm_window_lo(p.bits, p.windows, p.windows) == p.bits);
    CHECK(p.buckets == 1ull << p.c && p.keys == p.windows * p.buckets && p.pairs == p.count * p.windows);
    check_digits(p, stride);
    // every pair once
    CHECK((uint64_t)p.grid_pairs * MSM_BLOCK_PAIRS >= p.pairs && (uint64_t)(p.grid_pairs - 1) * MSM_BLOCK_PAIRS < p.pairs);
    if (p.pairs <= (1ull << 21)) {
        std::vector<uint8_t> seen(p.pairs, 0);
        for (uint64_t i = 0; i < p.pairs; i++) {
            uint32_t w;
            uint64_t t;
            msm_pair(p.count, i, &w, &t);
            CHECK(w < p.windows && t < p.count && !seen[w * p.count + t]);
            seen[w * p.count + t] = 1;
        }
    } else {                                                                 // the ends, the seams of the windows and a sample: the map is i = w * count + t
        for (int trial = 0; trial < 4096; trial++) {
            const uint64_t i = trial < 1024 ? (uint64_t)(trial % p.windows) * p.count + (trial & 1 ? p.count - 1 : 0) : (((uint64_t)rnd() << 32) | rnd()) % p.pairs;
            uint32_t w;
            uint64_t t;
            msm_pair(p.count, i, &w, &t);
            CHECK(w < p.windows && t < p.count && w * p.count + t == i);
        }
    }
    // the slices: enough threads and rows for the two extreme fillings (one bucket per window; every bucket alike), and for the bound itself
    CHECK((uint64_t)p.grid_slices * MSM_BLOCK_POINTS >= p.slices_max);
    const uint64_t one_bucket = p.windows * ((p.count + MSM_SLICE - 1) / MSM_SLICE);
    uint64_t spread = p.count;
    if (p.buckets > 1) {
        const uint64_t filled = p.buckets - 1, each = p.count / filled, more = p.count % filled;
        spread = more * ((each + 1 + MSM_SLICE - 1) / MSM_SLICE) + (filled - more) * ((each + MSM_SLICE - 1) / MSM_SLICE);
    }
    CHECK(one_bucket <= p.slices_max && p.windows * spread <= p.slices_max);
    CHECK(p.slices_max >= p.pairs / MSM_SLICE + (p.keys < p.pairs ? p.keys : p.pairs));   // sum of ceil(n / S) <= pairs / S + non-empty buckets
    CHECK(p.slices_max < (1ull << 32) && p.pairs < (1ull << 32) && p.keys + 1 < (1ull << 32));   // the kernels index them with 32 bits
    check_levels((p.count + MSM_SLICE - 1) / MSM_SLICE, p.bucket_levels);   // the most slices a bucket can have
    // every bucket in one chunk
    CHECK(p.chunk >= 1 && p.chunk <= MSM_CHUNK && p.chunks * p.chunk == p.buckets);
    CHECK((uint64_t)p.grid_chunks * MSM_BLOCK_POINTS >= p.windows * p.chunks && (uint64_t)(p.grid_chunks - 1) * MSM_BLOCK_POINTS < p.windows * p.chunks);
    CHECK(p.grid_chunk_tree == p.grid_chunks);
    if (chunk_maps_seen.insert({p.bits, p.c}).second) {
        std::vector<uint8_t> seen(p.keys, 0);
        for (uint64_t t = 0; t < p.windows * p.chunks; t++) {
            uint32_t w, lo, hi;
            msm_chunk_range(p.chunks, p.chunk, t, &w, &lo, &hi);
            CHECK(w < p.windows && lo < hi && hi <= p.buckets && hi - lo == p.chunk);
            for (uint32_t d = lo; d < hi; d++) {
                CHECK(!seen[w * p.buckets + d]);
                seen[w * p.buckets + d] = 1;
            }
        }
        for (uint8_t s : seen) CHECK(s);
        check_levels(p.chunks, p.chunk_levels);
    }
    // the workspace: regions in order, apart, inside
    const uint64_t offs[] = {p.off_start, p.off_cursor, p.off_slice_start, p.off_sorted, p.off_slice_key, p.off_partial, p.off_chunk_sums, p.off_chunk_runs, p.workspace};
    const uint64_t sizes[] = {(p.keys + 1) * 4, (p.keys + 1) * 4, (p.keys + 1) * 4, p.pairs * 4, p.slices_max * 4, p.slices_max * jac_bytes,
                              p.windows * p.chunks * jac_bytes, p.windows * p.chunks * jac_bytes};
    for (int r = 0; r < 8; r++) CHECK(offs[r] % 256 == 0 && offs[r] + sizes[r] <= offs[r + 1]);
    // the chains: a slice, a chunk's two running sums, its lift, the fold of the windows
    CHECK(p.chain_thread >= MSM_SLICE && p.chain_thread >= 2 * p.chunk && p.chain_thread >= p.bits + p.windows);
    CHECK(p.chunks == 1 || p.chain_thread >= 2 * p.c + 1);
}

int main() {
    const uint64_t counts[] = {0, 1, 2, 63, 64, 65, 4097, 1ull << 20};
    const uint32_t bit_counts[] = {1, 7, 128, 255, 256};
    unsigned admitted = 0, refused = 0, longest = 0;
    for (uint64_t count : counts)
        for (uint32_t bits : bit_counts)
            for (uint32_t window = 0; window <= 16; window++)
                for (uint32_t stride : {32u, 16u})
                    for (int force : {-1, (int)MSM_ROUTE_BUCKETS, (int)MSM_ROUTE_MULTIPLY_THEN_SUM}) {
                        g_count = count; g_bits = bits; g_window = window;
                        if (force >= 0 && window) continue;
                        msm_plan p;
                        const char *why = msm_plan_build(count, bits, window, 32, stride, p, force);
                        if (stride == 16 && bits > 128) { CHECK(why && std::strstr(why, "bits")); refused++; continue; }
                        if (why) {                                           // only a forced window may be too much, and it says so
                            CHECK(window && std::strstr(why, "window") && std::strstr(why, "cap"));
                            refused++;
                            continue;
                        }
                        admitted++;
                        if (!count) { CHECK(p.workspace == 0); continue; }
                        CHECK(force < 0 || p.route == force);
                        check_plan(p, stride);
                        if (p.chain_thread > longest) longest = p.chain_thread;
                    }
    // the plan's own choice is never refused, whatever the element size
    for (uint64_t count = 1; count <= (1ull << 20); count = count * 2 + (count & 1 ? 0 : 1))
        for (uint32_t elt : {16u, 32u}) {
            msm_plan p;
            g_count = count; g_bits = 256; g_window = 0;
            CHECK(!msm_plan_build(count, elt == 16 ? 128 : 256, 0, elt, elt, p));
        }
    // refusals name the argument
    msm_plan p;
    g_count = 0; g_bits = 0; g_window = 0;
    CHECK(std::strstr(msm_plan_build((1ull << 20) + 1, 256, 0, 32, 32, p), "count"));
    CHECK(std::strstr(msm_plan_build(4, 256, 0, 32, 8, p), "scalar_stride"));
    CHECK(std::strstr(msm_plan_build(4, 0, 0, 32, 32, p), "bits") && std::strstr(msm_plan_build(4, 257, 0, 32, 32, p), "bits"));
    CHECK(std::strstr(msm_plan_build(4, 129, 0, 16, 16, p), "bits"));
    CHECK(std::strstr(msm_plan_build(4, 256, 17, 32, 32, p), "window"));
    CHECK(std::strstr(msm_plan_build(1ull << 20, 256, 1, 32, 32, p), "cap"));      // 2^28 pairs
    std::printf("%u combinations ok, %u refused, longest chain of one thread %u\n", admitted, refused, longest);
    return 0;
}
