// scan_plan_host.cpp — the host plan of the scans (genstark_amd/csrc/scan_plan.h) on its own: the tile and the launches at every edge
// length, the cap, the size of rows * cols where it would overflow, and every aliasing case.  Plain C++ with its own main; the test
// suite builds it with -fsanitize=address,undefined (tests/test_scan.py).  Prints "scan plan OK" and returns 0, or says what failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../genstark_amd/csrc/scan_plan.h"

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static bool refused(const char *why, const char *part) { return why && strstr(why, part); }

static void check_lengths(uint32_t elt_bytes) {
    const uint32_t per = scan_per_thread(elt_bytes), tile = scan_tile(elt_bytes);
    CHECK(per * elt_bytes == SCAN_LANE_BYTES && tile == SCAN_BLOCK * per);
    CHECK(per == (elt_bytes == 16 ? 4u : 2u) && tile == (elt_bytes == 16 ? 1024u : 512u));
    // the cap is what one workgroup's scan of the aggregates covers, in every flavour
    CHECK((uint64_t)tile * SCAN_TOTALS_BLOCK * SCAN_MAX_AGGREGATES_PER_THREAD >= SCAN_MAX_ELEMENTS);
    const uint64_t T = tile;
    const uint64_t lengths[] = {0, 1, 2, 63, 64, 65, 64ull * per - 1, 64ull * per, 64ull * per + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 65 * T + 3,
                                SCAN_TOTALS_BLOCK * T, SCAN_TOTALS_BLOCK * T + 1, SCAN_MAX_ELEMENTS - 1, SCAN_MAX_ELEMENTS};
    for (uint64_t n : lengths) {
        for (uint32_t payload = 1; payload <= 2; payload++) {
            for (int single = 0; single < 2; single++) {
                scan_plan pl;
                const char *why = scan_plan_build(elt_bytes, payload, n, single != 0, pl);
                CHECK(!why);
                CHECK(pl.n == n && pl.tile == tile && pl.per_thread == per && pl.elt_bytes == elt_bytes);
                if (n == 0) { CHECK(pl.launches == 0 && pl.tiles == 0 && pl.aggregate_bytes == 0); continue; }
                CHECK((uint64_t)pl.tiles * T >= n && (uint64_t)(pl.tiles - 1) * T < n);
                if (n <= T) {
                    CHECK(pl.launches == 1 && pl.grid[0] == 1 && pl.grid[1] == 0 && pl.grid[2] == 0 && pl.aggregate_bytes == 0);
                    continue;
                }
                CHECK(pl.launches == (single ? 2u : 3u));
                CHECK(pl.grid[0] == pl.tiles && pl.grid[1] == 1 && pl.grid[2] == (single ? 0u : pl.tiles));
                CHECK(pl.aggregates_per_thread >= 1 && pl.aggregates_per_thread <= SCAN_MAX_AGGREGATES_PER_THREAD);
                CHECK((uint64_t)pl.aggregates_per_thread * SCAN_TOTALS_BLOCK >= pl.tiles);                 // every aggregate has a thread
                CHECK((uint64_t)(pl.aggregates_per_thread - 1) * SCAN_TOTALS_BLOCK < pl.tiles);            // ... and no thread more than it needs
                CHECK(pl.aggregate_bytes == (uint64_t)pl.tiles * (payload * elt_bytes + 4));
                // the buffer really holds what the kernels index: `tiles` payloads, then `tiles` flags
                std::vector<unsigned char> buffer(pl.aggregate_bytes);
                buffer[(uint64_t)(pl.tiles - 1) * payload * elt_bytes + payload * elt_bytes - 1] = 1;
                buffer[(uint64_t)pl.tiles * payload * elt_bytes + (uint64_t)(pl.tiles - 1) * 4 + 3] = 1;
            }
        }
    }
    scan_plan pl;
    CHECK(refused(scan_plan_build(elt_bytes, 1, SCAN_MAX_ELEMENTS + 1, false, pl), "2^24") && pl.launches == 0);
    CHECK(refused(scan_plan_build(elt_bytes, 2, ~0ull, false, pl), "2^24"));
    CHECK(refused(scan_plan_build(elt_bytes, 3, 5, false, pl), "pair"));
    CHECK(refused(scan_plan_build(elt_bytes, 0, 5, false, pl), "pair"));
}

static void check_counts() {
    uint64_t n = 99;
    CHECK(!scan_count(0, 0, &n) && n == 0);
    CHECK(!scan_count(0, 5, &n) && n == 0);
    CHECK(!scan_count(0, ~0ull, &n) && n == 0);
    CHECK(refused(scan_count(1, 0, &n), "cols is 0") && n == 0);
    CHECK(refused(scan_count(~0ull, 0, &n), "cols is 0"));
    CHECK(!scan_count(1, 1, &n) && n == 1);
    CHECK(!scan_count(1, SCAN_MAX_ELEMENTS, &n) && n == SCAN_MAX_ELEMENTS);
    CHECK(!scan_count(SCAN_MAX_ELEMENTS, 1, &n) && n == SCAN_MAX_ELEMENTS);
    CHECK(!scan_count(1ull << 12, 1ull << 12, &n) && n == SCAN_MAX_ELEMENTS);
    CHECK(refused(scan_count(1, SCAN_MAX_ELEMENTS + 1, &n), "2^24") && n == 0);
    CHECK(refused(scan_count((1ull << 12) + 1, 1ull << 12, &n), "2^24"));
    CHECK(refused(scan_count(3, (SCAN_MAX_ELEMENTS / 3) + 1, &n), "2^24"));
    // products that wrap 2^64: to 0, to 1 and to a small count
    CHECK(refused(scan_count(1ull << 32, 1ull << 32, &n), "2^24") && n == 0);
    CHECK(refused(scan_count(~0ull, ~0ull, &n), "2^24") && n == 0);                  // (2^64 - 1)^2 = 1 (mod 2^64)
    CHECK(refused(scan_count(1ull << 63, 2, &n), "2^24") && n == 0);
    CHECK(refused(scan_count((1ull << 63) + 8, 2, &n), "2^24") && n == 0);           // = 16 (mod 2^64)
    CHECK(refused(scan_count(2, (1ull << 63) + 8, &n), "2^24") && n == 0);
    CHECK(refused(scan_count(0x100000001ull, 0x100000000ull, &n), "2^24") && n == 0);
}

static void check_aliasing() {
    const uint64_t es = 16, n = 1000, bytes = n * es, base = 1ull << 20;
    const scan_range none = {0, 0}, values = {base, bytes}, a = {base + 4 * bytes, bytes}, heads = {base + 8 * bytes, n};
    const scan_range apart = {base + 2 * bytes, bytes}, totals = {base + 10 * bytes, 10 * es};
    CHECK(!scan_check_alias(values, none, none, apart, none));                       // apart
    CHECK(!scan_check_alias(values, none, none, values, none));                      // exactly the input
    CHECK(!scan_check_alias(values, a, heads, values, totals));
    CHECK(!scan_check_alias(values, none, none, {base + bytes, bytes}, none));       // touching at the end: no byte in common
    CHECK(!scan_check_alias(values, none, none, {base - bytes, bytes}, none));
    for (uint64_t shift : {es, bytes - es, bytes / 2}) {                             // shifted either way by one element, by all but one, by half
        CHECK(refused(scan_check_alias(values, none, none, {base + shift, bytes}, none), "exactly"));
        CHECK(refused(scan_check_alias(values, none, none, {base - shift, bytes}, none), "exactly"));
    }
    CHECK(refused(scan_check_alias(values, none, none, {base, bytes - es}, none), "exactly"));      // the same start, another length
    CHECK(refused(scan_check_alias(values, a, none, a, none), "overlaps a"));        // never a, not even exactly
    CHECK(refused(scan_check_alias(values, a, none, {a.at + es, bytes}, none), "overlaps a"));
    CHECK(refused(scan_check_alias(values, a, none, {a.at - bytes + es, bytes}, none), "overlaps a"));
    CHECK(refused(scan_check_alias(values, none, heads, {heads.at - bytes + 1, bytes}, none), "heads"));
    CHECK(refused(scan_check_alias(values, none, heads, {heads.at + n - 1, bytes}, none), "heads"));
    CHECK(!scan_check_alias(values, none, heads, {heads.at + n, bytes}, none));
    CHECK(refused(scan_check_alias(values, none, none, apart, {values.at + bytes - es, 10 * es}), "totals_out overlaps an input"));
    CHECK(refused(scan_check_alias(values, a, none, apart, {a.at, 10 * es}), "totals_out overlaps an input"));
    CHECK(refused(scan_check_alias(values, none, heads, apart, {heads.at - es, 10 * es}), "totals_out overlaps an input"));
    CHECK(refused(scan_check_alias(values, none, none, apart, {apart.at + bytes - es, 10 * es}), "totals_out overlaps out"));
    CHECK(refused(scan_check_alias(values, none, none, values, {values.at, es}), "totals_out overlaps an input"));
    CHECK(!scan_check_alias(values, none, none, none, totals));                      // the reduction: no out
    CHECK(refused(scan_check_alias(values, none, none, none, {values.at, es}), "totals_out overlaps an input"));
    // ranges at the top of the address space do not wrap
    const scan_range high = {~0ull - bytes + 1, bytes};
    CHECK(!scan_check_alias(high, none, none, values, none));
    CHECK(!scan_check_alias(values, none, none, high, none));
    CHECK(!scan_check_alias(high, none, none, high, none));
    CHECK(refused(scan_check_alias(high, none, none, {high.at + es, bytes - es}, none), "exactly"));
    CHECK(refused(scan_check_alias(high, none, none, {high.at - es, bytes}, none), "exactly"));
}

int main() {
    check_lengths(16);
    check_lengths(32);
    scan_plan pl;
    CHECK(refused(scan_plan_build(8, 1, 5, false, pl), "16 or 32"));
    CHECK(refused(scan_plan_build(64, 1, 5, false, pl), "16 or 32"));
    check_counts();
    check_aliasing();
    if (failures) { printf("scan plan: %d checks failed\n", failures); return 1; }
    printf("scan plan OK\n");
    return 0;
}
