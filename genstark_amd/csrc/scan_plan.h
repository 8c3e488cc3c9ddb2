// scan_plan.h — how a running sum, product or linear recurrence (include/gstark_scan.h) over n elements is scheduled: the tile one
// workgroup scans, the number of tiles, the grid of each launch, the size of the buffer of tile aggregates, and the argument checks
// (the size of rows * cols, the aliasing rules).  Plain C++, no HIP and no field header: scan.hip is the device side, and this file is
// tested on its own (tests/host_harness/scan_plan_host.cpp).  Nothing here depends on the VALUES that are scanned.
//   tile        SCAN_BLOCK threads, each owning the SCAN_LANE_BYTES / element-size consecutive elements that fill 64 bytes: 1024
//               elements of 16 bytes, 512 of 32 bytes.
//   launches    n <= tile: ONE (the apply kernel with no carry).  Otherwise three: one aggregate per tile, ONE workgroup of
//               SCAN_TOTALS_BLOCK threads that scans the aggregates exclusively (each thread owns ceil(tiles / SCAN_TOTALS_BLOCK)
//               consecutive ones), and the apply kernel with its tile's carry.  A reduction to ONE total stops after the second.
//   cap         2^24 elements: at most 2^15 aggregates, 32 per thread of the second launch.  A fourth launch never exists.
#pragma once
#include <cstdint>

#define SCAN_MAX_ELEMENTS (1ull << 24)       // per call, all segments together
#define SCAN_BLOCK 256u                      // threads of a tile's workgroup
#define SCAN_LANE_BYTES 64u                  // consecutive bytes one thread owns
#define SCAN_TOTALS_BLOCK 1024u              // threads of the ONE workgroup that scans the tile aggregates
#define SCAN_MAX_AGGREGATES_PER_THREAD 32u   // SCAN_MAX_ELEMENTS / (the smallest tile, 512) / SCAN_TOTALS_BLOCK

enum { SCAN_OP_SUM = 0, SCAN_OP_PRODUCT = 1, SCAN_OP_AFFINE = 2 };

struct scan_plan {
    uint32_t elt_bytes = 0;        // 16 or 32
    uint32_t per_thread = 0;       // consecutive elements of one thread
    uint32_t tile = 0;             // elements of one workgroup
    uint64_t n = 0;                // rows * cols
    uint32_t tiles = 0;
    uint32_t launches = 0;         // 0 (n == 0), 1, 2 (one total of more than a tile) or 3
    uint32_t grid[3] = {0, 0, 0};  // workgroups of each launch
    uint32_t aggregates_per_thread = 0;   // of the second launch
    uint64_t aggregate_bytes = 0;  // the temporary: `tiles` payloads of `payload_elts` elements, then `tiles` 32-bit flags
};

static inline uint32_t scan_per_thread(uint32_t elt_bytes) { return SCAN_LANE_BYTES / elt_bytes; }
static inline uint32_t scan_tile(uint32_t elt_bytes) { return SCAN_BLOCK * scan_per_thread(elt_bytes); }

// rows * cols as *n, or the reason it is refused
static inline const char *scan_count(uint64_t rows, uint64_t cols, uint64_t *n) {
    *n = 0;
    if (rows == 0) return nullptr;                                           // nothing to do, whatever cols says
    if (cols == 0) return "cols is 0 with rows > 0";
    if (rows > SCAN_MAX_ELEMENTS || cols > SCAN_MAX_ELEMENTS || rows * cols > SCAN_MAX_ELEMENTS) return "at most 2^24 elements per call";   // (no overflow: both factors are at most 2^24 here)
    *n = rows * cols;
    return nullptr;
}

// The schedule for n elements of elt_bytes bytes whose aggregate is payload_elts elements (1: sum, product; 2: the affine pair).
// single_total: the caller wants ONE total and no running values (the reduction of one row).
static inline const char *scan_plan_build(uint32_t elt_bytes, uint32_t payload_elts, uint64_t n, bool single_total, scan_plan &pl) {
    pl = scan_plan();
    if (elt_bytes != 16 && elt_bytes != 32) return "elements are 16 or 32 bytes";
    if (payload_elts != 1 && payload_elts != 2) return "an aggregate is one element or a pair";
    if (n > SCAN_MAX_ELEMENTS) return "at most 2^24 elements per call";
    pl.elt_bytes = elt_bytes;
    pl.per_thread = scan_per_thread(elt_bytes);
    pl.tile = scan_tile(elt_bytes);
    pl.n = n;
    if (n == 0) return nullptr;
    pl.tiles = (uint32_t)((n + pl.tile - 1) / pl.tile);
    if (pl.tiles == 1) {
        pl.launches = 1;
        pl.grid[0] = 1;
        return nullptr;
    }
    pl.aggregates_per_thread = (pl.tiles + SCAN_TOTALS_BLOCK - 1) / SCAN_TOTALS_BLOCK;
    if (pl.aggregates_per_thread > SCAN_MAX_AGGREGATES_PER_THREAD) return "more tile aggregates than one workgroup scans";      // (unreachable below the cap)
    pl.launches = single_total ? 2 : 3;
    pl.grid[0] = pl.tiles;
    pl.grid[1] = 1;
    pl.grid[2] = single_total ? 0 : pl.tiles;
    pl.aggregate_bytes = (uint64_t)pl.tiles * payload_elts * elt_bytes + (uint64_t)pl.tiles * 4;
    return nullptr;
}

// ---- aliasing: a range is (address, bytes); a range of 0 bytes or at address 0 overlaps nothing
struct scan_range { uint64_t at, bytes; };
static inline bool scan_overlap(const scan_range &x, const scan_range &y) {
    if (!x.at || !y.at || !x.bytes || !y.bytes) return false;
    return x.at >= y.at ? x.at - y.at < y.bytes : y.at - x.at < x.bytes;          // (no sum of an address and a size: nothing wraps)
}
static inline bool scan_same(const scan_range &x, const scan_range &y) { return x.at == y.at && x.bytes == y.bytes; }

// `out` may be exactly `in_place` (values, or b of the affine op) and nothing else that overlaps it; it touches neither `a` (the
// affine op's factors) nor `heads`; `totals` overlaps no input and not `out`.  Returns the reason of a refusal, or null.
static inline const char *scan_check_alias(const scan_range &in_place, const scan_range &a, const scan_range &heads, const scan_range &out, const scan_range &totals) {
    if (scan_overlap(out, in_place) && !scan_same(out, in_place)) return "out overlaps the input without being exactly the input";
    if (scan_overlap(out, a)) return "out overlaps a";
    if (scan_overlap(out, heads)) return "out overlaps heads";
    if (scan_overlap(totals, in_place) || scan_overlap(totals, a) || scan_overlap(totals, heads)) return "totals_out overlaps an input";
    if (scan_overlap(totals, out)) return "totals_out overlaps out";
    return nullptr;
}
