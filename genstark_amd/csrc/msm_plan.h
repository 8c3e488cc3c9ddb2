// msm_plan.h — how a sum of `count` scalar multiples (gs_curve_msm, include/gstark_msm.h) is laid out on the device: the route, the
// window width, every launch's grid, the workspace and the longest chain of dependent point additions (msm.hip is the device side;
// DESIGN.md "Sums of scalar multiples" has the argument).  Plain C++, no HIP: it is tested on its own
// (tests/host_harness/msm_plan_host.cpp).  The index maps the kernels use (pair -> (window, term), chunk -> buckets) stand here too,
// so the harness walks the same arithmetic the device runs.
//   buckets            scalars are cut into `windows` digits of c bits.  Every (term, window) PAIR with a non-zero digit d goes into
//                      bucket key = window * 2^c + d by a counting sort (histogram, scan, scatter).  A bucket of n points is cut into
//                      ceil(n / MSM_SLICE) SLICES; one thread adds one slice (<= MSM_SLICE mixed additions) whatever the scalars are, and
//                      a bucket's slice sums are combined MSM_RADIX at a time, level by level.  A window's sum of d * B_d is formed by
//                      threads that each run the two running sums over a CHUNK of MSM_CHUNK buckets and lift the chunk's total by its
//                      first digit; the chunk results are combined level by level again; one thread then folds the windows (c doublings
//                      and one addition per window) and inverts once.
//   multiply_then_sum  gs_curve_mul into workspace, then workgroups that each add MSM_BLOCK_SUM of the products through LDS, launch after
//                      launch until one sum is left.
//   No bound below depends on the VALUES of the scalars: only on (count, bits, window).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MSM_HD __host__ __device__ static inline
#else
#define MSM_HD static inline
#endif

#define MSM_MAX_COUNT (1ull << 20)           // terms per call: term numbers fit 20 bits, pair counts 28
#define MSM_MAX_BITS 256u
#define MSM_MAX_WINDOW 16u
#define MSM_SLICE 32u                        // points one thread adds in a row (mixed additions)
#define MSM_RADIX 4u                         // partial sums one thread combines per level: 3 additions; fewer levels cost more latency per level
#define MSM_CHUNK 8u                         // buckets one thread runs the running sums over: 2 * 8 additions
#define MSM_BLOCK_SUM 256u                   // points one workgroup of the multiply_then_sum route adds through LDS: 8 additions in a row per launch
#define MSM_BLOCK_PAIRS 256u                 // histogram and scatter: streaming kernels
#define MSM_BLOCK_POINTS 64u                 // every kernel that adds points: one wave, as k_curve_mul (three elements of accumulator per lane)
#define MSM_SCAN_THREADS 1024u               // the scan is one workgroup
#define MSM_WORKSPACE_CAP (512ull << 20)     // bytes of workspace a call may take from the context's block cache
#define MSM_CHAIN_CAP (1u << 12)             // additions in a row that any one thread may run

enum { MSM_ROUTE_BUCKETS = 0, MSM_ROUTE_MULTIPLY_THEN_SUM = 1 };

// The plan's own route (window 0), from profiles/msm.md (tools/msm_bench.py; 256-bit scalars, 2^12, 2^14, 2^16, 2^18, 2^20 terms):
//   32-byte elements (224-bit flavour): the bucket route took 0.90 .. 0.95 of gs_curve_mul's time at 2^12 .. 2^16 terms, 0.44 at 2^18 and
//     0.19 at 2^20; multiply_then_sum 1.14 at 2^12 .. 2^16 (the inversion and two sum launches on top of the multiplication) and 1.04 at
//     2^20: buckets at every count.
//   16-byte elements (128-bit flavour): the bucket route took 1.03 at 2^12 and 2^14 (windows of 7 and 8 bits), 1.16 at 2^16 (its best
//     width, 10), 0.73 at 2^18, 0.39 at 2^20; multiply_then_sum 1.09 at 2^12 .. 2^16, 1.06 at 2^18: multiply_then_sum around 2^16 only.
//     The two ends of that range lie between measured counts (2^14 | 2^16 | 2^18): they are placed half way, NOT measured.
#define MSM_NARROW_SUM_ABOVE (1ull << 15)    // 16-byte elements: multiply_then_sum for counts above this ...
#define MSM_NARROW_SUM_BELOW (1ull << 17)    // ... and below this
MSM_HD int msm_choose_route(uint64_t count, uint32_t elt_bytes) {
    return elt_bytes == 16 && count > MSM_NARROW_SUM_ABOVE && count < MSM_NARROW_SUM_BELOW ? MSM_ROUTE_MULTIPLY_THEN_SUM : MSM_ROUTE_BUCKETS;
}

struct msm_plan {
    int route = MSM_ROUTE_BUCKETS;
    uint64_t count = 0;
    uint32_t bits = 0, elt_bytes = 0;
    // buckets
    uint32_t c = 0, windows = 0;             // window width, ceil(bits / c)
    uint64_t buckets = 0;                    // 2^c digits per window, digit 0 never filled
    uint64_t keys = 0;                       // windows * buckets
    uint64_t pairs = 0;                      // count * windows
    uint64_t slices_max = 0;                 // upper bound of sum over buckets of ceil(n / MSM_SLICE)
    uint32_t bucket_levels = 0;              // levels of MSM_RADIX that combine the most slices one bucket can have: ceil(count / MSM_SLICE)
    uint32_t chunk = 0;                      // buckets per chunk: min(MSM_CHUNK, buckets)
    uint64_t chunks = 0;                     // chunks per window
    uint32_t chunk_levels = 0;               // levels of MSM_RADIX that combine a window's chunk results
    // multiply_then_sum
    uint32_t tree_levels = 0;                // launches of k_msm_block_sum, each MSM_BLOCK_SUM to one, until one sum is left
    // grids (blocks); the block sizes are the MSM_BLOCK_* above
    uint32_t grid_pairs = 0, grid_slices = 0, grid_chunks = 0, grid_chunk_tree = 0, grid_tree = 0;
    // workspace: byte offsets into ONE block, each a multiple of 256
    uint64_t off_start = 0, off_cursor = 0, off_slice_start = 0, off_sorted = 0, off_slice_key = 0, off_partial = 0, off_chunk_sums = 0, off_chunk_runs = 0;
    uint64_t off_scalars = 0, off_products = 0, off_flags = 0, off_partial_b = 0;
    uint64_t workspace = 0;
    // the longest chain of dependent point operations (additions and doublings alike) ONE thread runs, and the sum of the chains of
    // all launches in a row (the latency of the call in units of a point operation)
    uint32_t chain_thread = 0, chain_total = 0;
    uint64_t products = 0;                   // field products of the group law for the worst case of every digit non-zero (the final inversion not counted)
};

MSM_HD uint32_t msm_levels(uint64_t n) {     // the smallest L with MSM_RADIX^L >= n
    uint32_t l = 0;
    for (uint64_t reach = 1; reach < n; reach *= MSM_RADIX) l++;
    return l;
}
MSM_HD uint32_t msm_log2_ceil(uint64_t n) { uint32_t l = 0; while ((1ull << l) < n) l++; return l; }

// pair i -> (window, term): consecutive pairs are consecutive terms of one window, so a wave reads consecutive scalars
MSM_HD void msm_pair(uint64_t count, uint64_t i, uint32_t *window, uint64_t *term) { *window = (uint32_t)(i / count); *term = i % count; }

// The windows share the bits evenly: window w starts at bit msm_window_lo(w) and the widths differ by at most one (never above c, since
// windows = ceil(bits / c)).  A last window of a few bits would put every term into a handful of buckets, and then the sort's counters
// are what the call waits for (profiles/msm.md: widths whose last window had 4 bits took half as long again at 2^20 terms).
MSM_HD uint32_t msm_window_lo(uint32_t bits, uint32_t windows, uint32_t w) {
    const uint32_t base = bits / windows, more = bits % windows;
    return w * base + (w < more ? w : more);
}

// digit `window` of the low `bits` bits of a little-endian scalar of `stride` bytes (words: the scalar as 32-bit words)
MSM_HD uint32_t msm_digit(const uint32_t *words, uint32_t stride, uint32_t bits, uint32_t windows, uint32_t window) {
    const uint32_t lo = msm_window_lo(bits, windows, window), hi = msm_window_lo(bits, windows, window + 1);      // [lo, hi), at most 16 bits
    const uint32_t w = lo >> 5, nwords = stride / 4;
    uint64_t v = words[w];
    if (w + 1 < nwords) v |= (uint64_t)words[w + 1] << 32;
    return (uint32_t)((v >> (lo & 31)) & ((1ull << (hi - lo)) - 1));
}

// chunk thread t -> its window and the digits [lo, hi) it runs over; digit 0 is in chunk 0 and is skipped by the kernel
MSM_HD void msm_chunk_range(uint64_t chunks, uint32_t chunk, uint64_t t, uint32_t *window, uint32_t *lo, uint32_t *hi) {
    *window = (uint32_t)(t / chunks);
    *lo = (uint32_t)(t % chunks) * chunk;
    *hi = *lo + chunk;
}

// The window width the plan picks for `count` terms: ceil(log2 count) - 6, between 7 and 13.  From profiles/msm.md: the fastest forced
// width was 7 at 2^12 terms (of 3 .. 7), 8 at 2^14 (of 5 .. 9), 10 at 2^16 (of 7 .. 11), 12 at 2^18 (of 9 .. 13) and 13 at 2^20 (of
// 11 .. 15) in both measured flavours; below 2^12 terms nothing was measured and the width of 2^12 is kept.
MSM_HD uint32_t msm_choose_window(uint64_t count) {
    const uint32_t lg = msm_log2_ceil(count < 1 ? 1 : count);
    const uint32_t c = lg > 6 ? lg - 6 : 0;
    return c < 7 ? 7 : (c > 13 ? 13 : c);
}

static inline uint64_t msm_align(uint64_t v) { return (v + 255) & ~255ull; }

// Fills `plan`; returns nullptr, or the reason the combination is refused (naming the argument).  window 0: the plan chooses route and
// width; 1 .. 16: the bucket route with that width.  elt_bytes: 16 or 32 (the size of a field element; a Jacobian point is three).
// force_route: -1, or a route for window 0 (the measurement's handle, tools/msm_bench.py).
static inline const char *msm_plan_build(uint64_t count, uint32_t bits, uint32_t window, uint32_t elt_bytes, uint32_t scalar_stride, msm_plan &p,
                                         int force_route = -1) {
    p = msm_plan();
    if (count > MSM_MAX_COUNT) return "count: at most 2^20 terms per call";
    if (scalar_stride != 16 && scalar_stride != 32) return "scalar_stride: 16 or 32 bytes";
    if (bits < 1 || bits > MSM_MAX_BITS) return "bits: outside 1 .. 256";
    if (bits > 8 * scalar_stride) return "bits: above 128 with a scalar_stride of 16";
    if (window > MSM_MAX_WINDOW) return "window: outside 0 .. 16";
    p.count = count; p.bits = bits; p.elt_bytes = elt_bytes;
    const uint64_t jac_bytes = 3ull * elt_bytes;
    if (!count) return nullptr;
    p.route = window ? MSM_ROUTE_BUCKETS : (force_route >= 0 ? force_route : msm_choose_route(count, elt_bytes));
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) { const uint64_t here = at; at = msm_align(at + bytes); return here; };
    if (p.route == MSM_ROUTE_MULTIPLY_THEN_SUM) {
        const uint64_t first = (count + MSM_BLOCK_SUM - 1) / MSM_BLOCK_SUM, second = (first + MSM_BLOCK_SUM - 1) / MSM_BLOCK_SUM;
        p.tree_levels = 1;
        for (uint64_t left = first; left > 1; left = (left + MSM_BLOCK_SUM - 1) / MSM_BLOCK_SUM) p.tree_levels++;
        p.grid_tree = (uint32_t)first;
        p.off_scalars = take(scalar_stride == 32 ? 0 : count * 32);
        p.off_products = take(count * 2 * elt_bytes);
        p.off_flags = take(count);
        p.off_partial = take(first * jac_bytes);                             // the launches write here and to off_partial_b by turns
        p.off_partial_b = take(second * jac_bytes);
        p.workspace = at;
        p.chain_thread = 2 * bits;
        p.chain_total = 2 * bits + 8 * p.tree_levels;
        p.products = count * ((uint64_t)bits * 21 + 4 + 16);
        return nullptr;
    }
    p.c = window ? window : msm_choose_window(count);
    if (!window && p.c > bits) p.c = bits;
    p.windows = (bits + p.c - 1) / p.c;
    p.buckets = 1ull << p.c;
    p.keys = p.windows * p.buckets;
    p.pairs = count * p.windows;
    p.slices_max = p.pairs / MSM_SLICE + (p.keys < p.pairs ? p.keys : p.pairs);
    p.bucket_levels = msm_levels((count + MSM_SLICE - 1) / MSM_SLICE);
    p.chunk = p.buckets < MSM_CHUNK ? (uint32_t)p.buckets : MSM_CHUNK;
    p.chunks = p.buckets / p.chunk;
    p.chunk_levels = msm_levels(p.chunks);
    p.grid_pairs = (uint32_t)((p.pairs + MSM_BLOCK_PAIRS - 1) / MSM_BLOCK_PAIRS);
    p.grid_slices = (uint32_t)((p.slices_max + MSM_BLOCK_POINTS - 1) / MSM_BLOCK_POINTS);
    p.grid_chunks = (uint32_t)((p.windows * p.chunks + MSM_BLOCK_POINTS - 1) / MSM_BLOCK_POINTS);
    p.grid_chunk_tree = p.grid_chunks;
    p.off_start = take((p.keys + 1) * 4);
    p.off_cursor = take((p.keys + 1) * 4);
    p.off_slice_start = take((p.keys + 1) * 4);
    p.off_sorted = take(p.pairs * 4);
    p.off_slice_key = take(p.slices_max * 4);
    p.off_partial = take(p.slices_max * jac_bytes);
    p.off_chunk_sums = take(p.windows * p.chunks * jac_bytes);
    p.off_chunk_runs = take(p.windows * p.chunks * jac_bytes);
    p.workspace = at;
    if (p.workspace > MSM_WORKSPACE_CAP) return "window: the workspace of this width exceeds the cap of 512 MiB";
    const uint32_t chunk_chain = 2 * p.chunk, lift_chain = p.chunks > 1 ? 2 * p.c + 1 : 0, final_chain = bits + p.windows;
    p.chain_thread = MSM_SLICE;
    if (chunk_chain > p.chain_thread) p.chain_thread = chunk_chain;
    if (lift_chain > p.chain_thread) p.chain_thread = lift_chain;
    if (final_chain > p.chain_thread) p.chain_thread = final_chain;
    p.chain_total = MSM_SLICE + (MSM_RADIX - 1) * (p.bucket_levels + p.chunk_levels) + chunk_chain + lift_chain + final_chain;
    p.products = p.pairs * 11 + p.slices_max * 16 + p.windows * p.chunks * ((uint64_t)2 * p.chunk * 16 + p.c * 26ull + 16) + bits * 10ull + p.windows * 16ull;
    return nullptr;
}
