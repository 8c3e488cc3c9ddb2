// msm.hip — sums of scalar multiples sum_k scalars[k] * points[k] on short Weierstrass curves over the library's field
// (include/gstark_msm.h): a Pedersen-style commitment to a device column, the one equation that checks a block of Schnorr signatures,
// any linear combination of public keys.  msm_plan.h decides the route, the window width c, the grids and the workspace, and states the
// longest chain of additions a thread runs; curve_jac.h has the group law.  Nothing but the flavour-neutral fe_* API; LDS in the scan, as
// a parking place in k_msm_chunks and for the tree of k_msm_block_sum; the only traffic across lanes is the wave-wide counter update of the counting sort.
//
// The bucket route, all windows at once (key = window * 2^c + digit; a PAIR is one (term, window)):
//   memset            the counters
//   k_msm_pairs<histogram>  one thread per pair: its digit; counts[key] += 1 for a non-zero one (integer atomics)
//   k_msm_scan        ONE workgroup: start[] = exclusive sums of counts[], slice_start[] = exclusive sums of ceil(count / MSM_SLICE),
//                     cursor[] = start[]
//   k_msm_pairs<scatter>  one thread per pair: sorted[cursor[key]++] = term.  The order inside a bucket is whatever the atomics gave: it may
//                     differ from run to run, the sum cannot (it is a group element, written affine and canonical), and every addition
//                     below is complete, so whichever exceptional case an order meets is computed
//   k_msm_slices      one thread per slice: <= MSM_SLICE mixed additions of its bucket's points, whatever the scalars are (a batch of
//                     equal scalars fills ONE bucket per window: 2^20 / MSM_SLICE slices, not one thread adding 2^20 points)
//   k_msm_bucket_level  x plan.bucket_levels: inside every bucket, slice r (r a multiple of MSM_RADIX^(l+1)) takes in the sums of slices
//                     r + j * MSM_RADIX^l, j = 1 .. MSM_RADIX - 1; after the last level a bucket's sum is its first slice's
//   k_msm_chunks      one thread per (window, chunk of MSM_CHUNK buckets [lo, lo + MSM_CHUNK)): run = sum of B_d and acc = sum of
//                     (d - lo) * B_d by the two running sums
//   k_msm_chunk_lift  the same threads: acc + lo * run (lo < 2^c: a double-and-add of c bits); skipped when a window is one chunk
//   k_msm_level       x plan.chunk_levels: a window's chunk results combined the same way
//   k_msm_finish      one thread: from the top window down, a window's width of doublings and one addition per window; ONE inversion;
//                     (x, y) and the flag
// The multiply_then_sum route: gs_curve_mul (curve.hip) into workspace, k_msm_block_sum x plan.tree_levels (a workgroup adds 256 points
// through LDS; the first launch reads the affine products and their flags), k_msm_finish.
#include "common.h"
#include "curve_jac.h"
#include "msm_plan.h"
#include "../../include/gstark_curve.h"
#include "../../include/gstark_msm.h"

#include <stdlib.h>

// counters[key] += 1 for every active lane; returns the value the lane's own increment saw.  When every active lane of the wave holds the
// same key (a window of equal digits: the all-equal batch) ONE lane adds the wave's count and the lanes take consecutive values: 64 times
// fewer atomics on the one address everybody wants.  Every lane of the wave must call it.
__device__ __forceinline__ uint32_t msm_count(uint32_t *__restrict__ counters, bool active, uint32_t key) {
    const uint64_t mask = __ballot(active);
    if (!mask) return 0;
    const int first = __ffsll((long long)mask) - 1, lane = (int)(threadIdx.x & 63);
    const uint32_t key0 = (uint32_t)__shfl((int)key, first);
    if (__ballot(active && key == key0) == mask) {                           // (uniform: a ballot)
        uint32_t base = 0;
        if (lane == first) base = atomicAdd(&counters[key0], (uint32_t)__popcll(mask));
        base = (uint32_t)__shfl((int)base, first);
        return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
    }
    return active ? atomicAdd(&counters[key], 1u) : 0;
}

template <bool SCATTER>
__global__ __launch_bounds__(MSM_BLOCK_PAIRS) void k_msm_pairs(const uint32_t *__restrict__ scalars, uint32_t stride, uint32_t bits, uint32_t c, uint32_t windows,
                                                                uint64_t count, uint64_t pairs, uint32_t *__restrict__ counters, uint32_t *__restrict__ sorted) {
    const uint64_t i = (uint64_t)blockIdx.x * MSM_BLOCK_PAIRS + threadIdx.x;
    bool active = i < pairs;
    uint32_t key = 0, term = 0;
    if (active) {
        uint32_t window;
        uint64_t t;
        msm_pair(count, i, &window, &t);
        const uint32_t digit = msm_digit(scalars + t * (stride / 4), stride, bits, windows, window);
        active = digit != 0;
        key = (window << c) + digit;
        term = (uint32_t)t;
    }
    const uint32_t at = msm_count(counters, active, key);
    if (SCATTER && active) sorted[at] = term;
}

// one workgroup: thread t owns entries [t * per, (t + 1) * per) of the n = keys + 1 counters (the last one is zero: the totals land there)
__global__ __launch_bounds__(MSM_SCAN_THREADS) void k_msm_scan(uint32_t *__restrict__ start, uint32_t *__restrict__ cursor, uint32_t *__restrict__ slice_start, uint64_t n) {
    __shared__ uint32_t sums[2][MSM_SCAN_THREADS];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (n + MSM_SCAN_THREADS - 1) / MSM_SCAN_THREADS;
    const uint64_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t points = 0, slices = 0;
    for (uint64_t i = lo; i < hi; i++) {
        const uint32_t v = start[i];
        points += v;
        slices += (v + MSM_SLICE - 1) / MSM_SLICE;
    }
    sums[0][t] = points; sums[1][t] = slices;
    __syncthreads();
    for (uint32_t step = 1; step < MSM_SCAN_THREADS; step <<= 1) {           // inclusive sums over the threads
        const uint32_t p = t >= step ? sums[0][t - step] : 0, s = t >= step ? sums[1][t - step] : 0;
        __syncthreads();
        sums[0][t] += p; sums[1][t] += s;
        __syncthreads();
    }
    points = sums[0][t] - points; slices = sums[1][t] - slices;               // exclusive: what lies before this thread's entries
    for (uint64_t i = lo; i < hi; i++) {
        const uint32_t v = start[i];
        start[i] = points; cursor[i] = points; slice_start[i] = slices;
        points += v;
        slices += (v + MSM_SLICE - 1) / MSM_SLICE;
    }
}

__global__ __launch_bounds__(MSM_BLOCK_POINTS) void k_msm_slices(const fe a, const fe *__restrict__ points, const uint32_t *__restrict__ start,
                                                                  const uint32_t *__restrict__ slice_start, uint32_t keys, const uint32_t *__restrict__ sorted,
                                                                  uint32_t *__restrict__ slice_key, jac *__restrict__ partial) {
    const uint32_t s = blockIdx.x * MSM_BLOCK_POINTS + threadIdx.x;
    if (s >= slice_start[keys]) return;
    uint32_t lo = 0, hi = keys;                                              // the last key with slice_start[key] <= s: the one bucket that owns slice s
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (slice_start[mid] <= s) lo = mid; else hi = mid - 1;
    }
    const uint32_t key = lo, first = start[key] + (s - slice_start[key]) * MSM_SLICE, stop = start[key + 1];
    const uint32_t end = first + MSM_SLICE < stop ? first + MSM_SLICE : stop;
    jac acc = jac_infinity();
#pragma unroll 1
    for (uint32_t j = first; j < end; j++) {
        const fe *__restrict__ pt = points + 2 * (uint64_t)sorted[j];
        acc = jac_add_affine(acc, pt[0], pt[1], a);
    }
    partial[s] = acc;
    slice_key[s] = key;
}

// partial[s] += partial[s + j * stride], j = 1 .. MSM_RADIX - 1, for the element of rank r (a multiple of MSM_RADIX * stride) in a segment of m
__device__ __forceinline__ void msm_combine(const fe &a, jac *__restrict__ partial, uint64_t s, uint64_t r, uint64_t m, uint64_t stride) {
    if (r % (MSM_RADIX * stride) || r + stride >= m) return;
    jac acc = partial[s];
#pragma unroll 1
    for (uint32_t j = 1; j < MSM_RADIX && r + j * stride < m; j++) acc = jac_add(acc, partial[s + j * stride], a);
    partial[s] = acc;
}

__global__ __launch_bounds__(MSM_BLOCK_POINTS) void k_msm_bucket_level(const fe a, jac *__restrict__ partial, const uint32_t *__restrict__ slice_key,
                                                                        const uint32_t *__restrict__ slice_start, uint32_t keys, uint64_t stride) {
    const uint32_t s = blockIdx.x * MSM_BLOCK_POINTS + threadIdx.x;
    if (s >= slice_start[keys]) return;
    const uint32_t key = slice_key[s], first = slice_start[key];
    msm_combine(a, partial, s, s - first, slice_start[key + 1] - first, stride);
}

// `total` elements in segments of m (the last one may be short only when there is one segment)
__global__ __launch_bounds__(MSM_BLOCK_POINTS) void k_msm_level(const fe a, jac *__restrict__ partial, uint64_t m, uint64_t total, uint64_t stride) {
    const uint64_t s = (uint64_t)blockIdx.x * MSM_BLOCK_POINTS + threadIdx.x;
    if (s >= total) return;
    msm_combine(a, partial, s, s % m, m, stride);
}

// a point in LDS, one limb per row, one column per lane (no bank conflicts): a register file extension for k_msm_chunks, and the way
// points cross lanes in k_msm_block_sum
template <uint32_t N>
__device__ __forceinline__ void msm_park(uint32_t (*rows)[N], uint32_t col, const jac &p) {
#pragma unroll
    for (int i = 0; i < GF_LIMBS; i++) {
        rows[i][col] = fe_limb(p.X, i); rows[GF_LIMBS + i][col] = fe_limb(p.Y, i); rows[2 * GF_LIMBS + i][col] = fe_limb(p.Z, i);
    }
}
template <uint32_t N>
__device__ __forceinline__ jac msm_unpark(uint32_t (*rows)[N], uint32_t col) {
    jac p;
#pragma unroll
    for (int i = 0; i < GF_LIMBS; i++) {
        fe_set_limb(p.X, i, rows[i][col]); fe_set_limb(p.Y, i, rows[GF_LIMBS + i][col]); fe_set_limb(p.Z, i, rows[2 * GF_LIMBS + i][col]);
    }
    return p;
}

__global__ __launch_bounds__(MSM_BLOCK_POINTS) void k_msm_chunks(const fe a, const jac *__restrict__ partial, const uint32_t *__restrict__ slice_start, uint32_t c,
                                                                  uint32_t windows, uint32_t chunk, uint64_t chunks, jac *__restrict__ chunk_sums, jac *__restrict__ chunk_runs) {
    const uint64_t t = (uint64_t)blockIdx.x * MSM_BLOCK_POINTS + threadIdx.x;
    if (t >= windows * chunks) return;
    uint32_t window, lo, hi;
    msm_chunk_range(chunks, chunk, t, &window, &lo, &hi);
    const uint32_t base = window << c;
    // acc waits in LDS while run takes in a bucket: three points and the temporaries of an addition do not fit the 224-bit flavour's
    // registers.  One limb per lane and row: no bank conflicts
    __shared__ uint32_t parked[3 * GF_LIMBS][MSM_BLOCK_POINTS];
    jac run = jac_infinity();
    msm_park(parked, threadIdx.x, jac_infinity());
    // digits hi - 1 down to lo, two steps each: run += B_d, then (but for d == lo) acc += run.  Digit 0 has no bucket.
#pragma unroll 1
    for (uint32_t i = 0; i < 2 * (hi - lo) - 1; i++) {                        // (uniform: hi - lo is the same in every lane)
        const uint32_t d = hi - 1 - i / 2;
        jac other;
        if (i & 1) {
            other = msm_unpark(parked, threadIdx.x);
        } else {
            other = jac_infinity();
            if (d) {
                const uint32_t first = slice_start[base + d];
                if (slice_start[base + d + 1] != first) other = partial[first];
            }
        }
        const jac sum = jac_add(run, other, a);
        if (i & 1) msm_park(parked, threadIdx.x, sum); else run = sum;
    }
    const jac acc = msm_unpark(parked, threadIdx.x);
    chunk_sums[t] = acc;
    chunk_runs[t] = run;
}

// chunk_sums[t] += lo * chunk_runs[t], lo < 2^c the chunk's first digit: c doublings and as many additions as lo has bits set.  A launch
// of its own: with the running sums in the same kernel the 224-bit flavour spills.
__global__ __launch_bounds__(MSM_BLOCK_POINTS) void k_msm_chunk_lift(const fe a, uint32_t c, uint32_t windows, uint32_t chunk, uint64_t chunks,
                                                                      jac *__restrict__ chunk_sums, const jac *__restrict__ chunk_runs) {
    const uint64_t t = (uint64_t)blockIdx.x * MSM_BLOCK_POINTS + threadIdx.x;
    if (t >= windows * chunks) return;
    uint32_t window, lo, hi;
    msm_chunk_range(chunks, chunk, t, &window, &lo, &hi);
    if (!lo) return;
    const jac run = chunk_runs[t];
    jac lifted = jac_infinity();
#pragma unroll 1
    for (uint32_t k = 0; k <= 2 * c; k++) {                                  // even k doubles, odd k adds `run` where bit c - 1 - k / 2 of lo is set; k == 2 c adds chunk_sums[t]
        const bool last = k == 2 * c;
        if (!last && !(k & 1)) { lifted = jac_double(lifted, a); continue; }
        if (!last && !((lo >> (c - 1 - k / 2)) & 1u)) continue;
        jac rhs = run;
        if (last) rhs = chunk_sums[t];
        lifted = jac_add(lifted, rhs, a);
    }
    chunk_sums[t] = lifted;
}

// out[block] = the sum of the block's MSM_BLOCK_SUM points: `in` (Jacobian), or with AFFINE rows of (x, y) and a flag byte each (what
// gs_curve_mul wrote).  A binary tree through LDS: 8 additions in a row.
template <bool AFFINE>
__global__ __launch_bounds__(MSM_BLOCK_SUM) void k_msm_block_sum(const fe a, const fe *__restrict__ points, const uint8_t *__restrict__ inf, const jac *__restrict__ in,
                                                                  uint64_t n, jac *__restrict__ out) {
    __shared__ uint32_t rows[3 * GF_LIMBS][MSM_BLOCK_SUM];
    const uint32_t t = threadIdx.x;
    const uint64_t k = (uint64_t)blockIdx.x * MSM_BLOCK_SUM + t;
    jac mine = jac_infinity();
    if (k < n) {
        if (!AFFINE) mine = in[k];
        else if (!inf[k]) { mine.X = points[2 * k]; mine.Y = points[2 * k + 1]; mine.Z = fe_one(); }
    }
    msm_park(rows, t, mine);
    __syncthreads();
#pragma unroll 1
    for (uint32_t stride = MSM_BLOCK_SUM / 2; stride; stride >>= 1) {        // thread t < stride takes in column t + stride, which its owner wrote before the barrier
        if (t < stride) {
            mine = jac_add(mine, msm_unpark(rows, t + stride), a);
            msm_park(rows, t, mine);
        }
        __syncthreads();
    }
    if (!t) out[blockIdx.x] = mine;
}

// sum over w of 2^msm_window_lo(w) * sums[w * stride], from the top window down; one thread
__global__ __launch_bounds__(MSM_BLOCK_POINTS) void k_msm_finish(const fe a, const jac *__restrict__ sums, uint64_t stride, uint32_t windows, uint32_t bits,
                                                                  fe *__restrict__ out, uint8_t *__restrict__ inf_out) {
    if (blockIdx.x || threadIdx.x) return;
    jac acc = jac_infinity();
#pragma unroll 1
    for (int w = (int)windows - 1; w >= 0; w--) {
        const uint32_t width = w == (int)windows - 1 ? 0 : msm_window_lo(bits, windows, w + 1) - msm_window_lo(bits, windows, w);
#pragma unroll 1
        for (uint32_t i = 0; i < width; i++) acc = jac_double(acc, a);
        acc = jac_add(acc, sums[(uint64_t)w * stride], a);
    }
    const bool inf = fe_is_zero(acc.Z);
    const fe zi = fe_inv(acc.Z), zi2 = fe_sqr(zi);                           // (0 -> 0)
    out[0] = fe_select(inf, fe_zero(), fe_mul(acc.X, zi2));
    out[1] = fe_select(inf, fe_zero(), fe_mul(acc.Y, fe_mul(zi2, zi)));
    inf_out[0] = inf ? 1 : 0;
}

namespace {

int msm_levels_launch(gs_ctx *c, const fe &a, jac *partial, uint64_t m, uint64_t total, uint32_t levels, unsigned grid) {
    uint64_t stride = 1;
    for (uint32_t l = 0; l < levels; l++, stride *= MSM_RADIX) {
        gs_traffic(c, total / stride * sizeof(jac), total / stride / MSM_RADIX * (MSM_RADIX - 1) * GS_CURVE_FULL_ADD_PRODUCTS, "k_msm_level");
        hipLaunchKernelGGL(k_msm_level, dim3(grid), dim3(MSM_BLOCK_POINTS), 0, c->stream, a, partial, m, total, stride);
    }
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

}  // namespace

extern "C" {

int gs_curve_msm(gs_ctx *c, const gs_elt *a_host, const void *points, const void *scalars, uint32_t scalar_stride, uint32_t bits, uint64_t count,
                 uint32_t window, void *out, void *inf_out) {
    if (!c) return GS_ERR_ARG;
    if (!a_host) return gs_fail(c, GS_ERR_ARG, "curve_msm: a is required");
    const fe a = fe_from_bytes(a_host);
    if (fe_ge_p(a)) return gs_fail(c, GS_ERR_ARG, "curve_msm: a is not a canonical element");
    int force = -1;                                                          // the measurement's handle on the route of window 0 (tools/msm_bench.py)
    if (const char *env = getenv("GSTARK_MSM_ROUTE")) force = !strcmp(env, "multiply_then_sum") ? MSM_ROUTE_MULTIPLY_THEN_SUM : (!strcmp(env, "buckets") ? MSM_ROUTE_BUCKETS : -1);
    msm_plan p;
    if (const char *why = msm_plan_build(count, bits, window, (uint32_t)GS_ELT, scalar_stride, p, force))
        return gs_fail(c, GS_ERR_ARG, "curve_msm: %s (count %llu, scalar_stride %u, bits %u, window %u)", why, (unsigned long long)count, scalar_stride, bits, window);
    if (!out || !inf_out) return gs_fail(c, GS_ERR_ARG, "curve_msm: out and inf_out are required");
    if (count && (!points || !scalars)) return gs_fail(c, GS_ERR_ARG, "curve_msm: points and scalars are required");
    if (!count) {                                                            // the empty sum
        GS_HIP(c, hipMemsetAsync(out, 0, 2 * GS_ELT, c->stream));
        GS_HIP(c, hipMemsetAsync(inf_out, 1, 1, c->stream));
        return GS_OK;
    }
    void *block = nullptr;
    int rc = gs_tmp_alloc(c, p.workspace, &block);
    if (rc) return rc;
    uint8_t *ws = (uint8_t *)block;
    jac *partial = (jac *)(ws + p.off_partial);
    const dim3 wave(MSM_BLOCK_POINTS);
    if (p.route == MSM_ROUTE_MULTIPLY_THEN_SUM) {
        const void *wide = scalars;
        hipError_t e = hipSuccess;
        if (scalar_stride != 32) {                                           // gs_curve_mul reads 32-byte scalars
            wide = ws + p.off_scalars;
            e = hipMemsetAsync(ws + p.off_scalars, 0, count * 32, c->stream);
            if (e == hipSuccess) e = hipMemcpy2DAsync(ws + p.off_scalars, 32, scalars, scalar_stride, scalar_stride, count, hipMemcpyDeviceToDevice, c->stream);
        }
        if (e != hipSuccess) rc = gs_fail(c, GS_ERR_DEVICE, "curve_msm: widening the scalars: %s", hipGetErrorString(e));
        if (!rc) rc = gs_curve_mul(c, a_host, points, count, wide, bits, nullptr, nullptr, count, ws + p.off_products, ws + p.off_flags);
        const jac *sums = partial;
        if (!rc) {
            jac *to = partial, *other = (jac *)(ws + p.off_partial_b);
            uint64_t left = count;
            for (uint32_t l = 0; l < p.tree_levels; l++) {
                const unsigned grid = (unsigned)((left + MSM_BLOCK_SUM - 1) / MSM_BLOCK_SUM);
                gs_traffic(c, left * (l ? sizeof(jac) : 2 * GS_ELT + 1), left * GS_CURVE_FULL_ADD_PRODUCTS, "k_msm_block_sum");
                if (!l)
                    hipLaunchKernelGGL(k_msm_block_sum<true>, dim3(grid), dim3(MSM_BLOCK_SUM), 0, c->stream, a, (const fe *)(ws + p.off_products), (const uint8_t *)(ws + p.off_flags),
                                       (const jac *)nullptr, left, to);
                else
                    hipLaunchKernelGGL(k_msm_block_sum<false>, dim3(grid), dim3(MSM_BLOCK_SUM), 0, c->stream, a, (const fe *)nullptr, (const uint8_t *)nullptr, sums, left, to);
                sums = to;
                jac *swap = to; to = other; other = swap;
                left = grid;
            }
        }
        if (!rc) hipLaunchKernelGGL(k_msm_finish, dim3(1), wave, 0, c->stream, a, sums, (uint64_t)0, 1u, bits, (fe *)out, (uint8_t *)inf_out);
    } else {
        uint32_t *start = (uint32_t *)(ws + p.off_start), *cursor = (uint32_t *)(ws + p.off_cursor), *slice_start = (uint32_t *)(ws + p.off_slice_start);
        uint32_t *sorted = (uint32_t *)(ws + p.off_sorted), *slice_key = (uint32_t *)(ws + p.off_slice_key);
        jac *chunk_sums = (jac *)(ws + p.off_chunk_sums), *chunk_runs = (jac *)(ws + p.off_chunk_runs);
        const uint32_t keys = (uint32_t)p.keys;
        hipError_t e = hipMemsetAsync(start, 0, (p.keys + 1) * 4, c->stream);
        if (e != hipSuccess) rc = gs_fail(c, GS_ERR_DEVICE, "curve_msm: clearing the counters: %s", hipGetErrorString(e));
        if (!rc) {
            gs_traffic(c, p.pairs * 12, 0, "k_msm_pairs<histogram>");
            hipLaunchKernelGGL(k_msm_pairs<false>, dim3(p.grid_pairs), dim3(MSM_BLOCK_PAIRS), 0, c->stream, (const uint32_t *)scalars, scalar_stride, bits, p.c, p.windows, count, p.pairs,
                               start, (uint32_t *)nullptr);
            gs_traffic(c, (p.keys + 1) * 16, 0, "k_msm_scan");
            hipLaunchKernelGGL(k_msm_scan, dim3(1), dim3(MSM_SCAN_THREADS), 0, c->stream, start, cursor, slice_start, p.keys + 1);
            gs_traffic(c, p.pairs * 16, 0, "k_msm_pairs<scatter>");
            hipLaunchKernelGGL(k_msm_pairs<true>, dim3(p.grid_pairs), dim3(MSM_BLOCK_PAIRS), 0, c->stream, (const uint32_t *)scalars, scalar_stride, bits, p.c, p.windows, count, p.pairs,
                               cursor, sorted);
            gs_traffic(c, p.pairs * (4 + 2 * GS_ELT) + p.slices_max * sizeof(jac), p.pairs * GS_CURVE_ADD_PRODUCTS, "k_msm_slices");
            hipLaunchKernelGGL(k_msm_slices, dim3(p.grid_slices), wave, 0, c->stream, a, (const fe *)points, (const uint32_t *)start, (const uint32_t *)slice_start, keys,
                               (const uint32_t *)sorted, slice_key, partial);
            uint64_t stride = 1;
            for (uint32_t l = 0; l < p.bucket_levels; l++, stride *= MSM_RADIX) {
                gs_traffic(c, p.slices_max / stride * sizeof(jac), p.slices_max / stride / MSM_RADIX * (MSM_RADIX - 1) * GS_CURVE_FULL_ADD_PRODUCTS, "k_msm_bucket_level");
                hipLaunchKernelGGL(k_msm_bucket_level, dim3(p.grid_slices), wave, 0, c->stream, a, partial, (const uint32_t *)slice_key, (const uint32_t *)slice_start, keys, stride);
            }
            gs_traffic(c, p.keys * (sizeof(jac) + 4), p.windows * p.chunks * 2ull * p.chunk * GS_CURVE_FULL_ADD_PRODUCTS, "k_msm_chunks");
            hipLaunchKernelGGL(k_msm_chunks, dim3(p.grid_chunks), wave, 0, c->stream, a, (const jac *)partial, (const uint32_t *)slice_start, p.c, p.windows, p.chunk, p.chunks,
                               chunk_sums, chunk_runs);
            if (p.chunks > 1) {
                gs_traffic(c, p.windows * p.chunks * 3 * sizeof(jac), p.windows * p.chunks * (p.c * 26ull + 16), "k_msm_chunk_lift");
                hipLaunchKernelGGL(k_msm_chunk_lift, dim3(p.grid_chunks), wave, 0, c->stream, a, p.c, p.windows, p.chunk, p.chunks, chunk_sums, (const jac *)chunk_runs);
            }
            rc = msm_levels_launch(c, a, chunk_sums, p.chunks, p.windows * p.chunks, p.chunk_levels, p.grid_chunk_tree);
        }
        if (!rc) {
            gs_traffic(c, p.windows * sizeof(jac), (uint64_t)bits * GS_CURVE_DOUBLE_PRODUCTS + p.windows * GS_CURVE_FULL_ADD_PRODUCTS, "k_msm_finish");
            hipLaunchKernelGGL(k_msm_finish, dim3(1), wave, 0, c->stream, a, (const jac *)chunk_sums, p.chunks, p.windows, bits, (fe *)out, (uint8_t *)inf_out);
        }
    }
    gs_tmp_free(c, block);                                                   // (parked in the context's cache: every later user is ordered on the stream)
    if (rc) return rc;
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

}  // extern "C"
