// diagnose.hip — gs_nonzero_spans (include/gstark_diagnose.h): per row of a matrix of canonical elements, how many are non-zero and where
// the first and the last of them lie.  The diagnosis of a statement (csrc/diagnose.h) asks it twice: over constraints x steps ("which
// constraint fails at which steps") and over the constraints' coefficient rows ("last non-zero coefficient" = the measured degree).
//
// A memory-bound pass that reads every scanned byte once and writes 24 bytes per workgroup:
//   loads       the matrix is read as 16-byte words, one per lane per load, consecutive lanes at consecutive addresses; a lane has four
//               loads in flight per trip of its grid-stride loop.  An element is zero exactly when all its words are: with 32-byte
//               elements the two words of an element sit in neighbouring lanes (word index = multiple of the block size + lane, a row
//               starts on an element) and one shuffle joins them; the even lane counts the element.
//   per thread  a running (count, first, last + 1) in registers — no arrays, no scratch.
//   reduction   the wave by shuffles, the workgroup's four waves through 96 bytes of LDS, workgroups through a partials buffer
//               (rows x blocks x 3) that a second, small launch folds: one wave per row, lanes over the blocks.  No atomics.
//   read-back   the second launch writes the rows' results into the context's mapped staging memory (the path of gs_gather); the entry
//               synchronises the stream once and copies them out.
// Words of the columns [n, row_stride) are never addressed: a thread's word index stays below n * (words per element).
#include "common.h"
#include "../../include/gstark_diagnose.h"

#define GS_SPANS_BLOCK 256
#define GS_SPANS_LOADS 4                     // 16-byte loads in flight per lane
#define GS_SPANS_TRIPS 4                     // a row is given enough workgroups for about this many trips per lane, ...
#define GS_SPANS_MAX_BLOCKS 256              // ... at most this many (the second launch folds them with one wave)
#define GS_SPANS_GRID 2048                   // workgroups of the whole launch: 8 per compute unit

struct Span { unsigned long long count, first, last1; };       // last1 = last + 1; 0: none

__device__ __forceinline__ void span_join(Span &a, unsigned long long count, unsigned long long first, unsigned long long last1) {
    a.count += count;
    a.first = first < a.first ? first : a.first;
    a.last1 = last1 > a.last1 ? last1 : a.last1;
}
__device__ __forceinline__ Span span_wave(Span s) {             // every lane of the wave takes part; lane 0 holds the wave's
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) span_join(s, __shfl_down(s.count, d), __shfl_down(s.first, d), __shfl_down(s.last1, d));
    return s;
}

// partials[(row * gridDim.x + blockIdx.x) * 3 ..] = this workgroup's share of row `row`; EW = 16-byte words per element (1 or 2)
template <uint32_t EW>
__global__ __launch_bounds__(GS_SPANS_BLOCK) void k_nonzero_spans(const uint4 *__restrict__ m, uint64_t rows, uint64_t row_words, uint64_t scan_words,
                                                                   unsigned long long *__restrict__ partials) {
    __shared__ unsigned long long lds[GS_SPANS_BLOCK / 64][3];
    const uint64_t stride = (uint64_t)gridDim.x * GS_SPANS_BLOCK;
    for (uint64_t row = blockIdx.y; row < rows; row += gridDim.y) {               // (uniform over the workgroup)
        const uint4 *__restrict__ src = m + row * row_words;
        Span s{0, ~0ull, 0};
        // `base` is the same in every lane of the workgroup, so every lane runs every trip and takes part in the shuffle below
        for (uint64_t base = (uint64_t)blockIdx.x * GS_SPANS_BLOCK; base < scan_words; base += GS_SPANS_LOADS * stride) {
            uint4 v[GS_SPANS_LOADS];
#pragma unroll
            for (int k = 0; k < GS_SPANS_LOADS; k++) {
                const uint64_t w = base + k * stride + threadIdx.x;
                v[k] = w < scan_words ? src[w] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int k = 0; k < GS_SPANS_LOADS; k++) {
                const uint64_t w = base + k * stride + threadIdx.x;
                uint32_t nz = v[k].x | v[k].y | v[k].z | v[k].w;
                if (EW == 2) nz |= __shfl_xor(nz, 1);                             // the other half of the element (scan_words is even: both or neither in range)
                if (nz && (w % EW) == 0) { const uint64_t e = w / EW; span_join(s, 1, e, e + 1); }
            }
        }
        s = span_wave(s);
        const uint32_t wave = threadIdx.x / 64;
        if ((threadIdx.x & 63) == 0) { lds[wave][0] = s.count; lds[wave][1] = s.first; lds[wave][2] = s.last1; }
        __syncthreads();
        if (threadIdx.x == 0) {
            Span t{0, ~0ull, 0};
#pragma unroll
            for (int i = 0; i < GS_SPANS_BLOCK / 64; i++) span_join(t, lds[i][0], lds[i][1], lds[i][2]);
            unsigned long long *out = partials + (row * gridDim.x + blockIdx.x) * 3;
            out[0] = t.count; out[1] = t.first; out[2] = t.last1;
        }
        __syncthreads();                                                          // the next row reuses lds
    }
}

// one wave per row folds the row's `blocks` partials; out: count[rows], first[rows], last[rows] (mapped host memory)
__global__ __launch_bounds__(64) void k_nonzero_spans_fold(const unsigned long long *__restrict__ partials, uint64_t rows, uint32_t blocks, uint64_t n,
                                                           unsigned long long *__restrict__ out) {
    for (uint64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        Span s{0, ~0ull, 0};
        for (uint32_t b = threadIdx.x; b < blocks; b += 64) {
            const unsigned long long *p = partials + (row * blocks + b) * 3;
            span_join(s, p[0], p[1], p[2]);
        }
        s = span_wave(s);
        if (threadIdx.x == 0) {
            out[row] = s.count;
            out[rows + row] = s.count ? s.first : n;
            out[2 * rows + row] = s.count ? s.last1 - 1 : n;
        }
    }
}

extern "C" int gs_nonzero_spans(gs_ctx *c, const void *m, uint64_t rows, uint64_t row_stride, uint64_t n, uint64_t *count_host, uint64_t *first_host,
                                uint64_t *last_host) {
    if (!c) return GS_ERR_ARG;
    if (!m || !count_host || !first_host || !last_host) return gs_fail(c, GS_ERR_ARG, "nonzero_spans: the matrix and the three result arrays are required");
    if ((uintptr_t)m % 16) return gs_fail(c, GS_ERR_ARG, "nonzero_spans: the matrix is not aligned to 16 bytes");
    if (!rows) return gs_fail(c, GS_ERR_ARG, "nonzero_spans: a matrix of 0 rows");
    if (!n) return gs_fail(c, GS_ERR_ARG, "nonzero_spans: 0 columns to scan");
    if (n > row_stride) return gs_fail(c, GS_ERR_ARG, "nonzero_spans: %llu columns to scan in rows of %llu", (unsigned long long)n, (unsigned long long)row_stride);
    if (rows > (1ull << 32) || row_stride > (1ull << 40) || rows * row_stride > (1ull << 44))
        return gs_fail(c, GS_ERR_ARG, "nonzero_spans: a matrix of %llu x %llu elements", (unsigned long long)rows, (unsigned long long)row_stride);
    const uint64_t scan_words = n * GS_EW;
    const unsigned gy = (unsigned)(rows < 65535 ? rows : 65535);
    uint64_t blocks = (scan_words + GS_SPANS_BLOCK * GS_SPANS_LOADS * GS_SPANS_TRIPS - 1) / (GS_SPANS_BLOCK * GS_SPANS_LOADS * GS_SPANS_TRIPS);
    const uint64_t room = GS_SPANS_GRID / gy ? GS_SPANS_GRID / gy : 1;
    if (blocks > room) blocks = room;
    if (blocks > GS_SPANS_MAX_BLOCKS) blocks = GS_SPANS_MAX_BLOCKS;
    void *partials = nullptr;
    int rc = gs_tmp_alloc(c, rows * blocks * 3 * sizeof(unsigned long long), &partials);
    if (rc) return rc;
    rc = gs_stage_reserve(c, rows * 3 * sizeof(unsigned long long));
    if (rc) { gs_tmp_free(c, partials); return rc; }
    gs_traffic(c, rows * n * GS_ELT, rows * n, "k_nonzero_spans");
    hipLaunchKernelGGL(k_nonzero_spans<GS_EW>, dim3((unsigned)blocks, gy), dim3(GS_SPANS_BLOCK), 0, c->stream, (const uint4 *)m, rows, row_stride * GS_EW, scan_words,
                       (unsigned long long *)partials);
    hipLaunchKernelGGL(k_nonzero_spans_fold, dim3((unsigned)(rows < 1024 ? rows : 1024)), dim3(64), 0, c->stream, (const unsigned long long *)partials, rows,
                       (uint32_t)blocks, n, (unsigned long long *)c->h_stage_dev);
    gs_tmp_free(c, partials);                              // (parked in the context's cache; every later user is ordered on the stream)
    GS_LAUNCH_CHECK(c);
    GS_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t *got = (const uint64_t *)c->h_stage;
    memcpy(count_host, got, rows * 8);
    memcpy(first_host, got + rows, rows * 8);
    memcpy(last_host, got + 2 * rows, rows * 8);
    return GS_OK;
}
