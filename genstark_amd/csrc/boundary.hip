// boundary.hip — the boundary polynomials of registers with many assertions (include/gstark_boundary.h; BoundaryConstraints.ts:15-45),
// built where the proof needs them.  Per asserted register r with assertions (s_i, y_i), x_i = g^(s_i), g of order T:
//   Z_r(x) = prod (x - x_i)                  a product tree: pair products level by level, schoolbook while the operands are short,
//                                            through the batched NTT (gs_eval_polys_at_roots / gs_interpolate_roots, rows > 1) above;
//   c_i   = y_i / Z_r'(x_i)                  Z_r' at ALL points of the execution domain is one T-point transform, the m wanted values a
//                                            gather at the steps, one batch inversion (gs_vec_div);
//   W(x)  = sum_k x^k sum_i c_i x_i^-(k+1)   one T-point transform (root g^-1) of the sparse vector holding c_i at s_i, read one place on:
//                                            sum_i c_i / (x - x_i) = W(x) / (x^T - 1) because x_i^T = 1;
//   I_r   = (Z_r W) div x^T                  Z_r W = (x^T - 1) I_r and deg I_r < m <= T: the coefficients T .. T + m - 1 of one product
//                                            through 2T-point transforms.
// All rows of a statement share every launch.  Tree layout: level l holds W >> l nodes per row (W = the width rounded up to a power of
// two), a node is a polynomial of degree <= 2^l in a slot of 2 << l elements; a leaf is x - x_i, or the constant 1 beyond a row's count.
#include <atomic>

#include "common.h"
#include "../../include/gstark_boundary.h"

// Pair products whose operands lie in slots of at most 2^g_schoolbook_log2 elements are schoolbook products.  Measured (profiles/
// boundary_polys.md: 4 rows x 4 096 assertions, T = 2^16, ms per call by this exponent): 4: 0.871, 6: 0.782, 7: 0.772, 8: 0.753, 9: 0.786,
// 10: 0.899 — below 2^8 the batched transforms of many short nodes are launch-bound, above it the quadratic products cost more.
static std::atomic<uint32_t> g_schoolbook_log2{8};

// leaves: slot 2
__global__ __launch_bounds__(256) void k_bd_leaves(const uint64_t *__restrict__ steps, const uint32_t *__restrict__ per_row, uint32_t rows, uint32_t width,
                                                   uint64_t W, fe g, fe *__restrict__ nodes) {
    const uint64_t total = (uint64_t)rows * W;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = t / W, i = t % W;
        fe lo = fe_one(), hi = fe_zero();
        if (i < per_row[r]) { lo = fe_neg(fe_pow_u64(g, steps[r * width + i])); hi = fe_one(); }
        nodes[2 * t] = lo;
        nodes[2 * t + 1] = hi;
    }
}

// one level of the tree, schoolbook: `in` holds nodes of slot `slot` (degree <= slot / 2), `out` their pair products in slots of
// 2 * slot; one thread per output coefficient
__global__ __launch_bounds__(256) void k_bd_pair_schoolbook(const fe *__restrict__ in, uint64_t total_out, uint32_t slot, fe *__restrict__ out) {
    const uint32_t oslot = 2 * slot, la = slot / 2 + 1;          // operands of `la` coefficients
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total_out; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t node = t / oslot;
        const uint32_t k = (uint32_t)(t % oslot);
        const fe *a = in + node * oslot, *b = a + slot;
        fe acc = fe_zero();
        if (k <= 2 * (la - 1)) {
            const uint32_t j0 = k >= la ? k - la + 1 : 0, j1 = k < la ? k : la - 1;
            for (uint32_t j = j0; j <= j1; j++) acc = fe_add(acc, fe_mul(a[j], b[k - j]));
        }
        out[t] = acc;
    }
}

// values of the nodes over n points side by side: the product of every pair
__global__ __launch_bounds__(256) void k_bd_pair_pointwise(const fe *__restrict__ ev, uint64_t total_out, uint64_t n, fe *__restrict__ out) {
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total_out; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t node = t / n, k = t % n;
        out[t] = fe_mul(ev[2 * node * n + k], ev[(2 * node + 1) * n + k]);
    }
}

// Z' from Z: row r's Z in a slot of 2W, its derivative in W coefficients
__global__ __launch_bounds__(256) void k_bd_derivative(const fe *__restrict__ z, uint32_t rows, uint64_t W, fe *__restrict__ out) {
    const uint64_t total = (uint64_t)rows * W;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = t / W, k = t % W;
        out[t] = fe_mul(fe_make((uint32_t)(k + 1), (uint32_t)((k + 1) >> 32), 0, 0), z[r * 2 * W + k + 1]);
    }
}

// the denominators Z_r'(x_i) out of Z_r' over the execution domain (1 beyond a row's count, where the numerator is 0)
__global__ __launch_bounds__(256) void k_bd_gather(const fe *__restrict__ zd, const uint64_t *__restrict__ steps, const uint32_t *__restrict__ per_row,
                                                   uint32_t rows, uint32_t width, uint64_t T, fe *__restrict__ den) {
    const uint64_t total = (uint64_t)rows * width;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = t / width, i = t % width;
        den[t] = i < per_row[r] ? zd[r * T + steps[t]] : fe_one();
    }
}
// the weights to their steps in a zeroed rows x T matrix (the steps of a row are distinct: no two threads write one cell)
__global__ __launch_bounds__(256) void k_bd_scatter(const fe *__restrict__ cw, const uint64_t *__restrict__ steps, const uint32_t *__restrict__ per_row,
                                                    uint32_t rows, uint32_t width, uint64_t T, fe *__restrict__ w) {
    const uint64_t total = (uint64_t)rows * width;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = t / width, i = t % width;
        if (i < per_row[r]) w[r * T + steps[t]] = cw[t];
    }
}
// out[k] = v[(k + 1) mod T] per row
__global__ __launch_bounds__(256) void k_bd_shift(const fe *__restrict__ v, uint32_t rows, uint64_t T, fe *__restrict__ out) {
    const uint64_t total = (uint64_t)rows * T;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = t / T, k = t % T;
        out[t] = v[r * T + ((k + 1) & (T - 1))];
    }
}
// the results in the caller's layout: I_r = coefficients T .. T + m - 1 of the product, Z_r = the tree's top node; zero-extended
__global__ __launch_bounds__(256) void k_bd_take(const fe *__restrict__ prod, const fe *__restrict__ z, const uint32_t *__restrict__ per_row, uint32_t rows,
                                                 uint32_t width, uint64_t T, uint64_t W, fe *__restrict__ i_out, fe *__restrict__ z_out) {
    const uint64_t zw = (uint64_t)width + 1, total = (uint64_t)rows * zw;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = t / zw, k = t % zw;
        const uint32_t m = per_row[r];
        z_out[t] = k <= m ? z[r * 2 * W + k] : fe_zero();
        if (k < width) i_out[r * width + k] = k < m ? prod[r * 2 * T + T + k] : fe_zero();
    }
}

// ---- many polynomials at many ARBITRARY points (gs_eval_polys_at_points): what a verifier needs of I_r, Z_r and the columns of public
// input registers — their values at the <= 128 queried points, which are no roots of a transform.  One workgroup per (row, block of
// GS_EP_POINTS points, segment of GS_EP_SEGMENT coefficients): thread t runs Horner in y = x^256 over the coefficients = t (mod 256) of
// its segment (lanes read neighbouring coefficients, every coefficient loaded serves all points of the block), then
//   sum_t x^t a_t   is folded through LDS: a_t += x^h a_(t+h) for h = 128, 64, .. 1 — the powers x^(2^k) are the squarings that lead to y.
// A second small launch combines the segments (Horner in x^GS_EP_SEGMENT).  Field addition is exact: the value does not depend on how
// the sum is split, so neither on these two constants.
#define GS_EP_POINTS 4
#define GS_EP_SEGMENT 4096
__global__ __launch_bounds__(256) void k_eval_points_partial(const fe *__restrict__ polys, uint64_t stride, const uint64_t *__restrict__ lens,
                                                             const fe *__restrict__ points, uint32_t npoints, uint32_t nseg, fe *__restrict__ partial) {
    __shared__ fe xp[GS_EP_POINTS][9];                           // x^(2^k), k = 0 .. 8
    __shared__ fe red[GS_EP_POINTS][256];
    const uint32_t t = threadIdx.x, seg = blockIdx.x, pb = blockIdx.y, r = blockIdx.z;
    const uint64_t len = lens[r], start = (uint64_t)seg * GS_EP_SEGMENT;
    if (start >= len) return;                                    // (the whole workgroup: the combining launch reads the segments of `len` only)
    const uint64_t count = len - start < GS_EP_SEGMENT ? len - start : GS_EP_SEGMENT;
    if (t < GS_EP_POINTS) {
        const uint32_t k = pb * GS_EP_POINTS + t;
        fe x = k < npoints ? points[k] : fe_zero();
        for (int j = 0; j < 8; j++) { xp[t][j] = x; x = fe_mul(x, x); }
        xp[t][8] = x;
    }
    __syncthreads();
    fe y[GS_EP_POINTS], acc[GS_EP_POINTS];
#pragma unroll
    for (int p = 0; p < GS_EP_POINTS; p++) { y[p] = xp[p][8]; acc[p] = fe_zero(); }
    const fe *row = polys + (uint64_t)r * stride + start;
    // coefficients t, t + 256, ...: the highest first
    if (t < count) {
#pragma unroll 1
        for (int64_t i = (int64_t)(t + ((count - 1 - t) & ~255ull)); i >= 0; i -= 256) {
            const fe c = row[i];
#pragma unroll
            for (int p = 0; p < GS_EP_POINTS; p++) acc[p] = fe_add(fe_mul(acc[p], y[p]), c);
        }
    }
#pragma unroll
    for (int p = 0; p < GS_EP_POINTS; p++) red[p][t] = acc[p];
    __syncthreads();
    int k = 7;
#pragma unroll 1
    for (uint32_t h = 128; h >= 1; h >>= 1, k--) {
        if (t < h) {
#pragma unroll
            for (int p = 0; p < GS_EP_POINTS; p++) red[p][t] = fe_add(red[p][t], fe_mul(red[p][t + h], xp[p][k]));
        }
        __syncthreads();
    }
    if (t < GS_EP_POINTS) {
        const uint32_t q = pb * GS_EP_POINTS + t;
        if (q < npoints) partial[((uint64_t)r * nseg + seg) * npoints + q] = red[t][0];
    }
}
// out[r][k] = sum_s partial[r][s][k] x_k^(s * GS_EP_SEGMENT) over the segments row r has (none: 0)
__global__ __launch_bounds__(256) void k_eval_points_combine(const fe *__restrict__ partial, const uint64_t *__restrict__ lens, const fe *__restrict__ points,
                                                             uint32_t rows, uint32_t npoints, uint32_t nseg, fe *__restrict__ out) {
    const uint64_t total = (uint64_t)rows * npoints;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / npoints, k = i % npoints;
        const uint64_t segs = (lens[r] + GS_EP_SEGMENT - 1) / GS_EP_SEGMENT;
        fe acc = fe_zero();
        if (segs) {
            const fe *col = partial + r * nseg * npoints + k;
            acc = col[(segs - 1) * npoints];
            if (segs > 1) {
                const fe z = fe_pow_u64(points[k], GS_EP_SEGMENT);
                for (uint64_t s = segs - 1; s-- > 0;) acc = fe_add(fe_mul(acc, z), col[s * npoints]);
            }
        }
        out[i] = acc;
    }
}

namespace {

// device blocks of one call, returned to the context's cache on every way out
struct Blocks {
    gs_ctx *c;
    std::vector<void *> held;
    explicit Blocks(gs_ctx *ctx) : c(ctx) {}
    ~Blocks() { for (void *p : held) gs_tmp_free(c, p); }
    int get(uint64_t bytes, void **p) {
        const int rc = gs_tmp_alloc(c, bytes ? bytes : 16, p);
        if (rc == GS_OK) held.push_back(*p);
        return rc;
    }
};

// the batched transforms take at most 65535 rows per call
int eval_rows(gs_ctx *c, const fe *in, uint64_t rows, uint64_t len, const fe &w, uint64_t n, fe *out) {
    uint8_t wb[sizeof(fe)];
    fe_to_bytes(wb, w);
    for (uint64_t at = 0; at < rows; at += 32768) {
        const uint32_t cnt = (uint32_t)(rows - at < 32768 ? rows - at : 32768);
        const int rc = gs_eval_polys_at_roots(c, in + at * len, cnt, len, wb, n, out + at * n);
        if (rc) return rc;
    }
    return GS_OK;
}
int interpolate_rows(gs_ctx *c, const fe *in, uint64_t rows, const fe &w, uint64_t n, fe *out) {
    uint8_t wb[sizeof(fe)];
    fe_to_bytes(wb, w);
    for (uint64_t at = 0; at < rows; at += 32768) {
        const uint32_t cnt = (uint32_t)(rows - at < 32768 ? rows - at : 32768);
        const int rc = gs_interpolate_roots(c, in + at * n, cnt, wb, n, out + at * n);
        if (rc) return rc;
    }
    return GS_OK;
}

}  // namespace

extern "C" {

uint32_t gs_boundary_schoolbook_log2(uint32_t log2_len) {
    return g_schoolbook_log2.exchange(log2_len > 12 ? 12 : (log2_len < 1 ? 1 : log2_len));
}

int gs_boundary_polys(gs_ctx *c, const gs_elt *omega_bytes, uint64_t n, uint64_t T, const uint64_t *steps_host, const uint8_t *values_host,
                      const uint32_t *per_row, uint32_t rows, uint32_t width, void *i_out, void *z_out) {
    if (!c || !omega_bytes || !steps_host || !values_host || !per_row || !i_out || !z_out) return GS_ERR_ARG;
    if (!rows || !width || !gs_is_pow2(T) || !gs_is_pow2(n) || n < 2 * T || width > T || T > (1ull << 28))
        return gs_fail(c, GS_ERR_ARG, "boundary_polys: rows, width >= 1, width <= steps, steps and n powers of two, n >= 2 steps");
    {
        std::vector<bool> seen(T, false);                        // one bitmap, cleared by walking the row's steps again
        for (uint32_t r = 0; r < rows; r++) {
            if (!per_row[r] || per_row[r] > width) return gs_fail(c, GS_ERR_ARG, "boundary_polys: row %u has %u assertions (1 .. %u)", r, per_row[r], width);
            if (r)
                for (uint32_t i = 0; i < per_row[r - 1]; i++) seen[steps_host[(uint64_t)(r - 1) * width + i]] = false;
            for (uint32_t i = 0; i < per_row[r]; i++) {
                const uint64_t s = steps_host[(uint64_t)r * width + i];
                if (s >= T) return gs_fail(c, GS_ERR_ARG, "boundary_polys: step %llu is outside of the %llu steps", (unsigned long long)s, (unsigned long long)T);
                if (seen[s]) return gs_fail(c, GS_ERR_ARG, "boundary_polys: step %llu is asserted twice on row %u", (unsigned long long)s, r);
                seen[s] = true;
            }
        }
    }
    const fe omega = fe_from_bytes(omega_bytes);
    const fe g = fe_pow_u64(omega, n / T), ginv = fe_pow_u64(g, T - 1), w2t = fe_pow_u64(omega, n / (2 * T));
    uint64_t W = 1;
    while (W < width) W <<= 1;
    const uint64_t cells = (uint64_t)rows * width, tree = (uint64_t)rows * W * 2;

    Blocks blocks(c);
    void *p;
    int rc;
    uint64_t *d_steps; uint32_t *d_per_row; fe *d_values, *lvl[2], *ev = nullptr, *pr = nullptr;
    if ((rc = blocks.get(cells * 8, &p))) return rc;
    d_steps = (uint64_t *)p;
    if ((rc = blocks.get(rows * 4ull, &p))) return rc;
    d_per_row = (uint32_t *)p;
    if ((rc = blocks.get(cells * GS_ELT, &p))) return rc;
    d_values = (fe *)p;
    for (int k = 0; k < 2; k++) { if ((rc = blocks.get(tree * GS_ELT, &p))) return rc; lvl[k] = (fe *)p; }
    if ((rc = gs_push(c, d_steps, steps_host, cells * 8))) return rc;
    if ((rc = gs_push(c, d_per_row, per_row, rows * 4ull))) return rc;
    if ((rc = gs_push(c, d_values, values_host, cells * GS_ELT))) return rc;

    // ---- Z_r: the product tree
    hipLaunchKernelGGL(k_bd_leaves, dim3(gs_grid((uint64_t)rows * W)), dim3(256), 0, c->stream, d_steps, d_per_row, rows, width, W, g, lvl[0]);
    GS_LAUNCH_CHECK(c);
    int cur = 0;
    for (uint64_t slot = 2; slot < 2 * W; slot *= 2) {             // nodes of `slot` elements -> their pair products in 2 * slot
        const uint64_t nodes = tree / slot;
        if (slot <= (1ull << g_schoolbook_log2.load())) {
            gs_traffic(c, 2 * tree * GS_ELT, tree * (slot / 2 + 1), "k_bd_pair_schoolbook");
            hipLaunchKernelGGL(k_bd_pair_schoolbook, dim3(gs_grid(tree)), dim3(256), 0, c->stream, lvl[cur], tree, (uint32_t)slot, lvl[cur ^ 1]);
            GS_LAUNCH_CHECK(c);
        } else {
            const uint64_t pn = 2 * slot;                           // points: the product has at most slot + 1 coefficients
            if (!ev) {
                if ((rc = blocks.get(2 * tree * GS_ELT, &p))) return rc;
                ev = (fe *)p;
                if ((rc = blocks.get(tree * GS_ELT, &p))) return rc;
                pr = (fe *)p;
            }
            const fe wn = fe_pow_u64(omega, n / pn);
            if ((rc = eval_rows(c, lvl[cur], nodes, slot, wn, pn, ev))) return rc;
            hipLaunchKernelGGL(k_bd_pair_pointwise, dim3(gs_grid(tree)), dim3(256), 0, c->stream, ev, tree, pn, pr);
            GS_LAUNCH_CHECK(c);
            if ((rc = interpolate_rows(c, pr, nodes / 2, wn, pn, lvl[cur ^ 1]))) return rc;
        }
        cur ^= 1;
    }
    const fe *z = lvl[cur];                                         // rows x 2W
    fe *spare = lvl[cur ^ 1];                                       // rows x 2W: Z' (rows x W), then the weights (rows x width <= rows x W)

    // ---- c_i = y_i / Z_r'(x_i)
    fe *x1, *x2;
    if ((rc = blocks.get((uint64_t)rows * T * GS_ELT, &p))) return rc;
    x1 = (fe *)p;
    if ((rc = blocks.get((uint64_t)rows * T * GS_ELT, &p))) return rc;
    x2 = (fe *)p;
    hipLaunchKernelGGL(k_bd_derivative, dim3(gs_grid((uint64_t)rows * W)), dim3(256), 0, c->stream, z, rows, W, spare);
    GS_LAUNCH_CHECK(c);
    if ((rc = eval_rows(c, spare, rows, W, g, T, x1))) return rc;
    fe *den = spare, *cw = spare + (uint64_t)rows * W;
    hipLaunchKernelGGL(k_bd_gather, dim3(gs_grid(cells)), dim3(256), 0, c->stream, x1, d_steps, d_per_row, rows, width, T, den);
    GS_LAUNCH_CHECK(c);
    if ((rc = gs_vec_div(c, d_values, den, cells, cw))) return rc;

    // ---- W: the transform of the sparse weight vector, one place on
    GS_HIP(c, hipMemsetAsync(x1, 0, (uint64_t)rows * T * GS_ELT, c->stream));
    hipLaunchKernelGGL(k_bd_scatter, dim3(gs_grid(cells)), dim3(256), 0, c->stream, cw, d_steps, d_per_row, rows, width, T, x1);
    GS_LAUNCH_CHECK(c);
    if ((rc = eval_rows(c, x1, rows, T, ginv, T, x2))) return rc;
    hipLaunchKernelGGL(k_bd_shift, dim3(gs_grid((uint64_t)rows * T)), dim3(256), 0, c->stream, x2, rows, T, x1);
    GS_LAUNCH_CHECK(c);

    // ---- I_r = (Z_r W) div x^T
    fe *ez, *ew;
    if ((rc = blocks.get((uint64_t)rows * 2 * T * GS_ELT, &p))) return rc;
    ez = (fe *)p;
    if ((rc = blocks.get((uint64_t)rows * 2 * T * GS_ELT, &p))) return rc;
    ew = (fe *)p;
    if ((rc = eval_rows(c, z, rows, 2 * W, w2t, 2 * T, ez))) return rc;
    if ((rc = eval_rows(c, x1, rows, T, w2t, 2 * T, ew))) return rc;
    if ((rc = gs_vec_mul(c, ez, ew, (uint64_t)rows * 2 * T, ez))) return rc;
    if ((rc = interpolate_rows(c, ez, rows, w2t, 2 * T, ew))) return rc;
    hipLaunchKernelGGL(k_bd_take, dim3(gs_grid((uint64_t)rows * (width + 1ull))), dim3(256), 0, c->stream, ew, z, d_per_row, rows, width, T, W, (fe *)i_out,
                       (fe *)z_out);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

uint32_t gs_eval_polys_at_points_segment(void) { return GS_EP_SEGMENT; }

int gs_eval_polys_at_points(gs_ctx *c, const void *polys, uint32_t rows, uint64_t stride, const uint64_t *lens_host, const uint8_t *points_host, uint32_t npoints,
                            void *out) {
    if (!c || !lens_host || (npoints && !points_host) || ((uint64_t)rows * npoints && !out)) return GS_ERR_ARG;
    if (!rows || !npoints) return GS_OK;
    if (rows > 65535) return gs_fail(c, GS_ERR_ARG, "eval_polys_at_points: at most 65535 rows per call");
    if (stride > (1ull << 40) || (rows > 1 && !stride)) return gs_fail(c, GS_ERR_ARG, "eval_polys_at_points: rows of 1 .. 2^40 elements");
    uint64_t longest = 0;
    for (uint32_t r = 0; r < rows; r++) {
        if (lens_host[r] > stride) return gs_fail(c, GS_ERR_ARG, "eval_polys_at_points: row %u has %llu coefficients, the rows are %llu apart", r,
                                                  (unsigned long long)lens_host[r], (unsigned long long)stride);
        if (lens_host[r] > longest) longest = lens_host[r];
    }
    if (longest && !polys) return GS_ERR_ARG;
    const uint64_t nseg = (longest + GS_EP_SEGMENT - 1) / GS_EP_SEGMENT, pblocks = ((uint64_t)npoints + GS_EP_POINTS - 1) / GS_EP_POINTS;
    if (pblocks > 65535) return gs_fail(c, GS_ERR_ARG, "eval_polys_at_points: at most %u points per call", 65535u * GS_EP_POINTS);
    Blocks blocks(c);
    void *p;
    int rc;
    if ((rc = blocks.get(rows * 8ull, &p))) return rc;
    uint64_t *d_lens = (uint64_t *)p;
    if ((rc = blocks.get((uint64_t)npoints * GS_ELT, &p))) return rc;
    fe *d_points = (fe *)p;
    if ((rc = blocks.get((uint64_t)rows * nseg * npoints * GS_ELT, &p))) return rc;
    fe *partial = (fe *)p;
    if ((rc = gs_push(c, d_lens, lens_host, rows * 8ull))) return rc;
    if ((rc = gs_push(c, d_points, points_host, (uint64_t)npoints * GS_ELT))) return rc;
    if (nseg) {
        uint64_t coefficients = 0;
        for (uint32_t r = 0; r < rows; r++) coefficients += lens_host[r];
        gs_traffic(c, (coefficients * pblocks + (uint64_t)rows * nseg * npoints) * GS_ELT, coefficients * npoints, "k_eval_points_partial");
        hipLaunchKernelGGL(k_eval_points_partial, dim3((unsigned)nseg, (unsigned)pblocks, rows), dim3(256), 0, c->stream, (const fe *)polys, stride, d_lens, d_points,
                           npoints, (uint32_t)nseg, partial);
        GS_LAUNCH_CHECK(c);
    }
    hipLaunchKernelGGL(k_eval_points_combine, dim3(gs_grid((uint64_t)rows * npoints)), dim3(256), 0, c->stream, partial, d_lens, d_points, rows, npoints,
                       (uint32_t)nseg, (fe *)out);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

}  // extern "C"
