// scan.hip — running sums, running products and the linear recurrence x[i] = a[i]*x[i-1] + b[i] over device vectors
// (include/gstark_scan.h), in one vector, in uniform segments (the rows of a matrix) or in flagged segments.  Nothing but the
// flavour-neutral fe_* API.  The schedule is the host plan's (scan_plan.h): reduce-then-scan in at most three launches; a launch
// boundary is the only synchronisation between workgroups (no look-back, no spinning, no grid barrier).
//   operator    a scan element is (head flag, payload); (f1, x1) (+) (f2, x2) = (f1 | f2, f2 ? x2 : x1 o x2).  The payload is an element
//               for the sum and the product, and the pair (A, B) of the map x -> A*x + B for the recurrence, whose composition
//               (A2*A1, A2*B1 + B2) is NOT commutative: thread, lane, wave and tile order is the element order throughout.
//   flags       never stored next to the data: every kernel derives the flag of element i from its index (i % cols == 0; one vector
//               is the one row of cols = n elements) or-ed with the low bit of heads[i] where the caller gave heads.  ONE code path.
//   layout      each thread owns the SCAN_E consecutive elements that fill 64 bytes and loads them with 16-byte loads; a wave's
//               loads cover 4 KiB of consecutive addresses, every fetched line is used whole by the one wave that fetched it, and no
//               data element passes through LDS (DESIGN.md 3.19 has the argument).  LDS holds the waves' aggregates alone.
//   k_scan_tiles    one tile per workgroup: each thread folds its elements, the lanes combine with fe_shfl_up, the waves through
//                   LDS; the last thread writes the tile's (flag, payload).
//   k_scan_totals   ONE workgroup: the exclusive scan of the tile aggregates, in place (payloads only: a carry's flag is never
//                   read); the reduction of one row takes its total from here and stops.
//   k_scan_apply    the tile scan again with the carry of its tile; writes the inclusive or exclusive values (the recurrence:
//                   A*x0 + B) and the rows' totals.  An input of at most one tile takes this launch alone, with no carry.
#include "common.h"
#include "fe_shfl.h"
#include "scan_plan.h"
#include "../../include/gstark_scan.h"

#define SCAN_E ((int)(SCAN_LANE_BYTES / sizeof(fe)))

struct ScanPair { fe A, B; };                  // x -> A*x + B

// c ? a : b limb by limb (a conditional between two objects would pick an ADDRESS and keep both in memory)
__device__ __forceinline__ fe scan_pick(bool c, const fe &a, const fe &b) {
    fe o;
#pragma unroll
    for (int l = 0; l < GF_LIMBS; l++) fe_set_limb(o, l, c ? fe_limb(a, l) : fe_limb(b, l));
    return o;
}

template <int OP> struct ScanOp;
template <> struct ScanOp<SCAN_OP_SUM> {
    typedef fe T;
    static constexpr int PRODUCTS = 0;
    static __device__ __forceinline__ T identity() { return fe_zero(); }
    static __device__ __forceinline__ T comb(const T &l, const T &r) { return fe_add(l, r); }
    static __device__ __forceinline__ T shfl_up(const T &v, int d) { return fe_shfl_up(v, d); }
    static __device__ __forceinline__ T pick(bool c, const T &a, const T &b) { return scan_pick(c, a, b); }
    static __device__ __forceinline__ T load(const fe *v, const fe *, const fe &, uint32_t i) { return v[i]; }
    static __device__ __forceinline__ fe value(const T &v, const fe &, bool) { return v; }
};
template <> struct ScanOp<SCAN_OP_PRODUCT> {
    typedef fe T;
    static constexpr int PRODUCTS = 1;
    static __device__ __forceinline__ T identity() { return fe_one(); }
    static __device__ __forceinline__ T comb(const T &l, const T &r) { return fe_mul(l, r); }
    static __device__ __forceinline__ T shfl_up(const T &v, int d) { return fe_shfl_up(v, d); }
    static __device__ __forceinline__ T pick(bool c, const T &a, const T &b) { return scan_pick(c, a, b); }
    static __device__ __forceinline__ T load(const fe *v, const fe *, const fe &, uint32_t i) { return v[i]; }
    static __device__ __forceinline__ fe value(const T &v, const fe &, bool) { return v; }
};
template <> struct ScanOp<SCAN_OP_AFFINE> {
    typedef ScanPair T;
    static constexpr int PRODUCTS = 2;
    static __device__ __forceinline__ T identity() { return T{fe_one(), fe_zero()}; }
    // first l, then r: x -> r.A * (l.A * x + l.B) + r.B
    static __device__ __forceinline__ T comb(const T &l, const T &r) { return T{fe_mul(r.A, l.A), fe_add(fe_mul(r.A, l.B), r.B)}; }
    static __device__ __forceinline__ T shfl_up(const T &v, int d) { return T{fe_shfl_up(v.A, d), fe_shfl_up(v.B, d)}; }
    static __device__ __forceinline__ T pick(bool c, const T &a, const T &b) { return T{scan_pick(c, a.A, b.A), scan_pick(c, a.B, b.B)}; }
    static __device__ __forceinline__ T load(const fe *b, const fe *a, const fe &a_scalar, uint32_t i) {
        if (a) return T{a[i], b[i]};                                         // (uniform)
        return T{a_scalar, b[i]};
    }
    static __device__ __forceinline__ fe value(const T &v, const fe &x0, bool x0_is_zero) {
        if (x0_is_zero) return v.B;                                          // (uniform)
        return fe_add(fe_mul(v.A, x0), v.B);
    }
};

// what every kernel reads of a call.  v: the values (the recurrence: b); a: the recurrence's factors, or null for a_scalar
struct ScanIn {
    const fe *v, *a;
    fe a_scalar;
    const uint8_t *heads;                      // or null
    uint32_t n, cols;                          // one vector and flagged segments: cols == n
};

template <class Op>
__device__ __forceinline__ void scan_comb(bool lf, const typename Op::T &lx, bool rf, const typename Op::T &rx, bool &of, typename Op::T &ox) {
    const typename Op::T both = Op::comb(lx, rx);
    ox = Op::pick(rf, rx, both);
    of = lf | rf;
}

// The elements of one thread, in element order, from index i0: values and head flags (past the end: identities without a flag), and
// their fold (f, x).  *r0 = i0 % cols and *row0 = i0 / cols.
template <class Op>
__device__ __forceinline__ void scan_load(const ScanIn &in, uint32_t i0, typename Op::T (&v)[SCAN_E], bool (&h)[SCAN_E], bool &f, typename Op::T &x, uint32_t *r0,
                                          uint32_t *row0) {
    const uint32_t row = i0 / in.cols;
    uint32_t r = i0 - row * in.cols;
    *r0 = r;
    *row0 = row;
#pragma unroll
    for (int e = 0; e < SCAN_E; e++) {
        const uint32_t i = i0 + (uint32_t)e;
        if (i < in.n) {
            v[e] = Op::load(in.v, in.a, in.a_scalar, i);
            h[e] = r == 0 || (in.heads && (in.heads[i] & 1u));
        } else {
            v[e] = Op::identity();
            h[e] = false;
        }
        if (++r == in.cols) r = 0;
    }
    f = h[0];
    x = v[0];
#pragma unroll
    for (int e = 1; e < SCAN_E; e++) scan_comb<Op>(f, x, h[e], v[e], f, x);
}

// The exclusive prefix (pf, px) of this thread's aggregate (f, x) among the NT threads of the workgroup, in thread order.  Every thread
// of the workgroup calls it (shuffles and a barrier).  lds_x / lds_f: NT / 64 entries.
template <class Op, int NT>
__device__ __forceinline__ void scan_block(bool f, typename Op::T x, typename Op::T *lds_x, uint32_t *lds_f, bool &pf, typename Op::T &px) {
    typedef typename Op::T T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {                                       // inclusive over the lanes
        const bool uf = __shfl_up((int)f, d) != 0;
        const T ux = Op::shfl_up(x, d);
        if (lane >= d) scan_comb<Op>(uf, ux, f, x, f, x);
    }
    if (lane == 63) { lds_x[wave] = x; lds_f[wave] = f ? 1u : 0u; }
    __syncthreads();
    bool wf = false;
    T wx = Op::identity();
#pragma unroll 1
    for (int w = 0; w < wave; w++) scan_comb<Op>(wf, wx, lds_f[w] != 0, lds_x[w], wf, wx);      // (the trip count is the wave's own: uniform)
    bool ef = __shfl_up((int)f, 1) != 0;
    T ex = Op::shfl_up(x, 1);
    if (lane == 0) { ef = false; ex = Op::identity(); }
    scan_comb<Op>(wf, wx, ef, ex, pf, px);
}

template <int OP>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_tiles(const ScanIn in, typename ScanOp<OP>::T *agg_x, uint32_t *agg_f) {
    typedef ScanOp<OP> Op;
    typedef typename Op::T T;
    __shared__ T lds_x[SCAN_BLOCK / 64];
    __shared__ uint32_t lds_f[SCAN_BLOCK / 64];
    T v[SCAN_E], x, px;
    bool h[SCAN_E], f, pf;
    uint32_t r, row;
    scan_load<Op>(in, (blockIdx.x * SCAN_BLOCK + threadIdx.x) * (uint32_t)SCAN_E, v, h, f, x, &r, &row);
    scan_block<Op, SCAN_BLOCK>(f, x, lds_x, lds_f, pf, px);
    if (threadIdx.x == SCAN_BLOCK - 1) {
        scan_comb<Op>(pf, px, f, x, f, x);
        agg_x[blockIdx.x] = x;
        agg_f[blockIdx.x] = f ? 1u : 0u;
    }
}

// agg_x[t] becomes the combination of the aggregates of the tiles before t (tile 0: the identity); thread k owns the `per` consecutive
// aggregates from k * per.  total (or null): the value of all the tiles together (the sum and the product).
template <int OP>
__global__ __launch_bounds__(SCAN_TOTALS_BLOCK) void k_scan_totals(typename ScanOp<OP>::T *agg_x, const uint32_t *agg_f, uint32_t tiles, uint32_t per, fe *total) {
    typedef ScanOp<OP> Op;
    typedef typename Op::T T;
    __shared__ T lds_x[SCAN_TOTALS_BLOCK / 64];
    __shared__ uint32_t lds_f[SCAN_TOTALS_BLOCK / 64];
    const uint32_t first = threadIdx.x * per;
    bool f = false, pf;
    T x = Op::identity(), px;
#pragma unroll 1
    for (uint32_t k = first; k < first + per && k < tiles; k++) scan_comb<Op>(f, x, agg_f[k] != 0, agg_x[k], f, x);
    scan_block<Op, SCAN_TOTALS_BLOCK>(f, x, lds_x, lds_f, pf, px);
#pragma unroll 1
    for (uint32_t k = first; k < first + per && k < tiles; k++) {
        const T own = agg_x[k];
        agg_x[k] = px;
        scan_comb<Op>(pf, px, agg_f[k] != 0, own, pf, px);
        if (total && k == tiles - 1) *total = Op::value(px, fe_zero(), true);
    }
}

// values / out are NOT restrict: out may be the input (each thread reads its own elements before it writes them)
template <int OP>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_apply(const ScanIn in, const typename ScanOp<OP>::T *carry, int exclusive, const fe x0, int x0_is_zero, fe *out,
                                                         fe *totals) {
    typedef ScanOp<OP> Op;
    typedef typename Op::T T;
    __shared__ T lds_x[SCAN_BLOCK / 64];
    __shared__ uint32_t lds_f[SCAN_BLOCK / 64];
    T v[SCAN_E], x, cur;
    bool h[SCAN_E], f, pf;
    uint32_t r, row;
    const uint32_t i0 = (blockIdx.x * SCAN_BLOCK + threadIdx.x) * (uint32_t)SCAN_E;
    scan_load<Op>(in, i0, v, h, f, x, &r, &row);
    scan_block<Op, SCAN_BLOCK>(f, x, lds_x, lds_f, pf, cur);
    if (carry) scan_comb<Op>(false, carry[blockIdx.x], pf, cur, pf, cur);   // (uniform)
#pragma unroll
    for (int e = 0; e < SCAN_E; e++) {
        const uint32_t i = i0 + (uint32_t)e;
        const T before = Op::pick(h[e], Op::identity(), cur);
        cur = Op::comb(before, v[e]);
        if (i < in.n) {
            if (out) out[i] = Op::value(Op::pick(exclusive != 0, before, cur), x0, x0_is_zero != 0);
            if (totals && r + 1 == in.cols) totals[row] = Op::value(cur, x0, x0_is_zero != 0);
        }
        if (++r == in.cols) { r = 0; row++; }
    }
}

namespace {

int scan_element(gs_ctx *c, const char *who, const char *name, const gs_elt *v, fe *out) {
    *out = fe_from_bytes(v);
    return fe_ge_p(*out) ? gs_fail(c, GS_ERR_ARG, "%s: %s is not a canonical element", who, name) : GS_OK;
}

struct ScanCall {
    const char *who;
    int op, exclusive;
    const fe *v, *a;                           // v: values, or b
    fe a_scalar, x0;
    bool x0_is_zero;
    const uint8_t *heads;
    uint64_t rows, cols;
    fe *out, *totals;
};

template <int OP>
int scan_launch(gs_ctx *c, const ScanCall &k, const scan_plan &pl) {
    typedef typename ScanOp<OP>::T T;
    const uint64_t n = pl.n, es = GS_ELT;
    const uint64_t m = ScanOp<OP>::PRODUCTS;
    const char *name = OP == SCAN_OP_SUM ? "sum" : OP == SCAN_OP_PRODUCT ? "product" : "affine";
    ScanIn in;
    in.v = k.v; in.a = k.a; in.a_scalar = k.a_scalar; in.heads = k.heads;
    in.n = (uint32_t)n;
    in.cols = (uint32_t)(k.heads ? n : k.cols);
    const uint64_t in_bytes = n * (es * (k.a ? 2 : 1) + (k.heads ? 1 : 0)), threads = (uint64_t)pl.tiles * SCAN_BLOCK;
    // products a lane issues: its fold, six steps over the lanes (kept or not), the prefix of its wave and lane; the apply kernel also
    // walks its elements again (and evaluates A*x0 + B)
    const uint64_t fold = threads * (SCAN_E - 1 + 6 + 2) * m;
    const uint64_t apply = fold + threads * (1 + SCAN_E) * m + (OP == SCAN_OP_AFFINE && !k.x0_is_zero ? n : 0);
    const uint64_t out_bytes = (k.out ? n * es : 0) + (k.totals ? k.rows * es : 0);
    if (pl.launches == 1) {
        gs_traffic(c, in_bytes + out_bytes, apply, "k_scan_apply<%s>", name);
        hipLaunchKernelGGL(k_scan_apply<OP>, dim3(1), dim3(SCAN_BLOCK), 0, c->stream, in, (const T *)nullptr, k.exclusive, k.x0, k.x0_is_zero ? 1 : 0, k.out, k.totals);
        GS_LAUNCH_CHECK(c);
        return GS_OK;
    }
    void *tmp = nullptr;
    int rc = gs_tmp_alloc(c, pl.aggregate_bytes, &tmp);
    if (rc) return rc;
    T *agg_x = (T *)tmp;
    uint32_t *agg_f = (uint32_t *)((uint8_t *)tmp + (uint64_t)pl.tiles * sizeof(T));
    gs_traffic(c, in_bytes + pl.tiles * (sizeof(T) + 4), fold, "k_scan_tiles<%s>", name);
    hipLaunchKernelGGL(k_scan_tiles<OP>, dim3(pl.grid[0]), dim3(SCAN_BLOCK), 0, c->stream, in, agg_x, agg_f);
    gs_traffic(c, pl.tiles * (2 * sizeof(T) + 8), (2ull * pl.tiles + SCAN_TOTALS_BLOCK * 8ull) * m, "k_scan_totals<%s>", name);
    hipLaunchKernelGGL(k_scan_totals<OP>, dim3(1), dim3(SCAN_TOTALS_BLOCK), 0, c->stream, agg_x, (const uint32_t *)agg_f, pl.tiles, pl.aggregates_per_thread,
                       pl.launches == 2 ? k.totals : (fe *)nullptr);
    if (pl.launches == 3) {
        gs_traffic(c, in_bytes + pl.tiles * sizeof(T) + out_bytes, apply, "k_scan_apply<%s>", name);
        hipLaunchKernelGGL(k_scan_apply<OP>, dim3(pl.grid[2]), dim3(SCAN_BLOCK), 0, c->stream, in, (const T *)agg_x, k.exclusive, k.x0, k.x0_is_zero ? 1 : 0, k.out, k.totals);
    }
    gs_tmp_free(c, tmp);                        // (parked for reuse by work that is ordered on the same stream)
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int scan_run(gs_ctx *c, const ScanCall &k) {
    uint64_t n;
    if (const char *why = scan_count(k.rows, k.cols, &n)) return gs_fail(c, GS_ERR_ARG, "%s: %s (rows %llu, cols %llu)", k.who, why, (unsigned long long)k.rows, (unsigned long long)k.cols);
    if (!n) return GS_OK;
    if (!k.v || (!k.out && !k.totals)) return gs_fail(c, GS_ERR_ARG, "%s: the input and the output are required", k.who);
    if (k.heads && k.rows != 1) return gs_fail(c, GS_ERR_ARG, "%s: heads go with rows == 1, not %llu rows", k.who, (unsigned long long)k.rows);
    if (k.heads && k.totals) return gs_fail(c, GS_ERR_ARG, "%s: totals_out goes with uniform segments, not with heads", k.who);
    const uint64_t es = GS_ELT;
    const scan_range in_place = {(uint64_t)(uintptr_t)k.v, n * es}, a = {(uint64_t)(uintptr_t)k.a, n * es}, heads = {(uint64_t)(uintptr_t)k.heads, n};
    const scan_range out = {(uint64_t)(uintptr_t)k.out, n * es}, totals = {(uint64_t)(uintptr_t)k.totals, k.rows * es};
    if (const char *why = scan_check_alias(in_place, a, heads, out, totals)) return gs_fail(c, GS_ERR_ARG, "%s: %s", k.who, why);
    scan_plan pl;
    if (const char *why = scan_plan_build((uint32_t)es, k.op == SCAN_OP_AFFINE ? 2 : 1, n, !k.out && k.rows == 1, pl)) return gs_fail(c, GS_ERR_ARG, "%s: %s", k.who, why);
    if (k.op == SCAN_OP_SUM) return scan_launch<SCAN_OP_SUM>(c, k, pl);
    if (k.op == SCAN_OP_PRODUCT) return scan_launch<SCAN_OP_PRODUCT>(c, k, pl);
    return scan_launch<SCAN_OP_AFFINE>(c, k, pl);
}

}  // namespace

extern "C" {

int gs_scan(gs_ctx *c, int op, int exclusive, const void *values, const void *heads, uint64_t rows, uint64_t cols, void *out, void *totals_out) {
    if (!c) return GS_ERR_ARG;
    if (op != GS_SCAN_SUM && op != GS_SCAN_PRODUCT) return gs_fail(c, GS_ERR_ARG, "scan: op is GS_SCAN_SUM or GS_SCAN_PRODUCT, not %d", op);
    ScanCall k = {"scan", op == GS_SCAN_SUM ? SCAN_OP_SUM : SCAN_OP_PRODUCT, exclusive ? 1 : 0, (const fe *)values, nullptr, fe_zero(), fe_zero(), true, (const uint8_t *)heads,
                  rows, cols, (fe *)out, (fe *)totals_out};
    if (rows && cols && !out) return gs_fail(c, GS_ERR_ARG, "scan: out is required");
    return scan_run(c, k);
}

int gs_scan_affine(gs_ctx *c, int exclusive, const void *a, const gs_elt *a_scalar_host, const void *b, const gs_elt *x0_host, const void *heads, uint64_t rows,
                   uint64_t cols, void *out) {
    if (!c) return GS_ERR_ARG;
    ScanCall k = {"scan_affine", SCAN_OP_AFFINE, exclusive ? 1 : 0, (const fe *)b, (const fe *)a, fe_zero(), fe_zero(), true, (const uint8_t *)heads, rows, cols, (fe *)out, nullptr};
    int rc;
    if (x0_host) {
        if ((rc = scan_element(c, k.who, "x0", x0_host, &k.x0))) return rc;
        k.x0_is_zero = fe_is_zero(k.x0);
    }
    if (!a && a_scalar_host && (rc = scan_element(c, k.who, "a", a_scalar_host, &k.a_scalar))) return rc;
    if (rows && cols && ((!a && !a_scalar_host) || !out)) return gs_fail(c, GS_ERR_ARG, "scan_affine: a (or a_scalar_host) and out are required");
    return scan_run(c, k);
}

int gs_reduce(gs_ctx *c, int op, const void *values, uint64_t rows, uint64_t cols, void *totals_out) {
    if (!c) return GS_ERR_ARG;
    if (op != GS_SCAN_SUM && op != GS_SCAN_PRODUCT) return gs_fail(c, GS_ERR_ARG, "reduce: op is GS_SCAN_SUM or GS_SCAN_PRODUCT, not %d", op);
    ScanCall k = {"reduce", op == GS_SCAN_SUM ? SCAN_OP_SUM : SCAN_OP_PRODUCT, 0, (const fe *)values, nullptr, fe_zero(), fe_zero(), true, nullptr, rows, cols, nullptr,
                  (fe *)totals_out};
    return scan_run(c, k);
}

int gs_scan_plan(gs_ctx *c, uint64_t n, uint32_t *tile_elements, uint32_t *elements_per_thread, uint64_t *max_elements, uint32_t *launches) {
    if (!c) return GS_ERR_ARG;
    scan_plan pl;
    const char *why = scan_plan_build((uint32_t)GS_ELT, 1, n, false, pl);
    if (tile_elements) *tile_elements = scan_tile((uint32_t)GS_ELT);
    if (elements_per_thread) *elements_per_thread = scan_per_thread((uint32_t)GS_ELT);
    if (max_elements) *max_elements = SCAN_MAX_ELEMENTS;
    if (launches) *launches = why ? 0 : pl.launches;
    return GS_OK;
}

}  // extern "C"
