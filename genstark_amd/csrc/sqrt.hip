// sqrt.hip — square roots in the library's field, Euler's criterion on whole columns, and the lift of x coordinates to points of
// y^2 = x^3 + a*x + b with its inverse, the split into x and a parity byte (include/gstark_sqrt.h).  One thread takes one root; nothing
// but the flavour-neutral fe_* API, no LDS, nothing crosses lanes.  The schedule is the host plan's (sqrt_plan.h) and depends on the
// modulus alone: every loop below runs a trip count that is the same in every lane and in every call, and a digit of the discrete
// logarithm picks a table entry by its index, never a branch.
//   exponent    w0 = a^((t-1)/2) by the plan's sliding-window schedule (read at lane-independent indexes: scalar loads), then x = a * w0
//               and b = x * w0 = a^t = g^e.
//   logarithm   window by window from the low end (sqrt_plan.h).  CHAIN form: the powers b^(2^(s - lo_{j+1})) are computed once and stay in
//               registers (`windows` elements per lane; the window loop is unrolled so that they are indexed statically, its inner loop
//               over the lower digits is not).  WINDOW form: one running correction, every window squares anew; any number of windows in
//               three elements of state.  Which flavour runs which: sqrt_form() below and DESIGN.md.
//   digit       the two low limbs of an element of the subgroup of order 2^w, hashed, pick a bucket of four entries (ONE 16-byte load);
//               the tag that matches carries the digit.  The index is lane-dependent, unlike the Hades constants: a gather through L2.
//   tables      g^(-d * 2^k) rows, gathered at lane-dependent indexes from global memory: 96 KiB in the 224-bit field, which stays in L2.
//   output      flag = (a == 0 or e even); of r and p - r the even one; a non-residue gives 0.
#include "common.h"
#include "curve_jac.h"                         // fe_select
#include "sqrt_plan.h"
#include "../../include/gstark_sqrt.h"

#define GS_SQRT_BLOCK 64                       // one wave, as k_curve_mul: a batch of 2^12 roots spreads over 64 compute units

// what the kernels read of the plan: everything in ONE device block (table | hash buckets | row offsets | the two schedules)
struct SqrtDev {
    const fe *table;
    const uint4 *hash;
    const uint32_t *off;                       // [0, 32): T rows, [32, 65): U rows by k
    const uint32_t *root_pow, *euler_pow;      // steps: squarings | product << 16
    uint32_t root_steps, euler_steps;
    uint32_t s, w, windows, last_w, m0, m1;
};

// x^e by the plan's schedule: x, x^3, x^5, x^7 in registers, picked by a lane-independent index
__device__ __forceinline__ fe sqrt_pow(const fe &a, const uint32_t *__restrict__ sched, uint32_t steps) {
    if (!steps) return fe_one();
    const fe a2 = fe_sqr(a), a3 = fe_mul(a2, a), a5 = fe_mul(a3, a2), a7 = fe_mul(a5, a2);
    fe acc = fe_one();
#pragma unroll 1
    for (uint32_t k = 0; k < steps; k++) {
        const uint32_t step = sched[k], nsq = step & 0xffffu, m = step >> 16;
#pragma unroll 1
        for (uint32_t q = 0; q < nsq; q++) acc = fe_sqr(acc);
        if (m) {                                                             // (uniform)
            const fe f = fe_select(m == 1, a, fe_select(m == 3, a3, fe_select(m == 5, a5, a7)));
            acc = k ? fe_mul(acc, f) : f;
        }
    }
    return acc;
}

// the exponent of an element of the subgroup of order 2^w
__device__ __forceinline__ uint32_t sqrt_digit(const SqrtDev &d, const fe &v) {
    const uint32_t h = sqrt_hash(fe_limb(v, 0), fe_limb(v, 1), d.m0, d.m1);
    const uint4 b = d.hash[h >> (32 - d.w)];
    const uint32_t tag = (h << d.w) >> d.w, mask = (1u << d.w) - 1;
    uint32_t r = 0;
    r = (b.x != SQRT_HASH_EMPTY && (b.x >> d.w) == tag) ? (b.x & mask) : r;
    r = (b.y != SQRT_HASH_EMPTY && (b.y >> d.w) == tag) ? (b.y & mask) : r;
    r = (b.z != SQRT_HASH_EMPTY && (b.z >> d.w) == tag) ? (b.z & mask) : r;
    r = (b.w != SQRT_HASH_EMPTY && (b.w >> d.w) == tag) ? (b.w & mask) : r;
    return r;
}

// digit i of digits packed four to a word; `i` is lane-independent, the words are picked by selects (no indexed register file)
template <int NWORDS>
__device__ __forceinline__ uint32_t sqrt_digit_at(const uint32_t (&ew)[NWORDS], uint32_t i) {
    uint32_t word = ew[0];
#pragma unroll
    for (int k = 1; k < NWORDS; k++) word = (i >> 2) == (uint32_t)k ? ew[k] : word;
    return (word >> ((i & 3u) * 8)) & 0xffu;
}

// x * g^(-e/2) (any root, or garbage for a non-residue); *even = e is even
template <int NW>
__device__ __forceinline__ fe sqrt_root_chain(const SqrtDev &d, const fe &a, bool *even) {
    const fe w0 = sqrt_pow(a, d.root_pow, d.root_steps);
    const fe x = fe_mul(a, w0), b = fe_mul(x, w0);
    fe P[NW];
    P[NW - 1] = b;
#pragma unroll
    for (int j = NW - 2; j >= 0; j--) {
        fe v = P[j + 1];
        const uint32_t n = j == NW - 2 ? d.last_w : d.w;                     // the width of window j + 1
#pragma unroll 1
        for (uint32_t q = 0; q < n; q++) v = fe_sqr(v);
        P[j] = v;
    }
    constexpr int NWORDS = (NW + 3) / 4;
    uint32_t ew[NWORDS];
#pragma unroll
    for (int k = 0; k < NWORDS; k++) ew[k] = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) {
        fe v = P[j];
#pragma unroll 1
        for (int i = 0; i < j; i++) {
            const uint32_t row = j == NW - 1 ? d.off[i] : d.off[32 + j + 1 - i];
            v = fe_mul(v, d.table[row + sqrt_digit_at<NWORDS>(ew, (uint32_t)i)]);
        }
        uint32_t dg = sqrt_digit(d, v);
        if (j == NW - 1) dg >>= d.w - d.last_w;
        ew[j >> 2] |= dg << ((j & 3) * 8);
    }
    fe r = x;
#pragma unroll 1
    for (int m = 0; m < NW; m++) {
        const uint32_t em = sqrt_digit_at<NWORDS>(ew, (uint32_t)m);
        uint32_t f = em >> 1;
        if (m + 1 < NW) f |= (sqrt_digit_at<NWORDS>(ew, (uint32_t)m + 1) & 1u) << (d.w - 1);
        r = fe_mul(r, d.table[d.off[m] + f]);
    }
    *even = !(ew[0] & 1u);
    return r;
}

__device__ __forceinline__ fe sqrt_root_window(const SqrtDev &d, const fe &a, bool *even) {
    const fe w0 = sqrt_pow(a, d.root_pow, d.root_steps);
    const fe x = fe_mul(a, w0), b = fe_mul(x, w0);
    fe acc = fe_one(), r = x;
    uint32_t prev = 0, e0 = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < d.windows; j++) {
        const bool last = j + 1 == d.windows;
        fe v = j ? fe_mul(b, acc) : b;
        const uint32_t nsq = last ? 0u : d.s - (j + 1) * d.w;
#pragma unroll 1
        for (uint32_t q = 0; q < nsq; q++) v = fe_sqr(v);
        uint32_t dg = sqrt_digit(d, v);
        if (last) dg >>= d.w - d.last_w;
        if (!last) {
            const fe tj = d.table[d.off[j] + dg];
            acc = j ? fe_mul(acc, tj) : tj;
        }
        if (j) r = fe_mul(r, d.table[d.off[j - 1] + ((prev >> 1) | ((dg & 1u) << (d.w - 1)))]);
        else e0 = dg;
        prev = dg;
    }
    r = fe_mul(r, d.table[d.off[d.windows - 1] + (prev >> 1)]);
    *even = !(e0 & 1u);
    return r;
}

// the even root of a, or 0; *square = a has one.  NW: windows of the chain form, 0: the window form
template <int NW>
__device__ __forceinline__ fe sqrt_even_root(const SqrtDev &d, const fe &a, bool *square) {
    bool even;
    fe r;
    if constexpr (NW > 0) r = sqrt_root_chain<NW>(d, a, &even);
    else r = sqrt_root_window(d, a, &even);
    const bool ok = even || fe_is_zero(a);                                   // (a = 0: x = 0, so r = 0 whatever the digits were)
    r = fe_select((fe_limb(r, 0) & 1u) != 0, fe_neg(r), r);                  // p is odd: p - r has the other parity
    *square = ok;
    return fe_select(ok, r, fe_zero());
}

template <int NW>
__global__ __launch_bounds__(GS_SQRT_BLOCK) void k_field_sqrt(const SqrtDev d, const fe *__restrict__ values, uint64_t count, fe *__restrict__ roots,
                                                              uint8_t *__restrict__ flags) {
    const uint64_t k = (uint64_t)blockIdx.x * GS_SQRT_BLOCK + threadIdx.x;
    if (k >= count) return;                                                  // (nothing below crosses lanes)
    bool square;
    roots[k] = sqrt_even_root<NW>(d, values[k], &square);
    flags[k] = square ? 1 : 0;
}

// Euler's criterion: a^((p-1)/2) is 1 for a square, -1 for a non-residue, 0 for 0
__global__ __launch_bounds__(GS_SQRT_BLOCK) void k_field_is_square(const SqrtDev d, const fe *__restrict__ values, uint64_t count, uint8_t *__restrict__ flags) {
    const uint64_t k = (uint64_t)blockIdx.x * GS_SQRT_BLOCK + threadIdx.x;
    if (k >= count) return;
    const fe a = values[k];
    flags[k] = fe_is_zero(a) || fe_eq(sqrt_pow(a, d.euler_pow, d.euler_steps), fe_one()) ? 1 : 0;
}

template <int NW>
__global__ __launch_bounds__(GS_SQRT_BLOCK) void k_curve_lift_x(const SqrtDev d, const fe a, const fe b, const fe *__restrict__ xs, const uint8_t *__restrict__ parities,
                                                                uint64_t count, fe *__restrict__ out, uint8_t *__restrict__ flags) {
    const uint64_t k = (uint64_t)blockIdx.x * GS_SQRT_BLOCK + threadIdx.x;
    if (k >= count) return;
    const fe x = xs[k];
    const fe rhs = fe_add(fe_mul(fe_add(fe_sqr(x), a), x), b);               // (x^2 + a) x + b
    bool square;
    const fe y = sqrt_even_root<NW>(d, rhs, &square);
    const bool odd = parities && (parities[k] & 1u);
    out[2 * k] = fe_select(square, x, fe_zero());
    out[2 * k + 1] = fe_select(odd, fe_neg(y), y);                           // (y = 0 stays 0; a missing point has y = 0 already)
    flags[k] = square ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_curve_compress(const fe *__restrict__ points, uint64_t count, fe *__restrict__ xs, uint8_t *__restrict__ parities) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    xs[k] = points[2 * k];
    parities[k] = (uint8_t)(fe_limb(points[2 * k + 1], 0) & 1u);
}

namespace {

struct SqrtState {
    sqrt_plan plan;
    SqrtDev dev = {};
    void *block = nullptr;
    std::vector<uint8_t> host;                 // what was uploaded (the copy is asynchronous: kept until the context goes)
    std::string refused;                       // the plan's reason, if it refused the modulus
};

// The chain form keeps `windows` elements per lane and is compiled for the window counts of the fixed builds (2: the 17-bit field,
// 4: the 32-, 64-, 128- and 256-bit fields, 12: the 224-bit field; 1: s <= 8).  The runtime-modulus build runs the window form for every
// modulus: its product is a call (gf_wide.h), and live elements across a call are saved and restored around it.
uint32_t sqrt_chain_max() {
#if defined(GF_RUNTIME_MODULUS)
    return 0;
#else
    return SQRT_CHAIN_MAX_WINDOWS;
#endif
}
bool sqrt_chain_compiled(uint32_t windows) { return windows == 1 || windows == 2 || windows == 4 || windows == 12; }

uint64_t align16(uint64_t v) { return (v + 15) & ~15ull; }

int sqrt_state(gs_ctx *c, const char *who, SqrtState **out) {
    SqrtState *st = (SqrtState *)c->sqrt_state;
    if (!st) {
        st = new SqrtState();
        c->sqrt_state = st;
        const fe pm1 = fe_neg(fe_one());                                     // p - 1 in whatever flavour this is
        uint32_t p[SQRT_LIMBS] = {0};
        for (int i = 0; i < GF_LIMBS; i++) p[i] = fe_limb(pm1, i);
        p[0] += 1;                                                           // (p - 1 is even: no carry)
        sqrt_plan &pl = st->plan;
        if (const char *why = sqrt_plan_build(p, sqrt_chain_max(), pl)) st->refused = why;
        else {
            if (pl.form == SQRT_FORM_CHAIN && !sqrt_chain_compiled(pl.windows)) { pl.form = SQRT_FORM_WINDOW; pl.products_per_root = pl.products_window; }
            // the rows, in this flavour's own host arithmetic
            fe g = fe_zero();
            for (int i = 0; i < GF_LIMBS; i++) fe_set_limb(g, i, pl.g.w[i]);
            std::vector<fe> ginv_pow(pl.s), table(pl.table_elems);          // g^(-2^k)
            ginv_pow[0] = fe_inv(g);
            for (uint32_t k = 1; k < pl.s; k++) ginv_pow[k] = fe_sqr(ginv_pow[k - 1]);
            auto fill = [&](uint32_t off, uint32_t shift, uint32_t width) {
                fe cur = fe_one();
                for (uint32_t d = 0; d < (1u << width); d++) { table[off + d] = cur; cur = fe_mul(cur, ginv_pow[shift]); }
            };
            for (uint32_t m = 0; m < pl.windows; m++) fill(pl.off_T[m], sqrt_row_shift_T(pl, m), sqrt_window_width(pl, m));
            if (pl.s % pl.w) for (uint32_t k = 2; k < pl.windows; k++) fill(pl.off_U[k], sqrt_row_shift_U(pl, k), pl.w);
            // the subgroup of order 2^w and the hash from its elements to their exponents
            fe h = g;
            for (uint32_t k = 0; k < pl.s - pl.w; k++) h = fe_sqr(h);
            std::vector<uint32_t> keys(2u << pl.w), entries((size_t)pl.hash_buckets * SQRT_BUCKET);
            fe cur = fe_one();
            for (uint32_t d = 0; d < (1u << pl.w); d++) { keys[2 * d] = fe_limb(cur, 0); keys[2 * d + 1] = fe_limb(cur, 1); cur = fe_mul(cur, h); }
            uint32_t m0 = 0, m1 = 0;
            if (!fe_eq(cur, fe_one()) || !sqrt_hash_build((const uint32_t(*)[2])keys.data(), pl.w, &m0, &m1, entries.data())) st->refused = "modulus is not prime";
            else {
                const uint64_t table_bytes = align16(pl.table_elems * GS_ELT), hash_bytes = (uint64_t)entries.size() * 4, off_bytes = align16((32 + 33) * 4);
                const uint64_t root_bytes = align16(pl.root_pow.steps * 4ull + 4), euler_bytes = align16(pl.euler_pow.steps * 4ull + 4);
                st->host.assign(table_bytes + hash_bytes + off_bytes + root_bytes + euler_bytes, 0);
                uint8_t *hp = st->host.data();
                memcpy(hp, table.data(), pl.table_elems * GS_ELT);
                memcpy(hp + table_bytes, entries.data(), hash_bytes);
                uint32_t *off = (uint32_t *)(hp + table_bytes + hash_bytes);
                for (uint32_t m = 0; m < 32; m++) off[m] = pl.off_T[m];
                for (uint32_t k = 0; k < 33; k++) off[32 + k] = pl.off_U[k];
                uint32_t *rp = (uint32_t *)(hp + table_bytes + hash_bytes + off_bytes), *ep = (uint32_t *)(hp + table_bytes + hash_bytes + off_bytes + root_bytes);
                for (uint32_t k = 0; k < pl.root_pow.steps; k++) rp[k] = pl.root_pow.sqr[k] | (uint32_t)pl.root_pow.mul[k] << 16;
                for (uint32_t k = 0; k < pl.euler_pow.steps; k++) ep[k] = pl.euler_pow.sqr[k] | (uint32_t)pl.euler_pow.mul[k] << 16;
                GS_HIP(c, hipSetDevice(c->device));
                GS_HIP(c, hipMalloc(&st->block, st->host.size()));
                GS_HIP(c, hipMemcpyAsync(st->block, hp, st->host.size(), hipMemcpyHostToDevice, c->stream));
                uint8_t *dp = (uint8_t *)st->block;
                SqrtDev &d = st->dev;
                d.table = (const fe *)dp;
                d.hash = (const uint4 *)(dp + table_bytes);
                d.off = (const uint32_t *)(dp + table_bytes + hash_bytes);
                d.root_pow = (const uint32_t *)(dp + table_bytes + hash_bytes + off_bytes);
                d.euler_pow = (const uint32_t *)(dp + table_bytes + hash_bytes + off_bytes + root_bytes);
                d.root_steps = pl.root_pow.steps; d.euler_steps = pl.euler_pow.steps;
                d.s = pl.s; d.w = pl.w; d.windows = pl.windows; d.last_w = pl.last_w; d.m0 = m0; d.m1 = m1;
            }
        }
    }
    if (!st->refused.empty()) return gs_fail(c, GS_ERR_UNSUPPORTED, "%s: %s", who, st->refused.c_str());
    if (!st->block) return gs_fail(c, GS_ERR_DEVICE, "%s: the tables of the square root were not uploaded", who);
    *out = st;
    return GS_OK;
}

int check_element(gs_ctx *c, const char *who, const char *name, const gs_elt *v, fe *out) {
    if (!v) return gs_fail(c, GS_ERR_ARG, "%s: %s is required", who, name);
    *out = fe_from_bytes(v);
    return fe_ge_p(*out) ? gs_fail(c, GS_ERR_ARG, "%s: %s is not a canonical element", who, name) : GS_OK;
}

const char *form_name(const SqrtState *st) { return st->plan.form == SQRT_FORM_CHAIN ? "chain" : "window"; }

}  // namespace

void gs_sqrt_destroy(gs_ctx *c) {
    SqrtState *st = (SqrtState *)c->sqrt_state;
    if (!st) return;
    if (st->block) hipFree(st->block);
    delete st;
    c->sqrt_state = nullptr;
}

// one launch of a kernel that is compiled per form: the chain form for the plan's window count, or the window form
#if defined(GF_RUNTIME_MODULUS)
#define GS_SQRT_LAUNCH(kernel, st, blocks, ...) hipLaunchKernelGGL(kernel<0>, dim3(blocks), dim3(GS_SQRT_BLOCK), 0, c->stream, __VA_ARGS__)
#else
#define GS_SQRT_LAUNCH(kernel, st, blocks, ...)                                                                                        \
    do {                                                                                                                                 \
        const dim3 grid_(blocks), block_(GS_SQRT_BLOCK);                                                                                 \
        if ((st)->plan.form == SQRT_FORM_WINDOW) hipLaunchKernelGGL(kernel<0>, grid_, block_, 0, c->stream, __VA_ARGS__);                \
        else if ((st)->plan.windows == 1) hipLaunchKernelGGL(kernel<1>, grid_, block_, 0, c->stream, __VA_ARGS__);                       \
        else if ((st)->plan.windows == 2) hipLaunchKernelGGL(kernel<2>, grid_, block_, 0, c->stream, __VA_ARGS__);                       \
        else if ((st)->plan.windows == 4) hipLaunchKernelGGL(kernel<4>, grid_, block_, 0, c->stream, __VA_ARGS__);                       \
        else hipLaunchKernelGGL(kernel<12>, grid_, block_, 0, c->stream, __VA_ARGS__);                                                   \
    } while (0)
#endif

extern "C" {

int gs_field_sqrt(gs_ctx *c, const void *values, uint64_t count, void *roots_out, void *flags_out) {
    if (!c) return GS_ERR_ARG;
    if (count > SQRT_MAX_COUNT) return gs_fail(c, GS_ERR_ARG, "field_sqrt: at most 2^20 elements per call, not %llu", (unsigned long long)count);
    if (!count) return GS_OK;
    if (!values || !flags_out) return gs_fail(c, GS_ERR_ARG, "field_sqrt: values and flags_out are required");
    SqrtState *st;
    int rc = sqrt_state(c, "field_sqrt", &st);
    if (rc) return rc;
    const unsigned blocks = (unsigned)((count + GS_SQRT_BLOCK - 1) / GS_SQRT_BLOCK);
    if (!roots_out) {
        gs_traffic(c, count * (GS_ELT + 1), count * st->plan.products_flag, "k_field_is_square");
        hipLaunchKernelGGL(k_field_is_square, dim3(blocks), dim3(GS_SQRT_BLOCK), 0, c->stream, st->dev, (const fe *)values, count, (uint8_t *)flags_out);
    } else {
        gs_traffic(c, count * (2 * GS_ELT + 1), count * st->plan.products_per_root, "k_field_sqrt<%s>", form_name(st));
        GS_SQRT_LAUNCH(k_field_sqrt, st, blocks, st->dev, (const fe *)values, count, (fe *)roots_out, (uint8_t *)flags_out);
    }
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int gs_curve_lift_x(gs_ctx *c, const gs_elt *a_host, const gs_elt *b_host, const void *xs, const void *parities, uint64_t count, void *points_out,
                    void *flags_out) {
    if (!c) return GS_ERR_ARG;
    fe a, b;
    int rc;
    if ((rc = check_element(c, "curve_lift_x", "a", a_host, &a)) || (rc = check_element(c, "curve_lift_x", "b", b_host, &b))) return rc;
    if (count > SQRT_MAX_COUNT) return gs_fail(c, GS_ERR_ARG, "curve_lift_x: at most 2^20 points per call, not %llu", (unsigned long long)count);
    if (!count) return GS_OK;
    if (!xs || !points_out || !flags_out) return gs_fail(c, GS_ERR_ARG, "curve_lift_x: xs, points_out and flags_out are required");
    SqrtState *st;
    if ((rc = sqrt_state(c, "curve_lift_x", &st))) return rc;
    const unsigned blocks = (unsigned)((count + GS_SQRT_BLOCK - 1) / GS_SQRT_BLOCK);
    gs_traffic(c, count * (3 * GS_ELT + 1 + (parities ? 1 : 0)), count * (st->plan.products_per_root + 2), "k_curve_lift_x<%s>", form_name(st));
    GS_SQRT_LAUNCH(k_curve_lift_x, st, blocks, st->dev, a, b, (const fe *)xs, (const uint8_t *)parities, count, (fe *)points_out, (uint8_t *)flags_out);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int gs_curve_compress(gs_ctx *c, const void *points, uint64_t count, void *xs_out, void *parities_out) {
    if (!c) return GS_ERR_ARG;
    if (count > SQRT_MAX_COUNT) return gs_fail(c, GS_ERR_ARG, "curve_compress: at most 2^20 points per call, not %llu", (unsigned long long)count);
    if (!count) return GS_OK;
    if (!points || !xs_out || !parities_out) return gs_fail(c, GS_ERR_ARG, "curve_compress: points, xs_out and parities_out are required");
    gs_traffic(c, count * (3 * GS_ELT + 1), 0, "k_curve_compress");
    hipLaunchKernelGGL(k_curve_compress, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, (const fe *)points, count, (fe *)xs_out, (uint8_t *)parities_out);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int gs_field_sqrt_plan(gs_ctx *c, uint32_t *two_adicity, uint32_t *window_bits, uint32_t *windows, uint32_t *products_per_root) {
    if (!c) return GS_ERR_ARG;
    SqrtState *st;
    int rc = sqrt_state(c, "field_sqrt_plan", &st);
    if (rc) return rc;
    if (two_adicity) *two_adicity = st->plan.s;
    if (window_bits) *window_bits = st->plan.w;
    if (windows) *windows = st->plan.windows;
    if (products_per_root) *products_per_root = st->plan.products_per_root;
    return GS_OK;
}

}  // extern "C"
