// poly.hip — long polynomials at arbitrary points (include/gstark_poly.h; the layout of every call is csrc/poly_plan.h's, the argument
// DESIGN.md 3.16).  With M(x) = prod (x - x_i) over n points, padded by dummy points x = 0 to W = 2^L so that every node of the
// subproduct tree is monic of full degree (the top node is x^(W - n) M):
//   tree          pair products level by level, every level kept: per-thread schoolbook while the nodes are short, batched transforms
//                 (gs_eval_polys_at_roots / gs_interpolate_roots, rows > 1) above;
//   series        g = 1 / f mod x^prec: POLY_SEED terms by one thread, then g <- g (2 - f g), doubling, through transforms;
//   division      rev(q) = rev(a) / rev(b) mod x^(la - lb + 1), r = a - q b from the low lb - 1 coefficients of q and b alone;
//   evaluation    the transposed form of the combination below, ONE inversion at the root: with P reduced modulo the top node,
//                 u = rev((rev(P) / rev(top)) mod x^W), then down the tree u_child[m] = (sibling * u)[half + m] — the high half of a
//                 product that fits the cyclic length of the parent's slot — until u_leaf = P(x_i);
//   interpolation M' at the points (the evaluation above), c_i = y_i / M'(x_i) with the flag for a zero, then up the tree
//                 N = N_left M_right + N_right M_left from N_leaf = c_i (0 at a dummy point); the top N is x^(W - n) times the interpolant.
// Field addition and multiplication are exact: no value depends on the route of a level, the seed length or the transform lengths.
#include <atomic>

#include "common.h"
#include "poly_plan.h"
#include "../../include/gstark_poly.h"

static std::atomic<uint32_t> g_poly_switch_log2{POLY_SWITCH_DEFAULT};

#define POLY_FOR(t, total) for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < (total); t += (uint64_t)gridDim.x * blockDim.x)

// leaves: slot 2; x - xs[i], or x at a dummy point
__global__ __launch_bounds__(256) void k_poly_leaves(const fe *__restrict__ xs, uint64_t n, uint64_t W, fe *__restrict__ nodes) {
    POLY_FOR(t, W) {
        nodes[2 * t] = t < n ? fe_neg(xs[t]) : fe_zero();
        nodes[2 * t + 1] = fe_one();
    }
}

// one level of the tree, schoolbook: `in` holds nodes of slot `slot` (slot / 2 + 1 coefficients), `out` their pair products in slots
// of 2 * slot; one thread per output coefficient
__global__ __launch_bounds__(256) void k_poly_pair_schoolbook(const fe *__restrict__ in, uint64_t total_out, uint32_t slot, fe *__restrict__ out) {
    const uint32_t oslot = 2 * slot, la = slot / 2 + 1;
    POLY_FOR(t, total_out) {
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
__global__ __launch_bounds__(256) void k_poly_pair_pointwise(const fe *__restrict__ ev, uint64_t total_out, uint64_t n, fe *__restrict__ out) {
    POLY_FOR(t, total_out) {
        const uint64_t node = t / n, k = t % n;
        out[t] = fe_mul(ev[2 * node * n + k], ev[(2 * node + 1) * n + k]);
    }
}

// down one level, schoolbook: child c of `half` elements = the high half of (its sibling's node) * (its parent's vector of 2 * half)
//   out[c][m] = sum over j <= half of sibling[j] * u[parent][half + m - j]
__global__ __launch_bounds__(256) void k_poly_down_schoolbook(const fe *__restrict__ level, const fe *__restrict__ u, uint64_t W, uint32_t half,
                                                              fe *__restrict__ out) {
    const uint64_t N = 2ull * half;
    POLY_FOR(t, W) {
        const uint64_t c = t / half, m = t % half;
        const fe *b = level + (c ^ 1) * N, *v = u + (c >> 1) * N + half + m;
        fe acc = fe_zero();
        for (uint32_t j = 0; j <= half; j++) acc = fe_add(acc, fe_mul(b[j], *(v - j)));
        out[t] = acc;
    }
}
// ... through transforms of N points: child c's product = (transform of its parent's vector) * (transform of its sibling's node)
__global__ __launch_bounds__(256) void k_poly_down_pointwise(const fe *__restrict__ eu, const fe *__restrict__ em, uint64_t total, uint64_t N,
                                                             fe *__restrict__ out) {
    POLY_FOR(t, total) {
        const uint64_t c = t / N, k = t % N;
        out[t] = fe_mul(eu[(c >> 1) * N + k], em[(c ^ 1) * N + k]);
    }
}
// ... and the high half of every product
__global__ __launch_bounds__(256) void k_poly_take_high(const fe *__restrict__ res, uint64_t W, uint64_t half, fe *__restrict__ out) {
    POLY_FOR(t, W) {
        const uint64_t c = t / half, m = t % half;
        out[t] = res[c * 2 * half + half + m];
    }
}

// up one level, schoolbook: parent p of 2 * half elements = N_left * M_right + N_right * M_left (N_* of `half` elements, M_* the nodes)
__global__ __launch_bounds__(256) void k_poly_up_schoolbook(const fe *__restrict__ level, const fe *__restrict__ nv, uint64_t W, uint32_t half,
                                                            fe *__restrict__ out) {
    const uint64_t N = 2ull * half;
    POLY_FOR(t, W) {
        const uint64_t p = t / N;
        const uint32_t k = (uint32_t)(t % N);
        const fe *ml = level + 2 * p * N, *mr = ml + N, *nl = nv + 2 * p * half, *nr = nl + half;
        const uint32_t j0 = k > half ? k - half : 0, j1 = k < half ? k : half - 1;
        fe acc = fe_zero();
        for (uint32_t j = j0; j <= j1; j++) acc = fe_add(acc, fe_add(fe_mul(nl[j], mr[k - j]), fe_mul(nr[j], ml[k - j])));
        out[t] = acc;
    }
}
// ... through transforms of N points, the two products and their sum in one pass
__global__ __launch_bounds__(256) void k_poly_up_pointwise(const fe *__restrict__ en, const fe *__restrict__ em, uint64_t W, uint64_t N,
                                                           fe *__restrict__ out) {
    POLY_FOR(t, W) {
        const uint64_t p = t / N, k = t % N, l = 2 * p * N + k, r = l + N;
        out[t] = fe_add(fe_mul(en[l], em[r]), fe_mul(en[r], em[l]));
    }
}

// reverse and truncate: out[k] = in[top - k] where that index lies in [0, len), else 0; k < count
__global__ __launch_bounds__(256) void k_poly_reverse(const fe *__restrict__ in, uint64_t len, uint64_t top, uint64_t count, fe *__restrict__ out) {
    POLY_FOR(k, count) out[k] = (k <= top && top - k < len) ? in[top - k] : fe_zero();
}
// out[k] = in[from + k] where that index lies below len, else 0; k < count
__global__ __launch_bounds__(256) void k_poly_window(const fe *__restrict__ in, uint64_t len, uint64_t from, uint64_t count, fe *__restrict__ out) {
    POLY_FOR(k, count) out[k] = from + k < len ? in[from + k] : fe_zero();
}
__global__ __launch_bounds__(256) void k_poly_fill(fe value, uint64_t count, fe *__restrict__ out) {
    POLY_FOR(k, count) out[k] = value;
}
// out[k] = a[k] - qb[k], k < count <= la
__global__ __launch_bounds__(256) void k_poly_remainder(const fe *__restrict__ a, const fe *__restrict__ qb, uint64_t count, fe *__restrict__ out) {
    POLY_FOR(k, count) out[k] = fe_sub(a[k], qb[k]);
}

// the first `seed` terms of 1 / f (f[0] != 0; f has at least `seed` elements): g[k] = -g[0] * sum over 1 <= j <= k of f[j] g[k - j].
// One thread: seed <= POLY_SEED, at most 496 products in a row
__global__ __launch_bounds__(256) void k_poly_series_seed(const fe *__restrict__ f, uint32_t seed, fe *__restrict__ g) {
    if (blockIdx.x || threadIdx.x) return;
    const fe g0 = fe_inv(f[0]);
    g[0] = g0;
    for (uint32_t k = 1; k < seed; k++) {
        fe acc = fe_zero();
        for (uint32_t j = 1; j <= k; j++) acc = fe_add(acc, fe_mul(f[j], g[k - j]));
        g[k] = fe_neg(fe_mul(g0, acc));
    }
}
// one Newton step over the transforms: eg <- eg (2 - ef eg)
__global__ __launch_bounds__(256) void k_poly_newton(const fe *__restrict__ ef, uint64_t n, fe *__restrict__ eg) {
    const fe two = fe_add(fe_one(), fe_one());
    POLY_FOR(k, n) {
        const fe g = eg[k];
        eg[k] = fe_mul(g, fe_sub(two, fe_mul(ef[k], g)));
    }
}
// (a b)[from + k], k < count, for a short operand: one thread per coefficient
__global__ __launch_bounds__(256) void k_poly_product_direct(const fe *__restrict__ a, uint64_t la, const fe *__restrict__ b, uint64_t lb, uint64_t from,
                                                             uint64_t count, fe *__restrict__ out) {
    POLY_FOR(t, count) {
        const uint64_t k = from + t;
        fe acc = fe_zero();
        if (la && lb && k <= la + lb - 2) {
            const uint64_t i0 = k >= lb ? k - lb + 1 : 0, i1 = k < la ? k : la - 1;
            for (uint64_t i = i0; i <= i1; i++) acc = fe_add(acc, fe_mul(a[i], b[k - i]));
        }
        out[t] = acc;
    }
}

// M' from the top node x^pads M: out[k] = (k + 1) M[k + 1], k < n, zero up to W
__global__ __launch_bounds__(256) void k_poly_derivative(const fe *__restrict__ top, uint64_t pads, uint64_t n, uint64_t W, fe *__restrict__ out) {
    POLY_FOR(k, W) out[k] = k < n ? fe_mul(fe_make((uint32_t)(k + 1), (uint32_t)((k + 1) >> 32), 0, 0), top[pads + k + 1]) : fe_zero();
}
// numerators and denominators of the weights c_i = y_i / M'(x_i); 0 / 1 at a dummy point.  A zero denominator — two equal points —
// raises the flag (every writer stores the same 1) and is replaced by 1
__global__ __launch_bounds__(256) void k_poly_weights(const fe *__restrict__ ys, const fe *__restrict__ values, uint64_t n, uint64_t W, fe *__restrict__ num,
                                                      fe *__restrict__ den, uint8_t *__restrict__ flag) {
    POLY_FOR(k, W) {
        fe y = fe_zero(), d = fe_one();
        if (k < n) {
            y = ys[k];
            d = values[k];
            if (fe_is_zero(d)) { *flag = 1; d = fe_one(); }
        }
        num[k] = y;
        den[k] = d;
    }
}

namespace {

// one call: the context, the workspace, the roots of its transforms
struct Run {
    gs_ctx *c;
    fe omega;
    uint32_t omega_log2;
    fe *ws = nullptr;
    Run(gs_ctx *ctx, const fe &w, uint32_t lg) : c(ctx), omega(w), omega_log2(lg) {}
    ~Run() { if (ws) gs_tmp_free(c, ws); }
    int reserve(const poly_plan &p) {
        void *q;
        const int rc = gs_tmp_alloc(c, p.workspace ? p.workspace : 16, &q);
        if (rc == GS_OK) ws = (fe *)q;
        return rc;
    }
    fe *at(uint64_t off) const { return ws + off; }
    void root(uint64_t points, uint8_t *bytes) const {             // of order `points` (a power of two <= 2^omega_log2)
        fe_to_bytes(bytes, fe_pow_u64(omega, 1ull << (omega_log2 - (uint32_t)gs_log2(points))));
    }
    // the batched transforms take at most 65535 rows per call
    int eval(const fe *in, uint64_t rows, uint64_t len, uint64_t n, fe *out) const {
        uint8_t wb[sizeof(fe)];
        root(n, wb);
        for (uint64_t at = 0; at < rows; at += 32768) {
            const uint32_t cnt = (uint32_t)(rows - at < 32768 ? rows - at : 32768);
            const int rc = gs_eval_polys_at_roots(c, in + at * len, cnt, len, wb, n, out + at * n);
            if (rc) return rc;
        }
        return GS_OK;
    }
    int interpolate(const fe *in, uint64_t rows, uint64_t n, fe *out) const {
        uint8_t wb[sizeof(fe)];
        root(n, wb);
        for (uint64_t at = 0; at < rows; at += 32768) {
            const uint32_t cnt = (uint32_t)(rows - at < 32768 ? rows - at : 32768);
            const int rc = gs_interpolate_roots(c, in + at * n, cnt, wb, n, out + at * n);
            if (rc) return rc;
        }
        return GS_OK;
    }
};

#define POLY_LAUNCH(r, kernel, items, ...)                                                                              \
    do {                                                                                                                \
        hipLaunchKernelGGL(kernel, dim3(gs_grid(items)), dim3(256), 0, (r).c->stream, __VA_ARGS__);                     \
        GS_LAUNCH_CHECK((r).c);                                                                                         \
    } while (0)

int build_tree(const Run &r, const poly_tree_plan &t, const fe *xs) {
    const uint64_t W = t.W, tree = 2 * W;
    POLY_LAUNCH(r, k_poly_leaves, W, xs, t.n, W, r.at(t.level_off(0)));
    for (uint32_t l = 0; l < t.L; l++) {
        const fe *in = r.at(t.level_off(l));
        fe *out = r.at(t.level_off(l + 1));
        const uint64_t slot = t.slot(l);
        if (t.route[l] == POLY_ROUTE_SCHOOLBOOK) {
            gs_traffic(r.c, 2 * tree * GS_ELT, tree * (slot / 2 + 1), "k_poly_pair_schoolbook");
            POLY_LAUNCH(r, k_poly_pair_schoolbook, tree, in, tree, (uint32_t)slot, out);
        } else {
            const uint64_t pn = t.build_points(l), nodes = t.nodes(l);
            int rc;
            if ((rc = r.eval(in, nodes, slot, pn, r.at(t.off_ev)))) return rc;
            gs_traffic(r.c, 3 * tree * GS_ELT, tree, "k_poly_pair_pointwise");
            POLY_LAUNCH(r, k_poly_pair_pointwise, tree, r.at(t.off_ev), tree, pn, r.at(t.off_tmp));
            if ((rc = r.interpolate(r.at(t.off_tmp), nodes / 2, pn, out))) return rc;
        }
    }
    return GS_OK;
}

// u[*cur] holds the root's vector (W elements); on return u[*cur] holds the leaves' values
int walk_down(const Run &r, const poly_tree_plan &t, int *cur) {
    const uint64_t W = t.W;
    for (uint32_t l = t.L; l-- > 0;) {
        const uint64_t half = 1ull << l, N = 2 * half;
        const fe *level = r.at(t.level_off(l)), *u = r.at(t.off_u[*cur]);
        fe *next = r.at(t.off_u[*cur ^ 1]);
        if (t.route[l] == POLY_ROUTE_SCHOOLBOOK) {
            gs_traffic(r.c, 4 * W * GS_ELT, W * (half + 1), "k_poly_down_schoolbook");
            POLY_LAUNCH(r, k_poly_down_schoolbook, W, level, u, W, (uint32_t)half, next);
        } else {
            fe *eu = r.at(t.off_tmp), *em = r.at(t.off_ev), *res = r.at(t.off_ev) + 2 * W, *pr = r.at(t.off_pr);
            int rc;
            if ((rc = r.eval(u, W / N, N, N, eu))) return rc;
            if ((rc = r.eval(level, W / half, N, N, em))) return rc;
            gs_traffic(r.c, 5 * W * GS_ELT, 2 * W, "k_poly_down_pointwise");
            POLY_LAUNCH(r, k_poly_down_pointwise, 2 * W, eu, em, 2 * W, N, pr);
            if ((rc = r.interpolate(pr, W / half, N, res))) return rc;
            POLY_LAUNCH(r, k_poly_take_high, W, res, W, half, next);
        }
        *cur ^= 1;
    }
    return GS_OK;
}

// u[*cur] holds the leaves' weights (W elements); on return u[*cur] holds the root's combination
int walk_up(const Run &r, const poly_tree_plan &t, int *cur) {
    const uint64_t W = t.W;
    for (uint32_t l = 0; l < t.L; l++) {
        const uint64_t half = 1ull << l, N = 2 * half;
        const fe *level = r.at(t.level_off(l)), *nv = r.at(t.off_u[*cur]);
        fe *next = r.at(t.off_u[*cur ^ 1]);
        if (t.route[l] == POLY_ROUTE_SCHOOLBOOK) {
            gs_traffic(r.c, 4 * W * GS_ELT, 2 * W * half, "k_poly_up_schoolbook");
            POLY_LAUNCH(r, k_poly_up_schoolbook, W, level, nv, W, (uint32_t)half, next);
        } else {
            fe *en = r.at(t.off_ev), *em = r.at(t.off_pr), *sum = r.at(t.off_tmp);
            int rc;
            if ((rc = r.eval(nv, W / half, half, N, en))) return rc;
            if ((rc = r.eval(level, W / half, N, N, em))) return rc;
            gs_traffic(r.c, 5 * W * GS_ELT, 2 * W, "k_poly_up_pointwise");
            POLY_LAUNCH(r, k_poly_up_pointwise, W, en, em, W, N, sum);
            if ((rc = r.interpolate(sum, W / N, N, next))) return rc;
        }
        *cur ^= 1;
    }
    return GS_OK;
}

// f (s.prec elements, f[0] != 0) lies at s.off_f; *g receives where the s.prec terms of 1 / f stand
int series_inverse(const Run &r, const poly_series_plan &s, const fe **g) {
    const fe *f = r.at(s.off_f);
    fe *gs[2] = {r.at(s.off_g[0]), r.at(s.off_g[1])}, *ef = r.at(s.off_ef), *eg = r.at(s.off_eg);
    hipLaunchKernelGGL(k_poly_series_seed, dim3(1), dim3(64), 0, r.c->stream, f, (uint32_t)s.seed, gs[0]);
    GS_LAUNCH_CHECK(r.c);
    int cur = 0;
    for (uint32_t step = 0; step < s.steps; step++) {
        const uint64_t m = s.seed << step, pts = s.step_points(step);
        int rc;
        if ((rc = r.eval(f, 1, 2 * m < s.prec ? 2 * m : s.prec, pts, ef))) return rc;
        if ((rc = r.eval(gs[cur], 1, m, pts, eg))) return rc;
        POLY_LAUNCH(r, k_poly_newton, pts, ef, pts, eg);
        if ((rc = r.interpolate(eg, 1, pts, gs[cur ^ 1]))) return rc;
        cur ^= 1;
    }
    *g = gs[cur];
    return GS_OK;
}

// out[k] = (a b)[from + k], k < count; out overlaps neither operand
int product_range(const Run &r, const poly_product_plan &m, const fe *a, const fe *b, uint64_t from, uint64_t count, fe *out) {
    if (!count) return GS_OK;
    if (!m.points) {
        gs_traffic(r.c, (m.la + m.lb + count) * GS_ELT, count * (m.la < m.lb ? m.la : m.lb), "k_poly_product_direct");
        POLY_LAUNCH(r, k_poly_product_direct, count, a, m.la, b, m.lb, from, count, out);
        return GS_OK;
    }
    fe *ea = r.at(m.off_ea), *eb = r.at(m.off_eb), *res = r.at(m.off_res);
    int rc;
    if ((rc = r.eval(a, 1, m.la, m.points, ea))) return rc;
    if ((rc = r.eval(b, 1, m.lb, m.points, eb))) return rc;
    if ((rc = gs_vec_mul(r.c, ea, eb, m.points, ea))) return rc;
    if ((rc = r.interpolate(ea, 1, m.points, res))) return rc;
    POLY_LAUNCH(r, k_poly_window, count, res, m.points, from, count, out);
    return GS_OK;
}

// a = q b + r, b[lb - 1] != 0; q_out (nq, or one zero when la < lb) and r_out (lb - 1) may be null
int divide(const Run &r, const poly_div_plan &d, const fe *a, const fe *b, fe *q_out, fe *r_out) {
    if (!d.nq) {
        if (q_out) POLY_LAUNCH(r, k_poly_fill, 1, fe_zero(), 1, q_out);
        if (r_out && d.lr) POLY_LAUNCH(r, k_poly_window, d.lr, a, d.la, 0, d.lr, r_out);
        return GS_OK;
    }
    int rc;
    fe *ra = r.at(d.off_ra), *qrev = r.at(d.off_qrev), *q = q_out ? q_out : r.at(d.off_q);
    POLY_LAUNCH(r, k_poly_reverse, d.nq, a, d.la, d.la - 1, d.nq, ra);
    POLY_LAUNCH(r, k_poly_reverse, d.nq, b, d.lb, d.lb - 1, d.nq, r.at(d.series.off_f));
    const fe *g;
    if ((rc = series_inverse(r, d.series, &g))) return rc;
    if ((rc = product_range(r, d.quotient, ra, g, 0, d.nq, qrev))) return rc;
    POLY_LAUNCH(r, k_poly_reverse, d.nq, qrev, d.nq, d.nq - 1, d.nq, q);
    if (r_out && d.lr) {
        fe *qb = r.at(d.off_qb);
        if ((rc = product_range(r, d.back, q, b, 0, d.lr, qb))) return rc;
        gs_traffic(r.c, 3 * d.lr * GS_ELT, 0, "k_poly_remainder");
        POLY_LAUNCH(r, k_poly_remainder, d.lr, a, qb, d.lr, r_out);
    }
    return GS_OK;
}

// the polynomial at p.off_poly (W coefficients) at the tree's W points: on return u[*cur] holds the values
int values_at_tree_points(const Run &r, const poly_plan &p, int *cur) {
    const poly_tree_plan &t = p.tree;
    const uint64_t W = t.W;
    fe *poly = r.at(p.off_poly), *rev = r.at(p.off_rev);
    int rc;
    POLY_LAUNCH(r, k_poly_reverse, W, r.at(t.level_off(t.L)), W + 1, W, W, r.at(p.root.off_f));
    const fe *g;
    if ((rc = series_inverse(r, p.root, &g))) return rc;
    POLY_LAUNCH(r, k_poly_reverse, W, poly, W, W - 1, W, rev);
    if ((rc = product_range(r, p.top, rev, g, 0, W, poly))) return rc;
    *cur = 0;
    POLY_LAUNCH(r, k_poly_reverse, W, poly, W, W - 1, W, r.at(t.off_u[0]));
    return walk_down(r, t, cur);
}

// the checks every entry shares: omega canonical and of order 2^omega_log2, long enough for the plan
int check_omega(gs_ctx *c, const char *who, const gs_elt *omega_bytes, uint32_t omega_log2, const poly_plan &p, fe *omega) {
    if (!omega_bytes) return gs_fail(c, GS_ERR_ARG, "%s: omega is required", who);
    *omega = fe_from_bytes(omega_bytes);
    if (fe_ge_p(*omega)) return gs_fail(c, GS_ERR_ARG, "%s: omega is not a canonical element", who);
    if (omega_log2 > 63) return gs_fail(c, GS_ERR_ARG, "%s: omega_log2 is %u, at most 63", who, omega_log2);
    if (p.need_log2 > omega_log2)
        return gs_fail(c, GS_ERR_ARG, "%s: omega_log2 is %u, this call needs transforms of 2^%u points", who, omega_log2, p.need_log2);
    const bool order = omega_log2 ? fe_eq(fe_pow_u64(*omega, 1ull << (omega_log2 - 1)), fe_neg(fe_one())) : fe_eq(*omega, fe_one());
    if (!order) return gs_fail(c, GS_ERR_ARG, "%s: omega is not of order 2^%u", who, omega_log2);
    return GS_OK;
}

}  // namespace

extern "C" {

uint32_t gs_poly_schoolbook_log2(uint32_t log2_len) {
    return g_poly_switch_log2.exchange(log2_len > POLY_SWITCH_MAX ? POLY_SWITCH_MAX : (log2_len < POLY_SWITCH_MIN ? POLY_SWITCH_MIN : log2_len));
}

int gs_poly_from_roots(gs_ctx *c, const gs_elt *omega_bytes, uint32_t omega_log2, const void *xs, uint64_t n, void *out) {
    if (!c) return GS_ERR_ARG;
    poly_plan p;
    if (const char *why = poly_plan_build(POLY_OP_FROM_ROOTS, n, 0, g_poly_switch_log2.load(), (uint32_t)GS_ELT, p))
        return gs_fail(c, GS_ERR_ARG, "poly_from_roots: %s (n %llu)", why, (unsigned long long)n);
    fe omega;
    int rc;
    if ((rc = check_omega(c, "poly_from_roots", omega_bytes, omega_log2, p, &omega))) return rc;
    if (!out) return gs_fail(c, GS_ERR_ARG, "poly_from_roots: out is required");
    if (n && !xs) return gs_fail(c, GS_ERR_ARG, "poly_from_roots: xs is required");
    Run r(c, omega, omega_log2);
    if (!n) {
        POLY_LAUNCH(r, k_poly_fill, 1, fe_one(), 1, (fe *)out);
        return GS_OK;
    }
    if ((rc = r.reserve(p))) return rc;
    if ((rc = build_tree(r, p.tree, (const fe *)xs))) return rc;
    POLY_LAUNCH(r, k_poly_window, n + 1, r.at(p.tree.level_off(p.tree.L)), p.tree.W + 1, p.tree.pads, n + 1, (fe *)out);
    return GS_OK;
}

int gs_poly_div(gs_ctx *c, const gs_elt *omega_bytes, uint32_t omega_log2, const void *a, uint64_t la, const void *b, uint64_t lb, void *q, void *rem) {
    if (!c) return GS_ERR_ARG;
    poly_plan p;
    if (const char *why = poly_plan_build(POLY_OP_DIV, lb, la, g_poly_switch_log2.load(), (uint32_t)GS_ELT, p))
        return gs_fail(c, GS_ERR_ARG, "poly_div: %s (la %llu, lb %llu)", why, (unsigned long long)la, (unsigned long long)lb);
    fe omega;
    int rc;
    if ((rc = check_omega(c, "poly_div", omega_bytes, omega_log2, p, &omega))) return rc;
    if (!a) return gs_fail(c, GS_ERR_ARG, "poly_div: a is required");
    if (!b) return gs_fail(c, GS_ERR_ARG, "poly_div: b is required");
    fe lead;                                                      // the family's only read-back
    if ((rc = gs_download(c, &lead, (const fe *)b + (lb - 1), GS_ELT))) return rc;
    if (fe_is_zero(lead)) return gs_fail(c, GS_ERR_ARG, "poly_div: b: the leading coefficient b[lb - 1] is zero");
    if (!q && !rem) return GS_OK;
    Run r(c, omega, omega_log2);
    if ((rc = r.reserve(p))) return rc;
    return divide(r, p.div, (const fe *)a, (const fe *)b, (fe *)q, (fe *)rem);
}

int gs_poly_eval_points(gs_ctx *c, const gs_elt *omega_bytes, uint32_t omega_log2, const void *poly, uint64_t len, const void *xs, uint64_t npoints,
                        void *out) {
    if (!c) return GS_ERR_ARG;
    poly_plan p;
    if (const char *why = poly_plan_build(POLY_OP_EVAL, npoints, len, g_poly_switch_log2.load(), (uint32_t)GS_ELT, p))
        return gs_fail(c, GS_ERR_ARG, "poly_eval_points: %s (len %llu, npoints %llu)", why, (unsigned long long)len, (unsigned long long)npoints);
    fe omega;
    int rc;
    if ((rc = check_omega(c, "poly_eval_points", omega_bytes, omega_log2, p, &omega))) return rc;
    if (len && !poly) return gs_fail(c, GS_ERR_ARG, "poly_eval_points: poly is required");
    if (npoints && !xs) return gs_fail(c, GS_ERR_ARG, "poly_eval_points: xs is required");
    if (npoints && !out) return gs_fail(c, GS_ERR_ARG, "poly_eval_points: out is required");
    if (!npoints) return GS_OK;
    Run r(c, omega, omega_log2);
    if (!len) {
        POLY_LAUNCH(r, k_poly_fill, npoints, fe_zero(), npoints, (fe *)out);
        return GS_OK;
    }
    if ((rc = r.reserve(p))) return rc;
    const poly_tree_plan &t = p.tree;
    if ((rc = build_tree(r, t, (const fe *)xs))) return rc;
    if (p.reduce) {
        if ((rc = divide(r, p.div, (const fe *)poly, r.at(t.level_off(t.L)), nullptr, r.at(p.off_poly)))) return rc;
    } else {
        POLY_LAUNCH(r, k_poly_window, t.W, (const fe *)poly, len, 0, t.W, r.at(p.off_poly));
    }
    int cur;
    if ((rc = values_at_tree_points(r, p, &cur))) return rc;
    POLY_LAUNCH(r, k_poly_window, npoints, r.at(t.off_u[cur]), t.W, 0, npoints, (fe *)out);
    return GS_OK;
}

int gs_poly_interpolate_points(gs_ctx *c, const gs_elt *omega_bytes, uint32_t omega_log2, const void *xs, const void *ys, uint64_t n, void *out,
                               void *flag) {
    if (!c) return GS_ERR_ARG;
    poly_plan p;
    if (const char *why = poly_plan_build(POLY_OP_INTERPOLATE, n, 0, g_poly_switch_log2.load(), (uint32_t)GS_ELT, p))
        return gs_fail(c, GS_ERR_ARG, "poly_interpolate_points: %s (n %llu)", why, (unsigned long long)n);
    fe omega;
    int rc;
    if ((rc = check_omega(c, "poly_interpolate_points", omega_bytes, omega_log2, p, &omega))) return rc;
    if (!xs) return gs_fail(c, GS_ERR_ARG, "poly_interpolate_points: xs is required");
    if (!ys) return gs_fail(c, GS_ERR_ARG, "poly_interpolate_points: ys is required");
    if (!out) return gs_fail(c, GS_ERR_ARG, "poly_interpolate_points: out is required");
    if (!flag) return gs_fail(c, GS_ERR_ARG, "poly_interpolate_points: flag is required");
    Run r(c, omega, omega_log2);
    if ((rc = r.reserve(p))) return rc;
    const poly_tree_plan &t = p.tree;
    GS_HIP(c, hipMemsetAsync(flag, 0, 1, c->stream));
    if ((rc = build_tree(r, t, (const fe *)xs))) return rc;
    POLY_LAUNCH(r, k_poly_derivative, t.W, r.at(t.level_off(t.L)), t.pads, n, t.W, r.at(p.off_poly));
    int cur;
    if ((rc = values_at_tree_points(r, p, &cur))) return rc;
    POLY_LAUNCH(r, k_poly_weights, t.W, (const fe *)ys, r.at(t.off_u[cur]), n, t.W, r.at(p.off_num), r.at(p.off_den), (uint8_t *)flag);
    cur ^= 1;
    if ((rc = gs_vec_div(c, r.at(p.off_num), r.at(p.off_den), t.W, r.at(t.off_u[cur])))) return rc;
    if ((rc = walk_up(r, t, &cur))) return rc;
    POLY_LAUNCH(r, k_poly_window, n, r.at(t.off_u[cur]), t.W, t.pads, n, (fe *)out);
    return GS_OK;
}

}  // extern "C"
