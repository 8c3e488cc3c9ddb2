// poly_plan.h — how the entries of include/gstark_poly.h are laid out on the device: the subproduct tree's levels and slots, the route
// of every level, every transform length, and the workspace as offsets into ONE block (poly.hip is the device side; DESIGN.md 3.16 has
// the argument).  Plain C++, no HIP: it is tested on its own (tests/host_harness/poly_plan_host.cpp).
//   tree        n points are padded to W = 2^L points with dummy points x = 0, so EVERY node is monic of full degree: level l holds
//               W >> l nodes, node j the product of (x - x_i) over i in [j 2^l, (j + 1) 2^l), 2^l + 1 coefficients in a slot of
//               2 << l elements (zeros above).  Every level is kept: level l starts at element l * 2W of the tree region.  The top node is
//               x^(W - n) M(x), M the product over the n real points: M and anything computed from it is read `pads` = W - n places on.
//   steps       one level to the next (build), a parent's vector to its two children (down), two children to their parent (up).  A
//               step whose CHILD slot (2 << l elements) is at most 2^switch elements is a per-thread schoolbook sum; above it goes
//               through batched transforms: of 2 * slot points when building (the product has slot + 1 coefficients), of slot points
//               down and up (the middle product and the combination fit the cyclic length exactly).
//   series      the inverse of a power series to `prec` terms: POLY_SEED terms by one thread, then Newton steps m -> 2m, each through
//               transforms of 4m points (g (2 - f g) has fewer than 4m coefficients: no wrap-around).
//   products    of two single polynomials: per-thread sums when the shorter operand has at most POLY_DIRECT coefficients, else
//               transforms of the next power of two above la + lb - 1 points.
// No two regions of a plan overlap: nothing is aliased, every buffer of a call has its own range.
#pragma once
#include <cstdint>

#define POLY_MAX_LEN (1ull << 20)            // coefficients or points per operand
#define POLY_MAX_LOG2 20u
#define POLY_SEED 32u                        // terms of a series inverse one thread computes before the Newton steps
#define POLY_DIRECT 32u                      // a product whose shorter operand is at most this long is summed per thread
// Measured (profiles/poly.md; evaluation of 2^16 coefficients at 2^16 points, ms per call by this exponent, 128-bit | 224-bit flavour):
// 4: 3.44 | 14.2, 6: 3.17 | 13.1, 7: 3.01 | 12.5, 8: 2.98 | 12.2, 9: 3.04 | 12.3, 10: 3.30 | 13.2 — the same optimum as boundary.hip's tree.
#define POLY_SWITCH_DEFAULT 8u               // child slots of at most 2^8 elements are schoolbook
#define POLY_SWITCH_MIN 1u
#define POLY_SWITCH_MAX 12u
#define POLY_WORKSPACE_CAP (4ull << 30)      // bytes of workspace a call may take from the context's block cache (the largest plan, an
                                             // interpolation through 2^20 points of 32-byte elements, takes 2.4 GiB)

enum { POLY_OP_FROM_ROOTS = 0, POLY_OP_DIV = 1, POLY_OP_EVAL = 2, POLY_OP_INTERPOLATE = 3 };
enum { POLY_ROUTE_SCHOOLBOOK = 0, POLY_ROUTE_TRANSFORM = 1 };

static inline uint32_t poly_log2_ceil(uint64_t n) { uint32_t l = 0; while ((1ull << l) < n) l++; return l; }
static inline uint64_t poly_pow2_ceil(uint64_t n) { return 1ull << poly_log2_ceil(n); }

// one region of the workspace, in ELEMENTS
struct poly_region { const char *name; uint64_t off, size; };
#define POLY_MAX_REGIONS 40

struct poly_tree_plan {
    uint64_t n = 0, W = 1, pads = 0;         // points, padded points, dummy points
    uint32_t L = 0, levels = 1;              // W = 2^L, levels 0 .. L
    uint32_t route[POLY_MAX_LOG2 + 1] = {};  // route[l]: of the steps between level l (the children) and level l + 1, l < L
    uint64_t off = 0;                        // the tree region: levels * 2W elements
    uint64_t off_ev = 0, off_pr = 0;         // transforms: 4W; the nodes' transforms (up) or the pointwise products (down): 2W
    uint64_t off_tmp = 0;                    // 2W: products before interpolation (build), a parent's transform (down), sums (up)
    uint64_t off_u[2] = {0, 0};              // the vectors walking down or up, W each, written by turns
    uint64_t level_off(uint32_t l) const { return off + (uint64_t)l * 2 * W; }
    uint64_t slot(uint32_t l) const { return 2ull << l; }
    uint64_t nodes(uint32_t l) const { return W >> l; }
    uint64_t build_points(uint32_t l) const { return 4ull << l; }       // transform length of the build step from level l
    uint64_t walk_points(uint32_t l) const { return 2ull << l; }        // ... of the down and up steps between levels l and l + 1
};

struct poly_series_plan {                    // g = 1 / f mod x^prec
    uint64_t prec = 0, seed = 0;             // terms wanted, terms one thread computes
    uint32_t steps = 0;                      // Newton steps: seed << steps >= prec
    uint64_t off_f = 0;                      // prec elements: f, zero-extended
    uint64_t off_g[2] = {0, 0};              // 4 * (seed << (steps - 1)) each (at least seed): g and the next g by turns
    uint64_t off_ef = 0, off_eg = 0;         // transforms of the last step each
    uint64_t buf = 0;                        // elements of each of the four
    uint64_t step_points(uint32_t s) const { return (4 * seed) << s; }  // transform length of step s (m = seed << s terms to 2m)
};

struct poly_product_plan {                   // (a b)[from .. from + count) for la and lb coefficients
    uint64_t la = 0, lb = 0, points = 0;     // points = 0: per-thread sums
    uint64_t off_ea = 0, off_eb = 0, off_res = 0;
};

struct poly_div_plan {                       // a = q b + r
    uint64_t la = 0, lb = 0, nq = 0, lr = 0; // nq = la - lb + 1 quotient coefficients (0: la < lb), lr = lb - 1 of the remainder
    uint64_t off_ra = 0, off_qrev = 0, off_q = 0, off_qb = 0;
    poly_series_plan series;
    poly_product_plan quotient, back;        // rev(a) / rev(b), and (q mod x^lr)(b mod x^lr) for the remainder
};

struct poly_plan {
    int op = 0;
    uint32_t switch_log2 = POLY_SWITCH_DEFAULT, elt_bytes = 0;
    poly_tree_plan tree;
    bool reduce = false;                     // evaluation: the polynomial is longer than W and is first divided by the top node
    poly_div_plan div;
    poly_series_plan root;                   // 1 / rev(top node) mod x^W
    poly_product_plan top;                   // rev(polynomial) times that inverse, W coefficients kept
    uint64_t off_poly = 0;                   // W: the polynomial walked down (evaluation: the input or its remainder; interpolation: M'),
                                             // then its reversed product with the root's inverse
    uint64_t off_rev = 0;                    // W: that polynomial, highest coefficient first
    uint64_t off_num = 0, off_den = 0;       // interpolation: W each, y_i and M'(x_i), then the weights in place of y_i
    uint32_t need_log2 = 0;                  // the longest transform of the call has 2^need_log2 points (0: none)
    uint64_t workspace = 0;                  // bytes
    uint32_t nregions = 0;
    poly_region regions[POLY_MAX_REGIONS];
};

namespace poly_detail {
struct layout {
    poly_plan &p;
    uint64_t at = 0;
    uint64_t take(const char *name, uint64_t elems) {
        const uint64_t here = at;
        at += (elems + 15) & ~15ull;                                  // every region starts on a multiple of 16 elements
        if (p.nregions < POLY_MAX_REGIONS) p.regions[p.nregions] = poly_region{name, here, elems};
        p.nregions++;
        return here;
    }
    void need(uint64_t points) { const uint32_t l = poly_log2_ceil(points); if (points > 1 && l > p.need_log2) p.need_log2 = l; }
};

static inline void tree(layout &w, uint64_t n, uint32_t switch_log2, poly_tree_plan &t) {
    t = poly_tree_plan();
    t.n = n;
    t.L = poly_log2_ceil(n < 1 ? 1 : n);
    t.W = 1ull << t.L;
    t.pads = t.W - n;
    t.levels = t.L + 1;
    t.off = w.take("tree", (uint64_t)t.levels * 2 * t.W);
    t.off_ev = w.take("tree.ev", 4 * t.W);
    t.off_pr = w.take("tree.pr", 2 * t.W);
    t.off_tmp = w.take("tree.tmp", 2 * t.W);
    t.off_u[0] = w.take("tree.u0", t.W);
    t.off_u[1] = w.take("tree.u1", t.W);
    for (uint32_t l = 0; l < t.L; l++) {
        t.route[l] = t.slot(l) <= (1ull << switch_log2) ? POLY_ROUTE_SCHOOLBOOK : POLY_ROUTE_TRANSFORM;
        if (t.route[l] == POLY_ROUTE_TRANSFORM) w.need(t.build_points(l));      // (the walks take half of it)
    }
}

static inline void series(layout &w, uint64_t prec, poly_series_plan &s) {
    s = poly_series_plan();
    s.prec = prec;
    s.seed = prec < POLY_SEED ? prec : POLY_SEED;
    while (s.seed && (s.seed << s.steps) < prec) s.steps++;
    s.buf = s.steps ? s.step_points(s.steps - 1) : s.seed;
    s.off_f = w.take("series.f", prec);
    s.off_g[0] = w.take("series.g0", s.buf);
    s.off_g[1] = w.take("series.g1", s.buf);
    s.off_ef = w.take("series.ef", s.buf);
    s.off_eg = w.take("series.eg", s.buf);
    if (s.steps) w.need(s.buf);
}

static inline void product(layout &w, uint64_t la, uint64_t lb, poly_product_plan &m) {
    m = poly_product_plan();
    m.la = la; m.lb = lb;
    if (!la || !lb || (la < lb ? la : lb) <= POLY_DIRECT) return;
    m.points = poly_pow2_ceil(la + lb - 1);
    m.off_ea = w.take("product.ea", m.points);
    m.off_eb = w.take("product.eb", m.points);
    m.off_res = w.take("product.res", m.points);
    w.need(m.points);
}

static inline void division(layout &w, uint64_t la, uint64_t lb, poly_div_plan &d) {
    d = poly_div_plan();
    d.la = la; d.lb = lb; d.lr = lb - 1;
    if (la < lb) return;
    d.nq = la - lb + 1;
    d.off_ra = w.take("div.ra", d.nq);
    d.off_qrev = w.take("div.qrev", d.nq);
    d.off_q = w.take("div.q", d.nq);
    series(w, d.nq, d.series);
    product(w, d.nq, d.nq, d.quotient);
    if (d.lr) {
        const uint64_t lq = d.nq < d.lr ? d.nq : d.lr;
        d.off_qb = w.take("div.qb", d.lr);
        product(w, lq, d.lr, d.back);
    }
}
}  // namespace poly_detail

// Fills `p`; returns nullptr, or the reason the call is refused (naming the argument).
//   POLY_OP_FROM_ROOTS    n = the roots                       POLY_OP_EVAL         n = the points, len = the coefficients
//   POLY_OP_DIV           len = la, n = lb                    POLY_OP_INTERPOLATE  n = the points
static inline const char *poly_plan_build(int op, uint64_t n, uint64_t len, uint32_t switch_log2, uint32_t elt_bytes, poly_plan &p) {
    p = poly_plan();
    p.op = op; p.elt_bytes = elt_bytes;
    p.switch_log2 = switch_log2 < POLY_SWITCH_MIN ? POLY_SWITCH_MIN : (switch_log2 > POLY_SWITCH_MAX ? POLY_SWITCH_MAX : switch_log2);
    poly_detail::layout w{p};
    switch (op) {
    case POLY_OP_FROM_ROOTS:
        if (n > POLY_MAX_LEN) return "n: at most 2^20 roots per call";
        if (n) poly_detail::tree(w, n, p.switch_log2, p.tree);
        break;
    case POLY_OP_DIV:
        if (len > POLY_MAX_LEN) return "la: at most 2^20 coefficients per operand";
        if (n > POLY_MAX_LEN) return "lb: at most 2^20 coefficients per operand";
        if (!len) return "la: at least one coefficient";
        if (!n) return "lb: at least one coefficient";
        poly_detail::division(w, len, n, p.div);
        break;
    case POLY_OP_EVAL:
    case POLY_OP_INTERPOLATE:
        if (n > POLY_MAX_LEN) return op == POLY_OP_EVAL ? "npoints: at most 2^20 points per call" : "n: at most 2^20 points per call";
        if (op == POLY_OP_EVAL && len > POLY_MAX_LEN) return "len: at most 2^20 coefficients per operand";
        if (op == POLY_OP_INTERPOLATE && !n) return "n: at least one point";
        if (!n || (op == POLY_OP_EVAL && !len)) break;               // no point, or the zero polynomial: nothing to plan
        poly_detail::tree(w, n, p.switch_log2, p.tree);
        p.off_poly = w.take("poly", p.tree.W);
        p.off_rev = w.take("poly.rev", p.tree.W);
        if (op == POLY_OP_EVAL && len > p.tree.W) {
            p.reduce = true;
            poly_detail::division(w, len, p.tree.W + 1, p.div);
        }
        poly_detail::series(w, p.tree.W, p.root);
        poly_detail::product(w, p.tree.W, p.tree.W, p.top);
        if (op == POLY_OP_INTERPOLATE) {
            p.off_num = w.take("num", p.tree.W);
            p.off_den = w.take("den", p.tree.W);
        }
        break;
    default:
        return "op: unknown";
    }
    if (p.nregions > POLY_MAX_REGIONS) return "plan: too many regions";
    p.workspace = w.at * elt_bytes;
    if (p.workspace > POLY_WORKSPACE_CAP) return "workspace: above the cap of 4 GiB";
    return nullptr;
}
