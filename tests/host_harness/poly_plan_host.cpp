// The host plan of include/gstark_poly.h's entries (genstark_amd/csrc/poly_plan.h) on its own: for every operation, every size of the
// lists below and every switch-over 1 .. 12 the plan's tree has the levels, slots and routes the size calls for, every buffer a step
// touches lies inside its region, no two regions overlap and all lie below the workspace it reports, no step's transform is longer than
// the 2^need_log2 points it reports, the Newton steps reach the precision, and 2^20 + 1 of anything is refused naming the argument.
// Built with -fsanitize=address,undefined by tests/test_poly.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../genstark_amd/csrc/poly_plan.h"

static int g_op;
static uint64_t g_n, g_len;
static uint32_t g_switch;

#define CHECK(cond)                                                                                                                     \
    do {                                                                                                                                \
        if (!(cond)) {                                                                                                                  \
            std::printf("FAILED %s (line %d): op %d n %llu len %llu switch %u\n", #cond, __LINE__, g_op, (unsigned long long)g_n,       \
                        (unsigned long long)g_len, g_switch);                                                                           \
            std::exit(1);                                                                                                               \
        }                                                                                                                               \
    } while (0)

// the region that starts at `off`; a buffer of `elems` elements there must fit it
static void check_buffer(const poly_plan &p, uint64_t off, uint64_t elems) {
    for (uint32_t i = 0; i < p.nregions; i++) {
        const poly_region &r = p.regions[i];
        if (off >= r.off && off < r.off + (r.size ? r.size : 1)) {
            CHECK(off + elems <= r.off + r.size);
            return;
        }
    }
    CHECK(elems == 0);
}

static void check_points(const poly_plan &p, uint64_t points) {
    CHECK(points && !(points & (points - 1)));
    CHECK(points <= (1ull << p.need_log2));
}

static void check_regions(const poly_plan &p) {
    CHECK(p.nregions <= POLY_MAX_REGIONS);
    uint64_t end = 0;
    for (uint32_t i = 0; i < p.nregions; i++) {
        const poly_region &a = p.regions[i];
        CHECK(a.name && a.off % 16 == 0);
        for (uint32_t j = i + 1; j < p.nregions; j++) {
            const poly_region &b = p.regions[j];
            CHECK(a.off + a.size <= b.off || b.off + b.size <= a.off);
        }
        if (a.off + a.size > end) end = a.off + a.size;
    }
    CHECK(end * p.elt_bytes <= p.workspace && p.workspace <= POLY_WORKSPACE_CAP);
}

static void check_tree(const poly_plan &p, uint64_t n) {
    const poly_tree_plan &t = p.tree;
    CHECK(t.n == n && t.W >= n && t.W >= 1 && (t.W == 1 || t.W / 2 < n) && t.W == (1ull << t.L) && t.pads == t.W - n && t.levels == t.L + 1);
    check_buffer(p, t.off, (uint64_t)t.levels * 2 * t.W);
    check_buffer(p, t.off_u[0], t.W);
    check_buffer(p, t.off_u[1], t.W);
    for (uint32_t l = 0; l <= t.L; l++) {
        CHECK(t.nodes(l) * t.slot(l) == 2 * t.W);                    // every level fills 2W elements
        CHECK(t.slot(l) >= (1ull << l) + 1);                          // ... and a slot holds a node's 2^l + 1 coefficients
        CHECK(t.level_off(l) == t.off + (uint64_t)l * 2 * t.W);
    }
    CHECK(t.nodes(t.L) == 1);
    for (uint32_t l = 0; l < t.L; l++) {
        const bool schoolbook = t.slot(l) <= (1ull << p.switch_log2);
        CHECK(t.route[l] == (schoolbook ? POLY_ROUTE_SCHOOLBOOK : POLY_ROUTE_TRANSFORM));
        if (l) CHECK(t.route[l] >= t.route[l - 1]);                   // once through transforms, always
        if (schoolbook) continue;
        // build: the children's transforms, their products, the parents
        CHECK(t.build_points(l) >= t.slot(l) + 1 && t.build_points(l) == t.slot(l + 1));
        check_points(p, t.build_points(l));
        check_buffer(p, t.off_ev, t.nodes(l) * t.build_points(l));
        check_buffer(p, t.off_tmp, t.nodes(l) / 2 * t.build_points(l));
        // down: the parents' transforms, the children's nodes' transforms, the products, their interpolants
        const uint64_t N = t.walk_points(l), half = 1ull << l;
        CHECK(N == t.slot(l) && half + 1 <= N && half + half <= N);   // the node and the middle product fit the cyclic length
        check_points(p, N);
        check_buffer(p, t.off_tmp, t.W / N * N);
        check_buffer(p, t.off_ev, 2 * t.W + t.W / half * N);          // (the interpolants stand 2W into the region)
        check_buffer(p, t.off_pr, t.W / half * N);
        // up: the children's vectors' transforms, the nodes' transforms, the sums
        CHECK(half + half <= N);                                      // N_left M_right has 2^l + 2^l coefficients
        check_buffer(p, t.off_ev, t.W / half * N);
    }
}

static void check_series(const poly_plan &p, const poly_series_plan &s, uint64_t prec) {
    CHECK(s.prec == prec && s.seed >= 1 && s.seed <= POLY_SEED && s.seed <= prec);
    CHECK((s.seed << s.steps) >= prec && (!s.steps || (s.seed << (s.steps - 1)) < prec));
    check_buffer(p, s.off_f, prec);
    check_buffer(p, s.off_g[0], s.seed);
    for (uint32_t step = 0; step < s.steps; step++) {
        const uint64_t m = s.seed << step, pts = s.step_points(step);
        CHECK(pts >= 2 * m + 2 * m - 2);                              // g (2 - f g) for f of 2m and g of m coefficients does not wrap
        check_points(p, pts);
        check_buffer(p, s.off_ef, pts);
        check_buffer(p, s.off_eg, pts);
        check_buffer(p, s.off_g[0], pts);
        check_buffer(p, s.off_g[1], pts);
    }
}

static void check_product(const poly_plan &p, const poly_product_plan &m, uint64_t la, uint64_t lb) {
    CHECK(m.la == la && m.lb == lb);
    const bool direct = !la || !lb || (la < lb ? la : lb) <= POLY_DIRECT;
    CHECK((m.points == 0) == direct);
    if (direct) return;
    CHECK(m.points >= la + lb - 1 && m.points / 2 < la + lb - 1);
    check_points(p, m.points);
    check_buffer(p, m.off_ea, m.points);
    check_buffer(p, m.off_eb, m.points);
    check_buffer(p, m.off_res, m.points);
}

static void check_division(const poly_plan &p, const poly_div_plan &d, uint64_t la, uint64_t lb) {
    CHECK(d.la == la && d.lb == lb && d.lr == lb - 1);
    if (la < lb) { CHECK(d.nq == 0); return; }
    CHECK(d.nq == la - lb + 1);
    check_buffer(p, d.off_ra, d.nq);
    check_buffer(p, d.off_qrev, d.nq);
    check_buffer(p, d.off_q, d.nq);
    check_series(p, d.series, d.nq);
    check_product(p, d.quotient, d.nq, d.nq);
    if (d.lr) {
        check_buffer(p, d.off_qb, d.lr);
        check_product(p, d.back, d.nq < d.lr ? d.nq : d.lr, d.lr);
    }
}

static uint64_t g_plans = 0;

static void check(int op, uint64_t n, uint64_t len, uint32_t sw, uint32_t elt) {
    g_op = op; g_n = n; g_len = len; g_switch = sw;
    poly_plan p;
    const char *why = poly_plan_build(op, n, len, sw, elt, p);
    CHECK(why == nullptr);
    CHECK(p.switch_log2 == sw && p.elt_bytes == elt && p.need_log2 <= POLY_MAX_LOG2 + 1);
    check_regions(p);
    switch (op) {
    case POLY_OP_FROM_ROOTS:
        if (n) check_tree(p, n);
        else CHECK(p.workspace == 0);
        break;
    case POLY_OP_DIV:
        check_division(p, p.div, len, n);
        break;
    case POLY_OP_EVAL:
    case POLY_OP_INTERPOLATE:
        if (!n || (op == POLY_OP_EVAL && !len)) { CHECK(p.workspace == 0 && p.need_log2 == 0); break; }
        check_tree(p, n);
        check_buffer(p, p.off_poly, p.tree.W);
        check_buffer(p, p.off_rev, p.tree.W);
        CHECK(p.reduce == (op == POLY_OP_EVAL && len > p.tree.W));
        if (p.reduce) check_division(p, p.div, len, p.tree.W + 1);
        check_series(p, p.root, p.tree.W);
        check_product(p, p.top, p.tree.W, p.tree.W);
        if (op == POLY_OP_INTERPOLATE) {
            check_buffer(p, p.off_num, p.tree.W);
            check_buffer(p, p.off_den, p.tree.W);
        }
        break;
    }
    g_plans++;
}

static void refused(int op, uint64_t n, uint64_t len, const char *word) {
    g_op = op; g_n = n; g_len = len; g_switch = 8;
    poly_plan p;
    const char *why = poly_plan_build(op, n, len, 8, 32, p);
    CHECK(why != nullptr && std::strstr(why, word) == why);          // the message begins with the argument's name
}

int main() {
    const uint64_t sizes[] = {1, 2, 3, 255, 256, 257, 1ull << 20};
    const uint64_t others[] = {1, 2, 3, 31, 32, 33, 64, 65, 255, 256, 257, 1000, (1ull << 20) - 1, 1ull << 20};
    for (uint32_t elt : {16u, 32u})
        for (uint32_t sw = 1; sw <= 12; sw++) {
            check(POLY_OP_FROM_ROOTS, 0, 0, sw, elt);
            check(POLY_OP_EVAL, 0, 5, sw, elt);
            check(POLY_OP_EVAL, 5, 0, sw, elt);
            for (uint64_t n : sizes) {
                check(POLY_OP_FROM_ROOTS, n, 0, sw, elt);
                check(POLY_OP_INTERPOLATE, n, 0, sw, elt);
                for (uint64_t len : others) {
                    check(POLY_OP_EVAL, n, len, sw, elt);
                    check(POLY_OP_DIV, n, len, sw, elt);                 // (lb = n, la = len)
                    check(POLY_OP_DIV, len, n, sw, elt);
                }
            }
        }
    // the setter's clamp is the plan's too
    {
        poly_plan p;
        CHECK(!poly_plan_build(POLY_OP_FROM_ROOTS, 1000, 0, 0, 16, p) && p.switch_log2 == POLY_SWITCH_MIN);
        CHECK(!poly_plan_build(POLY_OP_FROM_ROOTS, 1000, 0, 99, 16, p) && p.switch_log2 == POLY_SWITCH_MAX);
    }
    const uint64_t over = (1ull << 20) + 1;
    refused(POLY_OP_FROM_ROOTS, over, 0, "n:");
    refused(POLY_OP_INTERPOLATE, over, 0, "n:");
    refused(POLY_OP_INTERPOLATE, 0, 0, "n:");
    refused(POLY_OP_EVAL, over, 5, "npoints:");
    refused(POLY_OP_EVAL, 5, over, "len:");
    refused(POLY_OP_DIV, 5, over, "la:");
    refused(POLY_OP_DIV, over, 5, "lb:");
    refused(POLY_OP_DIV, 5, 0, "la:");
    refused(POLY_OP_DIV, 0, 5, "lb:");
    refused(77, 5, 5, "op:");
    std::printf("%llu plans ok\n", (unsigned long long)g_plans);
    return 0;
}
