// The host plan of gs_field_sqrt (genstark_amd/csrc/sqrt_plan.h) on its own: the split, the non-residue and the windows of the six built
// moduli and of two primes with p = 3 (mod 4) and p = 5 (mod 8); a composite is refused; window widths sum to s, the rows of the tables
// lie apart inside the stated size; and on the field of 96769 elements, with the tables and the digit hash built here on 64-bit
// integers, BOTH forms of the planned algorithm return the even root, or none, for every element of the field.
// Built with -fsanitize=address,undefined by tests/test_sqrt.py.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../genstark_amd/csrc/sqrt_plan.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, g_what);       \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static const char *g_what = "";

struct Case { const char *name; uint32_t p[SQRT_LIMBS]; uint32_t s, z; };
static const uint32_t F = 0xffffffffu;
static const Case CASES[] = {
    {"p128", {1, 0xfffffff7u, F, F, 0, 0, 0, 0}, 32, 3},
    {"q64", {0xc0000001u, 0xfffffffau, 0, 0, 0, 0, 0, 0}, 30, 3},
    {"q32", {0xfa000001u, 0, 0, 0, 0, 0, 0, 0}, 25, 3},
    {"q17", {96769, 0, 0, 0, 0, 0, 0, 0}, 9, 11},
    {"p256", {1, 0xfffffea1u, F, F, F, F, F, F}, 32, 3},
    {"p224", {1, 0, 0, F, F, F, F, 0}, 96, 11},
    {"2^255 - 19", {0xffffffedu, F, F, F, F, F, F, 0x7fffffffu}, 2, 2},
    {"2^256 - 2^32 - 977", {0xfffffc2fu, 0xfffffffeu, F, F, F, F, F, F}, 1, 3},
};

static void check_layout(const sqrt_plan &pl) {
    CHECK(pl.w == (pl.s < 8 ? pl.s : 8) && pl.windows == (pl.s + pl.w - 1) / pl.w && pl.windows <= SQRT_MAX_WINDOWS);
    uint32_t sum = 0;
    for (uint32_t j = 0; j < pl.windows; j++) {
        const uint32_t width = sqrt_window_width(pl, j);
        CHECK(width >= 1 && width <= pl.w && (j + 1 == pl.windows || width == pl.w));
        CHECK(sqrt_window_lo(pl, j) == sum);
        sum += width;
    }
    CHECK(sum == pl.s && pl.last_w == sqrt_window_width(pl, pl.windows - 1));
    // rows: [offset, offset + size) inside the table, distinct rows apart (U rows may BE T rows when w divides s)
    std::vector<int> owner(pl.table_elems, -1);
    auto claim = [&](uint32_t off, uint32_t size, int id) {
        CHECK(off + size <= pl.table_elems);
        for (uint32_t d = 0; d < size; d++) { CHECK(owner[off + d] == -1); owner[off + d] = id; }
    };
    for (uint32_t m = 0; m < pl.windows; m++) claim(pl.off_T[m], 1u << sqrt_window_width(pl, m), (int)m);
    for (uint32_t k = 2; k < pl.windows; k++) {
        if (pl.s % pl.w == 0) {
            CHECK(pl.off_U[k] == pl.off_T[pl.windows - k] && sqrt_row_shift_U(pl, k) == sqrt_row_shift_T(pl, pl.windows - k));
            CHECK(sqrt_window_width(pl, pl.windows - k) == pl.w);
        } else claim(pl.off_U[k], 1u << pl.w, 100 + (int)k);
    }
    for (uint32_t i = 0; i < pl.table_elems; i++) CHECK(owner[i] != -1);
    for (uint32_t j = 0; j < pl.windows; j++)
        for (uint32_t i = 0; i < j; i++) {
            const uint32_t row = sqrt_correction_row(pl, j, i);
            CHECK(row + (1u << pl.w) <= pl.table_elems);
        }
    // the product counts, from the definition of the two forms
    uint32_t wsq = 0;
    for (uint32_t j = 0; j < pl.windows; j++) wsq += pl.s - sqrt_window_lo(pl, j + 1);
    const uint32_t n = pl.windows;
    CHECK(pl.products_chain == pl.root_pow.products + 2 + (pl.s - pl.w) + n * (n - 1) / 2 + n);
    CHECK(pl.products_window == pl.root_pow.products + 2 + wsq + (n - 1) + (n >= 2 ? n - 2 : 0) + n);
    CHECK(pl.products_per_root == (pl.form == SQRT_FORM_CHAIN ? pl.products_chain : pl.products_window));
}

// x^e by a schedule, on the plan's own 256-bit arithmetic: equals the binary method; counts the products
static void check_schedule(const sqrt_schedule &sc, const sqrt_u256 &e, const sqrt_u256 &p) {
    const sqrt_u256 x = sqrt_u256_from(7);
    sqrt_u256 odd[8];
    uint32_t products = 0;
    sqrt_u256 acc = sqrt_u256_from(1);
    if (sc.steps) {
        const sqrt_u256 x2 = sqrt_mulmod(x, x, p);
        odd[1] = x; odd[3] = sqrt_mulmod(x2, x, p); odd[5] = sqrt_mulmod(odd[3], x2, p); odd[7] = sqrt_mulmod(odd[5], x2, p);
        products = 4;
    }
    for (uint32_t k = 0; k < sc.steps; k++) {
        for (uint32_t q = 0; q < sc.sqr[k]; q++) { acc = sqrt_mulmod(acc, acc, p); products++; }
        CHECK(sc.mul[k] == 0 || (sc.mul[k] & 1u));
        CHECK(sc.mul[k] <= 7 && (k || (sc.mul[k] && !sc.sqr[k])));
        if (sc.mul[k]) { if (k) { acc = sqrt_mulmod(acc, odd[sc.mul[k]], p); products++; } else acc = odd[sc.mul[k]]; }
    }
    CHECK(sqrt_u256_eq(acc, sqrt_powmod(x, e, p)) && products == sc.products);
}

// ---- the field of 96769 elements on 64-bit integers
static const uint64_t Q = 96769;
static uint64_t qmul(uint64_t a, uint64_t b) { return a * b % Q; }
static uint64_t qpow(uint64_t a, uint64_t e) { uint64_t r = 1; for (; e; e >>= 1, a = qmul(a, a)) if (e & 1) r = qmul(r, a); return r; }
static uint64_t qpow_schedule(const sqrt_schedule &sc, uint64_t a) {
    if (!sc.steps) return 1;
    const uint64_t a2 = qmul(a, a);
    uint64_t odd[8] = {0, a, 0, qmul(a2, a), 0, 0, 0, 0};
    odd[5] = qmul(odd[3], a2); odd[7] = qmul(odd[5], a2);
    uint64_t acc = 1;
    for (uint32_t k = 0; k < sc.steps; k++) {
        for (uint32_t q = 0; q < sc.sqr[k]; q++) acc = qmul(acc, acc);
        if (sc.mul[k]) acc = k ? qmul(acc, odd[sc.mul[k]]) : odd[sc.mul[k]];
    }
    return acc;
}

struct SmallTables { std::vector<uint64_t> table; std::vector<uint32_t> hash; uint32_t m0, m1; };

static uint32_t small_digit(const sqrt_plan &pl, const SmallTables &t, uint64_t v) {
    const uint32_t h = sqrt_hash((uint32_t)v, 0, t.m0, t.m1);
    return sqrt_hash_lookup(&t.hash[(size_t)(h >> (32 - pl.w)) * SQRT_BUCKET], h, pl.w);
}

// the planned algorithm, form by form: the root x * g^(-e/2) and the parity of e
static uint64_t small_root(const sqrt_plan &pl, const SmallTables &t, uint64_t a, int form, bool *even, uint32_t *products) {
    const uint64_t w0 = qpow_schedule(pl.root_pow, a), x = qmul(a, w0), b = qmul(x, w0);
    uint32_t count = pl.root_pow.products + 2;
    std::vector<uint32_t> e(pl.windows);
    if (form == SQRT_FORM_CHAIN) {
        std::vector<uint64_t> P(pl.windows);
        P[pl.windows - 1] = b;
        for (int j = (int)pl.windows - 2; j >= 0; j--) {
            uint64_t v = P[j + 1];
            for (uint32_t q = 0; q < sqrt_window_width(pl, (uint32_t)j + 1); q++) { v = qmul(v, v); count++; }
            P[j] = v;
        }
        for (uint32_t j = 0; j < pl.windows; j++) {
            uint64_t v = P[j];
            for (uint32_t i = 0; i < j; i++) { v = qmul(v, t.table[sqrt_correction_row(pl, j, i) + e[i]]); count++; }
            e[j] = small_digit(pl, t, v) >> (pl.w - sqrt_window_width(pl, j));
        }
    } else {
        uint64_t acc = 1;
        for (uint32_t j = 0; j < pl.windows; j++) {
            uint64_t v = b;
            if (j) { v = qmul(b, acc); count++; }
            for (uint32_t q = 0; q < pl.s - sqrt_window_lo(pl, j + 1); q++) { v = qmul(v, v); count++; }
            e[j] = small_digit(pl, t, v) >> (pl.w - sqrt_window_width(pl, j));
            if (j + 1 < pl.windows) { if (j) { acc = qmul(acc, t.table[pl.off_T[j] + e[j]]); count++; } else acc = t.table[pl.off_T[0] + e[0]]; }
        }
    }
    uint64_t r = x;
    for (uint32_t m = 0; m < pl.windows; m++) {
        const uint32_t f = sqrt_half_digit(pl, m, e[m], m + 1 < pl.windows ? e[m + 1] : 0);
        CHECK(f < (1u << sqrt_window_width(pl, m)));
        r = qmul(r, t.table[pl.off_T[m] + f]);
        count++;
    }
    *even = !(e[0] & 1u);
    *products = count;
    return r;
}

static void check_small_field() {
    g_what = "every element of the 96769 field";
    const uint32_t p[SQRT_LIMBS] = {(uint32_t)Q, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int64_t> want(Q, -1);                                        // the even root of every square
    for (uint64_t r = 0; r < Q; r++) if (r % 2 == 0) want[qmul(r, r)] = (int64_t)r;
    uint64_t squares = 0;
    for (uint64_t a = 0; a < Q; a++) squares += want[a] >= 0;
    CHECK(squares == 48385);
    for (int form = 0; form < 2; form++) {
        sqrt_plan pl;
        CHECK(sqrt_plan_build(p, form == SQRT_FORM_CHAIN ? SQRT_CHAIN_MAX_WINDOWS : 0, pl) == nullptr);
        CHECK((int)pl.form == form && pl.s == 9 && pl.windows == 2 && pl.last_w == 1 && pl.z == 11);
        const uint64_t g = pl.g.w[0], ginv = qpow(g, Q - 2);
        CHECK(g == qpow(11, (Q - 1) >> 9) && qpow(g, 1u << 8) == Q - 1);
        SmallTables t;
        t.table.assign(pl.table_elems, 0);
        for (uint32_t m = 0; m < pl.windows; m++)
            for (uint32_t d = 0; d < (1u << sqrt_window_width(pl, m)); d++) t.table[pl.off_T[m] + d] = qpow(ginv, (uint64_t)d << sqrt_row_shift_T(pl, m));
        for (uint32_t k = 2; k < pl.windows; k++)
            for (uint32_t d = 0; d < (1u << pl.w); d++) t.table[pl.off_U[k] + d] = qpow(ginv, (uint64_t)d << sqrt_row_shift_U(pl, k));
        const uint64_t h = qpow(g, 1ull << (pl.s - pl.w));
        std::vector<uint32_t> keys(2u << pl.w);
        for (uint32_t d = 0; d < (1u << pl.w); d++) { keys[2 * d] = (uint32_t)qpow(h, d); keys[2 * d + 1] = 0; }
        t.hash.assign((size_t)pl.hash_buckets * SQRT_BUCKET, 0);
        CHECK(sqrt_hash_build((const uint32_t(*)[2])keys.data(), pl.w, &t.m0, &t.m1, t.hash.data()));
        for (uint32_t d = 0; d < (1u << pl.w); d++) CHECK(small_digit(pl, t, keys[2 * d]) == d);
        for (uint64_t a = 0; a < Q; a++) {
            bool even;
            uint32_t products;
            uint64_t r = small_root(pl, t, a, form, &even, &products);
            CHECK(products == pl.products_per_root);
            const bool square = even || a == 0;
            if (r & 1) r = Q - r;
            if (!square) r = 0;
            CHECK(square == (want[a] >= 0));
            CHECK(square ? (int64_t)r == want[a] : r == 0);
            CHECK((a == 0 || qpow_schedule(pl.euler_pow, a) == 1) == square);
        }
    }
}

int main() {
    for (const Case &c : CASES) {
        g_what = c.name;
        for (uint32_t chain_max : {0u, SQRT_CHAIN_MAX_WINDOWS}) {
            sqrt_plan pl;
            const char *why = sqrt_plan_build(c.p, chain_max, pl);
            CHECK(why == nullptr);
            CHECK(pl.s == c.s && pl.z == c.z);
            CHECK(pl.form == (chain_max && pl.windows <= chain_max ? SQRT_FORM_CHAIN : SQRT_FORM_WINDOW));
            sqrt_u256 back = pl.t, one = sqrt_u256_from(1), pm1, e, half;    // 2^s * t + 1 = p, t odd
            CHECK(back.w[0] & 1u);
            for (uint32_t i = 0; i < pl.s; i++) CHECK(sqrt_u256_add(back, back, back) == 0);
            CHECK(sqrt_u256_add(back, back, one) == 0 && sqrt_u256_eq(back, pl.p));
            sqrt_u256_sub(pm1, pl.p, one);
            sqrt_u256 gp = pl.g;                                             // g has order exactly 2^s
            for (uint32_t i = 0; i + 1 < pl.s; i++) gp = sqrt_mulmod(gp, gp, pl.p);
            CHECK(sqrt_u256_eq(gp, pm1));
            check_layout(pl);
            e = pl.t; sqrt_u256_shr1(e);
            half = pm1; sqrt_u256_shr1(half);
            check_schedule(pl.root_pow, e, pl.p);
            check_schedule(pl.euler_pow, half, pl.p);
            CHECK(pl.products_flag == pl.euler_pow.products);
        }
    }
    {
        g_what = "p224";
        sqrt_plan pl;
        CHECK(sqrt_plan_build(CASES[5].p, SQRT_CHAIN_MAX_WINDOWS, pl) == nullptr);
        CHECK(pl.windows == 12 && pl.w == 8 && pl.table_elems == 12 * 256 && pl.form == SQRT_FORM_CHAIN);
        CHECK(pl.products_chain - pl.root_pow.products == 2 + 88 + 66 + 12);
    }
    {
        g_what = "composites";
        sqrt_plan pl;
        const sqrt_u256 odd = sqrt_u256_from(96769ull * 65537ull);
        const char *why = sqrt_plan_build(odd.w, SQRT_CHAIN_MAX_WINDOWS, pl);
        CHECK(why != nullptr && std::string(why) == "modulus is not prime");
        const sqrt_u256 even = sqrt_u256_from(96770), carmichael = sqrt_u256_from(561);
        CHECK(sqrt_plan_build(even.w, 0, pl) != nullptr);
        CHECK(sqrt_plan_build(carmichael.w, 0, pl) != nullptr);
    }
    check_small_field();
    std::printf("sqrt plan OK\n");
    return 0;
}
