// sqrt_plan.h — how a modular square root (gs_field_sqrt, include/gstark_sqrt.h) is scheduled for ONE modulus: the split p - 1 = 2^s * t,
// the non-residue z and g = z^t (a generator of the 2-Sylow subgroup), the windows of the discrete logarithm in that subgroup, the offsets
// of its tables, the fixed schedules of the two exponentiations and the exact product count of every form (sqrt.hip is the device side;
// DESIGN.md "Square roots" has the argument).  Plain C++, no HIP and no field header: the modulus arrives as eight 32-bit limbs and the
// few hundred products of the search for z run on the bit-serial arithmetic below; it is tested on its own
// (tests/host_harness/sqrt_plan_host.cpp).  Nothing here depends on the VALUES whose roots are taken.
//   the root      w0 = a^((t-1)/2), x = a * w0, b = x * w0 = a^t = g^e with 0 <= e < 2^s; a is a square exactly when e is even (or a = 0),
//                 and then x * g^(-e/2) is a root.
//   windows       e is cut into `windows` digits of w = min(8, s) bits from the low end; the LAST window may be narrower.  Window j covers
//                 bits [lo_j, lo_{j+1}).  With every lower digit known, b^(2^(s - lo_{j+1})) times one table entry per lower digit is
//                 h^(e_j * 2^(w - w_j)), h = g^(2^(s-w)) of order 2^w, and a hash of that element's two low limbs finds the digit.
//   chain form    the powers P_j = b^(2^(s - lo_{j+1})) are computed ONCE (s - w squarings, all kept); window j multiplies P_j by
//                 U[j+1-i][e_i] for i < j, U[k][d] = g^(-d * 2^(s - k*w)) (the last window by T[i][e_i]): windows*(windows-1)/2 products.
//   window form   acc = g^(-(e mod 2^lo_j)) is kept instead of the powers: window j squares b * acc (s - lo_{j+1}) times.
//   tables        T[m][d] = g^(-d * 2^lo_m), d < 2^w_m.  U[k] is T[windows-k] when w divides s, rows of its own otherwise.  The root's
//                 g^(-e/2) is the product of T[m][f_m] over the digits f_m of e >> 1, which are shifts of the e_m: no table of its own.
#pragma once
#include <cstdint>
#include <cstring>

#define SQRT_MAX_COUNT (1ull << 20)          // roots per call
#define SQRT_LIMBS 8u                        // 32-bit limbs of a modulus (below 2^256)
#define SQRT_WINDOW_BITS 8u
#define SQRT_MAX_WINDOWS 32u                 // s <= 255
#define SQRT_MAX_STEPS 192u                  // steps of one exponentiation schedule (a 256-bit exponent has at most 128 windows)
#define SQRT_BUCKET 4u                       // entries per bucket of the digit hash: one 16-byte load
#define SQRT_HASH_EMPTY 0xffffffffu
#define SQRT_CANDIDATES_BELOW 1000u          // z is searched below this
#define SQRT_CHAIN_MAX_WINDOWS 12u           // the chain form keeps `windows` elements per lane: up to here they stay in registers

enum { SQRT_FORM_CHAIN = 0, SQRT_FORM_WINDOW = 1 };

// ---- 256-bit integers for the plan's own few products (bit-serial: a product is 256 doublings; nothing here is on a hot path)
struct sqrt_u256 { uint32_t w[SQRT_LIMBS]; };
static inline sqrt_u256 sqrt_u256_from(uint64_t v) { sqrt_u256 r = {}; r.w[0] = (uint32_t)v; r.w[1] = (uint32_t)(v >> 32); return r; }
static inline bool sqrt_u256_is_zero(const sqrt_u256 &a) { uint32_t o = 0; for (uint32_t i = 0; i < SQRT_LIMBS; i++) o |= a.w[i]; return o == 0; }
static inline bool sqrt_u256_eq(const sqrt_u256 &a, const sqrt_u256 &b) { return memcmp(a.w, b.w, sizeof a.w) == 0; }
static inline int sqrt_u256_cmp(const sqrt_u256 &a, const sqrt_u256 &b) {
    for (int i = (int)SQRT_LIMBS - 1; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}
static inline uint32_t sqrt_u256_add(sqrt_u256 &r, const sqrt_u256 &a, const sqrt_u256 &b) {      // returns the carry
    uint64_t c = 0;
    for (uint32_t i = 0; i < SQRT_LIMBS; i++) { c += (uint64_t)a.w[i] + b.w[i]; r.w[i] = (uint32_t)c; c >>= 32; }
    return (uint32_t)c;
}
static inline uint32_t sqrt_u256_sub(sqrt_u256 &r, const sqrt_u256 &a, const sqrt_u256 &b) {      // returns the borrow
    uint64_t br = 0;
    for (uint32_t i = 0; i < SQRT_LIMBS; i++) { const uint64_t d = (uint64_t)a.w[i] - b.w[i] - br; r.w[i] = (uint32_t)d; br = (d >> 32) & 1u; }
    return (uint32_t)br;
}
static inline void sqrt_u256_shr1(sqrt_u256 &a) {
    for (uint32_t i = 0; i < SQRT_LIMBS; i++) a.w[i] = (a.w[i] >> 1) | (i + 1 < SQRT_LIMBS ? a.w[i + 1] << 31 : 0u);
}
static inline uint32_t sqrt_u256_bit(const sqrt_u256 &a, uint32_t i) { return (a.w[i >> 5] >> (i & 31)) & 1u; }
static inline uint32_t sqrt_u256_bits(const sqrt_u256 &a) {                                         // position of the top bit + 1
    for (int i = 255; i >= 0; i--) if (sqrt_u256_bit(a, (uint32_t)i)) return (uint32_t)i + 1;
    return 0;
}
static inline sqrt_u256 sqrt_addmod(const sqrt_u256 &a, const sqrt_u256 &b, const sqrt_u256 &p) {  // a, b < p
    sqrt_u256 s, d;
    const uint32_t carry = sqrt_u256_add(s, a, b);
    const uint32_t borrow = sqrt_u256_sub(d, s, p);
    return carry || !borrow ? d : s;
}
static inline sqrt_u256 sqrt_mulmod(const sqrt_u256 &a, const sqrt_u256 &b, const sqrt_u256 &p) {  // a, b < p
    sqrt_u256 r = {};
    for (int i = (int)sqrt_u256_bits(b) - 1; i >= 0; i--) {
        r = sqrt_addmod(r, r, p);
        if (sqrt_u256_bit(b, (uint32_t)i)) r = sqrt_addmod(r, a, p);
    }
    return r;
}
static inline sqrt_u256 sqrt_powmod(const sqrt_u256 &a, const sqrt_u256 &e, const sqrt_u256 &p) {
    sqrt_u256 r = sqrt_u256_from(1);
    for (int i = (int)sqrt_u256_bits(e) - 1; i >= 0; i--) {
        r = sqrt_mulmod(r, r, p);
        if (sqrt_u256_bit(e, (uint32_t)i)) r = sqrt_mulmod(r, a, p);
    }
    return r;
}

// ---- a fixed schedule for x -> x^e: sliding windows of three bits over e from the top.  Step k is `sqr` squarings, then a product by
// x^mul (mul = 1, 3, 5, 7; 0: none).  The first step's product is an assignment (no squarings before it).  e = 0: no steps, the value 1.
struct sqrt_schedule {
    uint32_t steps = 0;
    uint16_t sqr[SQRT_MAX_STEPS] = {0}, mul[SQRT_MAX_STEPS] = {0};
    uint32_t products = 0;                   // 4 for x^2, x^3, x^5, x^7, every squaring, every product but the first
};
static inline bool sqrt_schedule_build(const sqrt_u256 &e, sqrt_schedule &sc) {
    sc = sqrt_schedule();
    int i = (int)sqrt_u256_bits(e) - 1;
    if (i < 0) return true;
    uint32_t pending = 0;
    while (i >= 0) {
        if (!sqrt_u256_bit(e, (uint32_t)i)) { pending++; i--; continue; }
        int len = i >= 2 ? 3 : i + 1;                                        // the longest window of at most 3 bits that ends in a one
        while (!sqrt_u256_bit(e, (uint32_t)(i - len + 1))) len--;
        uint32_t v = 0;
        for (int k = 0; k < len; k++) v = (v << 1) | sqrt_u256_bit(e, (uint32_t)(i - k));
        if (sc.steps >= SQRT_MAX_STEPS) return false;
        sc.sqr[sc.steps] = (uint16_t)(sc.steps ? pending + (uint32_t)len : 0);
        sc.mul[sc.steps] = (uint16_t)v;
        sc.steps++;
        pending = 0;
        i -= len;
    }
    if (pending) {
        if (sc.steps >= SQRT_MAX_STEPS) return false;
        sc.sqr[sc.steps] = (uint16_t)pending; sc.mul[sc.steps] = 0; sc.steps++;
    }
    sc.products = 4;
    for (uint32_t k = 0; k < sc.steps; k++) sc.products += sc.sqr[k] + (k && sc.mul[k] ? 1u : 0u);
    return true;
}

struct sqrt_plan {
    sqrt_u256 p = {}, t = {}, g = {};        // the modulus, the odd part of p - 1, z^t
    uint32_t s = 0, z = 0;                   // p - 1 = 2^s * t; the smallest z >= 2 with z^((p-1)/2) = -1
    uint32_t w = 0, windows = 0, last_w = 0; // window width min(8, s), ceil(s / w), the width of the last window
    uint32_t form = SQRT_FORM_CHAIN;
    uint32_t off_T[SQRT_MAX_WINDOWS] = {0};  // element offsets of the rows T[m]
    uint32_t off_U[SQRT_MAX_WINDOWS + 1] = {0};   // ... and of U[k], 2 <= k < windows (chain form)
    uint32_t table_elems = 0;                // elements of all rows
    uint32_t hash_buckets = 0;               // 2^w buckets of SQRT_BUCKET entries
    sqrt_schedule root_pow, euler_pow;       // x^((t-1)/2) and x^((p-1)/2)
    uint32_t products_chain = 0, products_window = 0;     // per root, both forms
    uint32_t products_per_root = 0;          // ... of `form`
    uint32_t products_flag = 0;              // Euler's criterion
};

static inline uint32_t sqrt_window_lo(const sqrt_plan &pl, uint32_t j) { return j < pl.windows ? j * pl.w : pl.s; }
static inline uint32_t sqrt_window_width(const sqrt_plan &pl, uint32_t j) { return sqrt_window_lo(pl, j + 1) - sqrt_window_lo(pl, j); }
// the row that corrects window j for the digit of window i < j
static inline uint32_t sqrt_correction_row(const sqrt_plan &pl, uint32_t j, uint32_t i) { return j + 1 == pl.windows ? pl.off_T[i] : pl.off_U[j + 1 - i]; }
// the exponent k of g^(-d * 2^k) that a row holds (the harness and the table builder walk the same numbers)
static inline uint32_t sqrt_row_shift_T(const sqrt_plan &pl, uint32_t m) { return sqrt_window_lo(pl, m); }
static inline uint32_t sqrt_row_shift_U(const sqrt_plan &pl, uint32_t k) { return pl.s - k * pl.w; }
// digit m of e >> 1 from the digits of e (the root's own digits)
static inline uint32_t sqrt_half_digit(const sqrt_plan &pl, uint32_t m, uint32_t e_m, uint32_t e_next) {
    return (e_m >> 1) | (m + 1 < pl.windows ? (e_next & 1u) << (sqrt_window_width(pl, m) - 1) : 0u);
}

// Fills `pl` for the modulus `p` (eight limbs, little endian); chain_max_windows: the most windows the caller's chain form takes (0: the
// window form always).  Returns nullptr, or the reason the modulus is refused.
static inline const char *sqrt_plan_build(const uint32_t p_limbs[SQRT_LIMBS], uint32_t chain_max_windows, sqrt_plan &pl) {
    pl = sqrt_plan();
    memcpy(pl.p.w, p_limbs, sizeof pl.p.w);
    const sqrt_u256 one = sqrt_u256_from(1);
    if (!(pl.p.w[0] & 1u) || sqrt_u256_cmp(pl.p, sqrt_u256_from(3)) < 0) return "modulus is not prime";
    sqrt_u256 pm1, half;
    sqrt_u256_sub(pm1, pl.p, one);
    pl.t = pm1;
    while (!(pl.t.w[0] & 1u)) { sqrt_u256_shr1(pl.t); pl.s++; }
    half = pm1;
    sqrt_u256_shr1(half);
    for (uint32_t z = 2; z < SQRT_CANDIDATES_BELOW && !pl.z; z++) {
        const sqrt_u256 zz = sqrt_u256_from(z);
        if (sqrt_u256_cmp(zz, pl.p) >= 0) break;
        const sqrt_u256 euler = sqrt_powmod(zz, half, pl.p);
        if (sqrt_u256_eq(euler, pm1)) pl.z = z;
        else if (!sqrt_u256_eq(euler, one)) return "modulus is not prime";
    }
    if (!pl.z) return "modulus is not prime";                                // (or no non-residue below 1000: no prime below 2^256 is known to lack one)
    pl.g = sqrt_powmod(sqrt_u256_from(pl.z), pl.t, pl.p);
    pl.w = pl.s < SQRT_WINDOW_BITS ? pl.s : SQRT_WINDOW_BITS;
    pl.windows = (pl.s + pl.w - 1) / pl.w;
    pl.last_w = pl.s - (pl.windows - 1) * pl.w;
    pl.hash_buckets = 1u << pl.w;
    pl.form = pl.windows <= chain_max_windows ? SQRT_FORM_CHAIN : SQRT_FORM_WINDOW;
    uint32_t at = 0;
    for (uint32_t m = 0; m < pl.windows; m++) { pl.off_T[m] = at; at += 1u << sqrt_window_width(pl, m); }
    for (uint32_t k = 2; k < pl.windows; k++) {
        if (pl.s % pl.w == 0) pl.off_U[k] = pl.off_T[pl.windows - k];
        else { pl.off_U[k] = at; at += 1u << pl.w; }
    }
    pl.table_elems = at;
    sqrt_u256 e = pl.t;                                                      // (t - 1) / 2: t is odd
    sqrt_u256_shr1(e);
    if (!sqrt_schedule_build(e, pl.root_pow) || !sqrt_schedule_build(half, pl.euler_pow)) return "modulus is not prime";
    // x and b (2), the digits, one product per window for g^(-e/2)
    const uint32_t n = pl.windows;
    uint32_t window_squarings = 0;
    for (uint32_t j = 0; j < n; j++) window_squarings += pl.s - sqrt_window_lo(pl, j + 1);
    pl.products_chain = pl.root_pow.products + 2 + (pl.s - pl.w) + n * (n - 1) / 2 + n;
    pl.products_window = pl.root_pow.products + 2 + window_squarings + (n - 1) + (n >= 2 ? n - 2 : 0) + n;
    pl.products_per_root = pl.form == SQRT_FORM_CHAIN ? pl.products_chain : pl.products_window;
    pl.products_flag = pl.euler_pow.products;
    return nullptr;
}

// ---- the digit hash: from an element of the subgroup of order 2^w (its two low limbs) to its exponent.  hash = l0 * m0 + l1 * m1;
// the top w bits pick a bucket of SQRT_BUCKET entries, an entry is the hash's other bits above the digit: (hash << w) | digit.
#if defined(__HIPCC__)
#define SQRT_HD __host__ __device__ static inline
#else
#define SQRT_HD static inline
#endif
SQRT_HD uint32_t sqrt_hash(uint32_t l0, uint32_t l1, uint32_t m0, uint32_t m1) { return l0 * m0 + l1 * m1; }
static inline uint32_t sqrt_hash_lookup(const uint32_t *bucket, uint32_t hash, uint32_t w) {        // what the kernel does, with selects
    uint32_t d = 0;
    for (uint32_t k = 0; k < SQRT_BUCKET; k++)
        if (bucket[k] != SQRT_HASH_EMPTY && (bucket[k] >> w) == ((hash << w) >> w)) d = bucket[k] & ((1u << w) - 1);
    return d;
}
// keys: the two low limbs of h^d for d < 2^w; entries: 2^w * SQRT_BUCKET words.  false: no multiplier pair was found (the keys repeat)
static inline bool sqrt_hash_build(const uint32_t (*keys)[2], uint32_t w, uint32_t *m0_out, uint32_t *m1_out, uint32_t *entries) {
    const uint32_t n = 1u << w;
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    for (uint32_t attempt = 0; attempt < 4096; attempt++) {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t m0 = (uint32_t)(rng >> 32) | 1u, m1 = (uint32_t)(rng >> 11) | 1u;
        for (uint32_t i = 0; i < n * SQRT_BUCKET; i++) entries[i] = SQRT_HASH_EMPTY;
        bool ok = true;
        for (uint32_t d = 0; d < n && ok; d++) {
            const uint32_t h = sqrt_hash(keys[d][0], keys[d][1], m0, m1), entry = (h << w) | d;
            uint32_t *bucket = entries + (size_t)(h >> (32 - w)) * SQRT_BUCKET;
            uint32_t k = 0;
            while (k < SQRT_BUCKET && bucket[k] != SQRT_HASH_EMPTY && (bucket[k] >> w) != (entry >> w)) k++;
            if (k == SQRT_BUCKET || bucket[k] != SQRT_HASH_EMPTY || entry == SQRT_HASH_EMPTY) ok = false;     // full, the same tag twice, or the empty mark
            else bucket[k] = entry;
        }
        if (ok) { *m0_out = m0; *m1_out = m1; return true; }
    }
    return false;
}
