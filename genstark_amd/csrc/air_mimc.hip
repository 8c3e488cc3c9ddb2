// air_mimc.hip — the air-assembly ProvingContext pieces on the prove() path for the MiMC AIR
// (examples/mimc/mimc128Assembly.ts:28-51): execution trace generation and transition-constraint
// evaluation over the composition domain (lib/Stark.ts:97; lib/components/CompositionPolynomial.ts:76).
#include "common.h"
#include "host_field.h"
#include "../../include/gstark_mimc.h"

#include <atomic>

// q[j] = p[(j + shift) mod nc] - (p[j]^3 + k[j mod klen])
__global__ void k_mimc_constraints(const fe *__restrict__ p, uint64_t nc, uint64_t shift, const fe *__restrict__ k, uint64_t klen,
                                   fe *__restrict__ out) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < nc; j += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t jn = j + shift;
        if (jn >= nc) jn -= nc;
        fe x = p[j], nx = p[jn];
        fe x3 = fe_mul(fe_mul(x, x), x);
        out[j] = fe_sub(nx, fe_add(x3, k[j % klen]));
    }
}

// CompositionPolynomial.evaluateAll for this AIR in ONE pass over the evaluation domain (see include/gstark.h): per point nine field
// products, reads p[i], p[i + E], k, two entries of the domain's table u = 1/(omega^j - 1); everything that depends on x^T only
// (the degree-adjustment factors and 1/(x^T - 1): E distinct values) comes from two E-entry tables built on the host.
#define GS_MIMC_COMP_MAX_PERIOD 32
#define GS_MIMC_COMP_MAX_ROOTS 4
struct MimcCompArgs {
    fe qz[GS_MIMC_COMP_MAX_PERIOD];   // (d0 + d1 * g^(j*qm)) / (g^j - 1),  g = omega^steps
    fe bt[GS_MIMC_COMP_MAX_PERIOD];   // (b0 + b1 * g^(j*bm)) * prod_a omega^-k_a
    fe lt[GS_MIMC_COMP_MAX_PERIOD];   // l0 + l1 * g^(j*bm)   (linear combination with P; zeros when not asked for)
    fe ipoly[GS_MIMC_COMP_MAX_ROOTS];
    uint64_t root[GS_MIMC_COMP_MAX_ROOTS];
    fe x_last;
};
__global__ void k_mimc_composition(const fe *__restrict__ p, uint64_t n, uint64_t shift, const fe *__restrict__ k, uint64_t klen,
                                   const fe *__restrict__ tw_lo, const fe *__restrict__ tw_hi, int log_lo, int logn, const fe *__restrict__ u,
                                   MimcCompArgs a, uint32_t period, uint32_t nroots, int with_lc, fe *__restrict__ out) {
    __shared__ fe qz[GS_MIMC_COMP_MAX_PERIOD], bt[GS_MIMC_COMP_MAX_PERIOD], lt[GS_MIMC_COMP_MAX_PERIOD];
    if (threadIdx.x < period) { qz[threadIdx.x] = a.qz[threadIdx.x]; bt[threadIdx.x] = a.bt[threadIdx.x]; lt[threadIdx.x] = a.lt[threadIdx.x]; }
    __syncthreads();
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        fe x = tw_lo[i & ((1ull << log_lo) - 1)];
        if (logn > log_lo) x = fe_mul(x, tw_hi[i >> log_lo]);
        const fe pi = p[i], pn = p[(i + shift) & (n - 1)];
        const fe q = fe_sub(pn, fe_add(fe_mul(fe_mul(pi, pi), pi), k[i % klen]));                    // transition constraint
        const fe d = fe_mul(fe_mul(q, fe_sub(x, a.x_last)), qz[i & (period - 1)]);                     // Q * adjustment / Z
        fe iv = a.ipoly[nroots - 1];                                                                   // I(x), Horner
        for (int c = (int)nroots - 2; c >= 0; c--) iv = fe_add(fe_mul(iv, x), a.ipoly[c]);
        fe b = fe_mul(fe_sub(pi, iv), bt[i & (period - 1)]);
        for (uint32_t r = 0; r < nroots; r++) b = fe_mul(b, u[(i + n - a.root[r]) & (n - 1)]);         // / prod (x - x_a)
        fe r = fe_add(d, b);
        if (with_lc) r = fe_add(r, fe_mul(pi, lt[i & (period - 1)]));                                 // wave-uniform
        out[i] = r;
    }
}

// The same pass with what depends on neither the trace nor the Fiat-Shamir coefficients taken from three per-point tables
// (gs_mimc_composition_prepare builds them while the host runs the trace recurrence):
//     X[i]  = omega^i - x_last
//     U[i]  = prod_a u[(i - root_a) mod n]                  (0 at the asserted points: the u table's 0^-1 = 0)
//     IU[i] = I(omega^i) * U[i]
// so that B * bt = bt * (p U - IU) — seven field products per point (five reductions in the 128-bit field: mimc_dot), no Horner loop, no loop
// over the roots.  prod_a omega^-k_a stays in bt.
__global__ void k_mimc_table_x(const fe *__restrict__ tw_lo, const fe *__restrict__ tw_hi, int log_lo, int logn, uint64_t n, fe x_last,
                               fe *__restrict__ X) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        fe x = tw_lo[i & ((1ull << log_lo) - 1)];
        if (logn > log_lo) x = fe_mul(x, tw_hi[i >> log_lo]);
        X[i] = fe_sub(x, x_last);
    }
}
struct MimcRoots {
    uint64_t root[GS_MIMC_COMP_MAX_ROOTS];
    fe ipoly[GS_MIMC_COMP_MAX_ROOTS];
};
__global__ void k_mimc_table_u(const fe *__restrict__ u, uint64_t n, MimcRoots a, uint32_t nroots, fe *__restrict__ U) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        fe v = u[(i + n - a.root[0]) & (n - 1)];
        for (uint32_t r = 1; r < nroots; r++) v = fe_mul(v, u[(i + n - a.root[r]) & (n - 1)]);
        U[i] = v;
    }
}
__global__ void k_mimc_table_iu(const fe *__restrict__ X, const fe *__restrict__ U, uint64_t n, MimcRoots a, uint32_t nroots, fe x_last,
                                fe *__restrict__ IU) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const fe x = fe_add(X[i], x_last);
        fe iv = a.ipoly[nroots - 1];                                                                   // I(x), Horner
        for (int c = (int)nroots - 2; c >= 0; c--) iv = fe_add(fe_mul(iv, x), a.ipoly[c]);
        IU[i] = fe_mul(iv, U[i]);
    }
}
// a0 b0 + a1 b1 (+ a2 b2).  In the 128-bit field the 256-bit products are added up and reduced once (gf128.h: a reduction is as many
// operations as the product itself); the other flavours add canonical products.  The same field element either way
__device__ __forceinline__ fe mimc_dot(const fe &a0, const fe &b0, const fe &a1, const fe &b1, const fe &a2, const fe &b2, bool three) {
#ifdef GS_FIELD_128
    uint32_t s[8], t[8], top = 0;
    fe_mul_wide(a0, b0, s);
    fe_mul_wide(a1, b1, t);
    fe_wide_add(s, t, top);
    if (three) {                                                                                       // wave-uniform
        fe_mul_wide(a2, b2, t);
        fe_wide_add(s, t, top);
    }
    return fe_reduce_wide9(s, top);
#else
    const fe r = fe_add(fe_mul(a0, b0), fe_mul(a1, b1));
    return three ? fe_add(r, fe_mul(a2, b2)) : r;
#endif
}
// (of `a`: qz, bt and lt only)
__global__ void k_mimc_composition_tables(const fe *__restrict__ p, uint64_t n, uint64_t shift, const fe *__restrict__ k, uint64_t klen,
                                          const fe *__restrict__ X, const fe *__restrict__ U, const fe *__restrict__ IU, MimcCompArgs a,
                                          uint32_t period, int with_lc, fe *__restrict__ out) {
    __shared__ fe qz[GS_MIMC_COMP_MAX_PERIOD], bt[GS_MIMC_COMP_MAX_PERIOD], lt[GS_MIMC_COMP_MAX_PERIOD];
    if (threadIdx.x < period) { qz[threadIdx.x] = a.qz[threadIdx.x]; bt[threadIdx.x] = a.bt[threadIdx.x]; lt[threadIdx.x] = a.lt[threadIdx.x]; }
    __syncthreads();
    const bool kpow2 = !(klen & (klen - 1));                                                           // no 64-bit division per point then
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const fe pi = p[i], pn = p[(i + shift) & (n - 1)];
        const fe q = fe_sub(pn, fe_add(fe_mul(fe_mul(pi, pi), pi), k[kpow2 ? i & (klen - 1) : i % klen]));   // transition constraint
        const uint32_t j = (uint32_t)i & (period - 1);
        out[i] = mimc_dot(fe_mul(q, X[i]), qz[j], fe_sub(fe_mul(pi, U[i]), IU[i]), bt[j], pi, lt[j], with_lc != 0);
    }
}

// The MiMC recurrence x <- x^3 + k is a serial dependency chain (examples/mimc/utils.ts:7-15): like
// the reference (generated JS over one input) it runs on one host core, here on native 64-bit limbs
// (host_field.h), written straight into a pinned staging buffer that is then copied to the device.
// One chunk of the chain.  Two forms of the same step: the portable one (128-bit temporaries) for any x86-64 / any host, and for cores with
// BMI2 — what MI355X hosts are: EPYC 9005 — the one with mulx products and the carry chains written out by rows, scheduled for Zen 5: 9 % on
// the chain there (tools/trace_bench.cpp, profiles/r05_c_*); picked at run time, never assumed.
#define GS_MIMC_CHUNK_BODY(STEP)                                                                                \
    for (uint64_t i = base; i < end; i++) {                                                                    \
        t[i] = hf_mimc_out(x);                /* the canonical value, beside the chain */                      \
        x = STEP(x, rc[ri]);                  /* the chain itself stays weak (host_field.h) */                 \
        if (++ri == nrc) ri = 0;                                                                               \
    }                                                                                                          \
    *ri_io = ri;                                                                                               \
    return x;
static hfe mimc_chunk_generic(hfe *t, hfe x, const hfe *rc, uint32_t nrc, uint32_t *ri_io, uint64_t base, uint64_t end) {
    uint32_t ri = *ri_io;
    GS_MIMC_CHUNK_BODY(hf_mimc_step_weak)
}
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__) && defined(GS_FIELD_128)
#define GS_MIMC_CHUNK_V3 1
__attribute__((target("arch=x86-64-v3,tune=znver5"))) static hfe mimc_chunk_v3(hfe *t, hfe x, const hfe *rc, uint32_t nrc, uint32_t *ri_io, uint64_t base,
                                                                               uint64_t end) {
    uint32_t ri = *ri_io;
    GS_MIMC_CHUNK_BODY(hf_cube_add_rows)      // mulx + adc chains by rows (host_field.h): 7.3 instead of 8.0 ms per 2^20 steps on the EPYC 9575F
}
#endif

// ---- what gs_mimc_composition and its table-reading form share on the host: the shapes they take, and the per-call kernel arguments
static int mimc_comp_check(gs_ctx *c, uint64_t n, uint64_t steps, uint64_t klen, uint64_t q_inc, uint64_t b_inc, uint32_t nroots) {
    if (!gs_is_pow2(n) || !gs_is_pow2(steps) || steps > n || !klen) return gs_fail(c, GS_ERR_ARG, "mimc_composition: bad sizes");
    if (n / steps > GS_MIMC_COMP_MAX_PERIOD || nroots == 0 || nroots > GS_MIMC_COMP_MAX_ROOTS)
        return gs_fail(c, GS_ERR_UNSUPPORTED, "mimc_composition: n / steps <= %d and 1..%d assertions", GS_MIMC_COMP_MAX_PERIOD, GS_MIMC_COMP_MAX_ROOTS);
    if (q_inc % steps || b_inc % steps) return gs_fail(c, GS_ERR_ARG, "mimc_composition: degree increments must be multiples of the trace length");
    return GS_OK;
}
static fe mimc_x_last(gs_ctx *c, const fe &w, uint64_t n, uint64_t steps) { return gs_memo_pow(c, w, (steps - 1) * (n / steps)); }
static void mimc_comp_args(gs_ctx *c, const fe &w, uint64_t n, uint64_t steps, const uint8_t *coeffs_host, uint64_t q_inc, uint64_t b_inc,
                           const uint8_t *ipoly_host, const uint64_t *root_index_host, uint32_t nroots, const uint8_t *lc_coeffs_host, MimcCompArgs &a) {
    const uint64_t period = n / steps;
    const fe d0 = fe_from_bytes(coeffs_host), d1 = fe_from_bytes(coeffs_host + GS_ELT), b0 = fe_from_bytes(coeffs_host + 2 * GS_ELT),
             b1 = fe_from_bytes(coeffs_host + 3 * GS_ELT);
    const fe l0 = lc_coeffs_host ? fe_from_bytes(lc_coeffs_host) : fe_zero(), l1 = lc_coeffs_host ? fe_from_bytes(lc_coeffs_host + GS_ELT) : fe_zero();
    uint64_t ksum = 0;
    for (uint32_t r = 0; r < GS_MIMC_COMP_MAX_ROOTS; r++) {
        a.root[r] = r < nroots ? root_index_host[r] & (n - 1) : 0;
        a.ipoly[r] = r < nroots ? fe_from_bytes(ipoly_host + GS_ELT * r) : fe_zero();
        if (r < nroots) ksum = (ksum + a.root[r]) & (n - 1);
    }
    const fe scale = gs_memo_pow(c, w, (n - ksum) & (n - 1));                // prod omega^-k_a
    // what depends on the domain and the degrees alone, remembered per context: [3j] 1/(g^j - 1) (j = 0: 0^-1 = 0), [3j+1] g^(j*qm),
    // [3j+2] g^(j*bm) for g = omega^steps (x^steps = g^(i mod period)), then x_last — sixteen inversions of 4 us each otherwise, on the
    // host between the arrival of the evaluation root and this launch
    const std::vector<fe> &tab = gs_memo(c, gs_memo_key("mimc_comp").add(w).add(n).add(steps).add(q_inc).add(b_inc), [&](std::vector<fe> &t) {
        const fe g = fe_pow_u64(w, steps);
        const fe gq = fe_pow_u64(g, (q_inc / steps) % period), gb = fe_pow_u64(g, (b_inc / steps) % period);
        fe gj = fe_one(), gqj = fe_one(), gbj = fe_one();
        for (uint64_t j = 0; j < period; j++) {
            t.push_back(fe_inv(fe_sub(gj, fe_one())));
            t.push_back(gqj);
            t.push_back(gbj);
            gj = fe_mul(gj, g); gqj = fe_mul(gqj, gq); gbj = fe_mul(gbj, gb);
        }
        t.push_back(fe_pow_u64(w, (steps - 1) * period));
    });
    for (uint64_t j = 0; j < GS_MIMC_COMP_MAX_PERIOD; j++) {
        if (j < period) {
            a.qz[j] = fe_mul(fe_add(d0, fe_mul(d1, tab[3 * j + 1])), tab[3 * j]);
            a.bt[j] = fe_mul(fe_add(b0, fe_mul(b1, tab[3 * j + 2])), scale);
            a.lt[j] = fe_add(l0, fe_mul(l1, tab[3 * j + 2]));
        } else {
            a.qz[j] = a.bt[j] = a.lt[j] = fe_zero();
        }
    }
    a.x_last = tab[3 * period];
}

static MimcRoots mimc_roots(uint64_t n, const uint64_t *root_index_host, uint32_t nroots, const uint8_t *ipoly_host) {
    MimcRoots a;
    for (uint32_t r = 0; r < GS_MIMC_COMP_MAX_ROOTS; r++) {
        a.root[r] = r < nroots ? root_index_host[r] & (n - 1) : 0;
        a.ipoly[r] = r < nroots ? fe_from_bytes(ipoly_host + GS_ELT * r) : fe_zero();
    }
    return a;
}
// the keys of the per-point tables: everything each depends on (the tables of a context: common.h)
static std::string mimc_x_key(const fe &w, uint64_t n, uint64_t steps) { return gs_memo_key("X").add(w).add(n).add(steps).k; }
static std::string mimc_u_key(const std::string &x_key, const uint64_t *root, uint32_t nroots) {
    gs_memo_key k("U");
    k.add(x_key.data(), x_key.size()).add((uint64_t)nroots);
    for (uint32_t r = 0; r < nroots; r++) k.add(root[r]);
    return k.k;
}
static std::string mimc_iu_key(const std::string &u_key, const fe *ipoly, uint32_t nroots) {
    gs_memo_key k("IU");
    k.add(u_key.data(), u_key.size());
    for (uint32_t r = 0; r < nroots; r++) k.add(ipoly[r]);
    return k.k;
}
static void mimc_tables_drop(gs_ctx *c) {
    gs_ctx::MimcTables &t = c->mimc_tables;
    gs_free(c, t.X); gs_free(c, t.U); gs_free(c, t.IU);
    t = gs_ctx::MimcTables();
}
// domains above this many points keep the table-free pass: three tables of n elements stop being a fair price (3 GiB per context at 2^26)
#define GS_MIMC_TABLES_MAX_N (1ull << 26)
static std::atomic<uint64_t> g_mimc_tables_max_n{GS_MIMC_TABLES_MAX_N};

extern "C" {

int gs_mimc_trace(gs_ctx *c, const gs_elt *seed, const uint8_t *rc_host, uint32_t nrc, uint64_t steps, void *out) {
    if (!c || !seed || !rc_host || !out) return GS_ERR_ARG;
    if (!nrc || !steps) return gs_fail(c, GS_ERR_ARG, "mimc_trace: empty");
    std::vector<hfe> rc(nrc);
    for (uint32_t i = 0; i < nrc; i++) rc[i] = hf_load(rc_host + GS_ELT * i);
    // pinned, grow-only; waits only for the previous trace's upload, so device work the caller queued before this call
    // (domains, Z(x) inverses, ...) runs while this core grinds through the recurrence
    int rcode = gs_trace_begin(c, steps * GS_ELT);
    if (rcode) return rcode;
    hfe *t = (hfe *)c->h_trace;
    hfe x = hf_load(seed);
    uint32_t ri = 0;
    const uint64_t CHUNK = 1ull << 16;            // copy finished chunks while the next one is being generated
#ifdef GS_MIMC_CHUNK_V3
    static const bool v3 = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("bmi2") && __builtin_cpu_supports("fma");
#else
    const bool v3 = false;
#endif
    for (uint64_t base = 0; base < steps; base += CHUNK) {
        const uint64_t end = base + CHUNK < steps ? base + CHUNK : steps;
#ifdef GS_MIMC_CHUNK_V3
        if (v3) x = mimc_chunk_v3(t, x, rc.data(), nrc, &ri, base, end);
        else
#endif
            x = mimc_chunk_generic(t, x, rc.data(), nrc, &ri, base, end);
        (void)v3;
        GS_HIP(c, hipMemcpyAsync((uint8_t *)out + base * GS_ELT, t + base, (end - base) * GS_ELT, hipMemcpyHostToDevice, c->stream));
    }
    return gs_trace_end(c);   // no synchronisation: consumers are ordered on the stream
}

int gs_mimc_constraints(gs_ctx *c, const void *p_comp, uint64_t nc, uint64_t shift, const void *k_table, uint64_t klen, void *out) {
    if (!c || !p_comp || !k_table || !out) return GS_ERR_ARG;
    if (!nc || !klen) return gs_fail(c, GS_ERR_ARG, "mimc_constraints: empty");
    hipLaunchKernelGGL(k_mimc_constraints, dim3(gs_grid(nc)), dim3(256), 0, c->stream, (const fe *)p_comp, nc, shift % nc,
                       (const fe *)k_table, klen, (fe *)out);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int gs_mimc_composition(gs_ctx *c, const void *p_eval, uint64_t n, uint64_t steps, const gs_elt *omega, const void *k_table, uint64_t klen,
                        const uint8_t *coeffs_host, uint64_t q_inc, uint64_t b_inc, const uint8_t *ipoly_host, const uint64_t *root_index_host,
                        uint32_t nroots, const uint8_t *lc_coeffs_host, void *out) {
    if (!c || !p_eval || !omega || !k_table || !coeffs_host || !ipoly_host || !root_index_host || !out) return GS_ERR_ARG;
    int rc = mimc_comp_check(c, n, steps, klen, q_inc, b_inc, nroots);
    if (rc) return rc;
    const fe w = fe_from_bytes(omega);
    const uint64_t period = n / steps;
    const fe *lo, *hi, *u;
    int log_lo;
    rc = gs_plan_pow_tables(c, w, n, &lo, &hi, &log_lo);
    if (!rc) rc = gs_plan_inverse_table(c, w, n, &u);
    if (rc) return rc;
    MimcCompArgs a;
    mimc_comp_args(c, w, n, steps, coeffs_host, q_inc, b_inc, ipoly_host, root_index_host, nroots, lc_coeffs_host, a);
    gs_traffic(c, 2 * n * GS_ELT, n, "k_mimc_composition");      // P over the evaluation domain in (its neighbour P(x g) is the same vector), L out
    hipLaunchKernelGGL(k_mimc_composition, dim3(gs_grid(n)), dim3(256), 0, c->stream, (const fe *)p_eval, n, period, (const fe *)k_table, klen, lo, hi,
                       log_lo, gs_log2(n), u, a, (uint32_t)period, nroots, lc_coeffs_host ? 1 : 0, (fe *)out);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

uint64_t gs_mimc_composition_tables_max_n(uint64_t max_n) {
    return g_mimc_tables_max_n.exchange(max_n && max_n < GS_MIMC_TABLES_MAX_N ? max_n : GS_MIMC_TABLES_MAX_N);
}

int gs_mimc_composition_prepare(gs_ctx *c, uint64_t n, uint64_t steps, const gs_elt *omega, const uint64_t *root_index_host, uint32_t nroots,
                                const uint8_t *ipoly_host) {
    if (!c || !omega || !root_index_host || !ipoly_host) return GS_ERR_ARG;
    int rc = mimc_comp_check(c, n, steps, 1, 0, 0, nroots);
    if (rc) return rc;
    gs_ctx::MimcTables &t = c->mimc_tables;
    t.iu_key.clear();                                             // whatever happens below, the last proof's IU no longer counts
    if (n > g_mimc_tables_max_n.load()) { mimc_tables_drop(c); return GS_OK; }
    const fe w = fe_from_bytes(omega);
    const fe *lo, *hi, *u;
    int log_lo;
    rc = gs_plan_pow_tables(c, w, n, &lo, &hi, &log_lo);
    if (!rc) rc = gs_plan_inverse_table(c, w, n, &u);
    if (rc) return rc;
    if (t.n != n) {
        mimc_tables_drop(c);
        void *q[3] = {nullptr, nullptr, nullptr};
        for (int i = 0; i < 3 && !rc; i++) rc = gs_alloc(c, n * GS_ELT, &q[i]);
        if (rc) {                                                 // no room for them: the table-free pass answers (gs_mimc_composition_tables)
            for (int i = 0; i < 3; i++) gs_free(c, q[i]);
            return GS_OK;
        }
        t.X = (fe *)q[0]; t.U = (fe *)q[1]; t.IU = (fe *)q[2];
        t.n = n;
    }
    const MimcRoots a = mimc_roots(n, root_index_host, nroots, ipoly_host);
    const fe x_last = mimc_x_last(c, w, n, steps);
    const dim3 grid(gs_grid(n)), block(256);
    const std::string x_key = mimc_x_key(w, n, steps), u_key = mimc_u_key(x_key, a.root, nroots);
    const bool make_x = t.x_key != x_key, make_u = t.u_key != u_key;
    if (make_x) {
        t.x_key.clear();
        gs_traffic(c, n * GS_ELT, n, "k_mimc_table_x");
        hipLaunchKernelGGL(k_mimc_table_x, grid, block, 0, c->stream, lo, hi, log_lo, gs_log2(n), n, x_last, t.X);
    }
    if (make_u) {
        t.u_key.clear();
        gs_traffic(c, 2 * n * GS_ELT, n * (nroots - 1), "k_mimc_table_u");      // the u table in (every look-up is a shift of it), U out
        hipLaunchKernelGGL(k_mimc_table_u, grid, block, 0, c->stream, u, n, a, nroots, t.U);
    }
    gs_traffic(c, 3 * n * GS_ELT, n * nroots, "k_mimc_table_iu");                // X and U in, IU out
    hipLaunchKernelGGL(k_mimc_table_iu, grid, block, 0, c->stream, t.X, t.U, n, a, nroots, x_last, t.IU);
    GS_LAUNCH_CHECK(c);
    t.x_key = x_key;
    t.u_key = u_key;
    t.iu_key = mimc_iu_key(u_key, a.ipoly, nroots);
    return GS_OK;
}

int gs_mimc_composition_tables(gs_ctx *c, const void *p_eval, uint64_t n, uint64_t steps, const gs_elt *omega, const void *k_table, uint64_t klen,
                               const uint8_t *coeffs_host, uint64_t q_inc, uint64_t b_inc, const uint8_t *ipoly_host, const uint64_t *root_index_host,
                               uint32_t nroots, const uint8_t *lc_coeffs_host, void *out) {
    if (!c || !p_eval || !omega || !k_table || !coeffs_host || !ipoly_host || !root_index_host || !out) return GS_ERR_ARG;
    int rc = mimc_comp_check(c, n, steps, klen, q_inc, b_inc, nroots);
    if (rc) return rc;
    const fe w = fe_from_bytes(omega);
    const gs_ctx::MimcTables &t = c->mimc_tables;
    const MimcRoots ra = mimc_roots(n, root_index_host, nroots, ipoly_host);
    // the tables of exactly this statement, or the table-free pass: same values
    if (t.iu_key.empty() || t.n != n || t.iu_key != mimc_iu_key(mimc_u_key(mimc_x_key(w, n, steps), ra.root, nroots), ra.ipoly, nroots))
        return gs_mimc_composition(c, p_eval, n, steps, omega, k_table, klen, coeffs_host, q_inc, b_inc, ipoly_host, root_index_host, nroots,
                                   lc_coeffs_host, out);
    MimcCompArgs a;
    mimc_comp_args(c, w, n, steps, coeffs_host, q_inc, b_inc, ipoly_host, root_index_host, nroots, lc_coeffs_host, a);
    const uint64_t period = n / steps;
    gs_traffic(c, 5 * n * GS_ELT, n, "k_mimc_composition_tables");      // P and the three tables in, L out
    hipLaunchKernelGGL(k_mimc_composition_tables, dim3(gs_grid(n)), dim3(256), 0, c->stream, (const fe *)p_eval, n, period, (const fe *)k_table, klen,
                       t.X, t.U, t.IU, a, (uint32_t)period, lc_coeffs_host ? 1 : 0, (fe *)out);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

}  // extern "C"
