// host_poly.h — the polynomial helpers of the HOST side, written once over host_field.h's interface (include after host_field.h):
// the radix-2 transform, batch inversion, the product of linear factors and Horner evaluation that small.hip (gs_small_interpolate),
// the native drivers (prover.cc: Plan::zero_poly, the remainder check) and the verifier (verifier.h: cyclic_poly, the boundary forms)
// compute with.  Plain C++: no HIP, no ABI calls; tools/host_poly_check.cpp builds it stand-alone.
//
// Representatives (they differ in the 128-bit flavour only, host_field.h): == / != and hf_is_zero are meaningful on CANONICAL values
// alone, so every helper says what it takes and every helper RETURNS canonical values.  Inside, long chains run on the weak operations
// and are canonicalised once at their end.
#pragma once
#include <stddef.h>

#include <utility>
#include <vector>

// a canonical product through the weak form: no data-dependent reduction loops where the field has one (any representatives in)
static inline hfe hp_mul(hfe a, hfe b) { return hf_canon(hf_mul_weak(a, b)); }

// In place: a[j] <- sum_i a[i] w^(i j), w of order a.size() (a power of two; a single value is its own transform).  Decimation in
// time over a bit-reversed copy, one table of the n/2 powers of w read at the stage's stride.  The inverse is the transform with w^-1
// and a scale by 1/n, which is the caller's (the remainder check compares unscaled coefficients).
// in: any representatives (w canonical); out: canonical
static inline void host_transform(std::vector<hfe> &a, hfe w) {
    const size_t n = a.size();
    uint32_t lg = 0;
    while (((size_t)1 << lg) < n) lg++;
    for (size_t i = 0; i < n; i++) {
        size_t r = 0;
        for (uint32_t b = 0; b < lg; b++) r |= ((i >> b) & 1) << (lg - 1 - b);
        if (i < r) std::swap(a[i], a[r]);
    }
    for (hfe &v : a) v = hf_canon(v);                    // (the butterflies' sums and differences take canonical operands)
    std::vector<hfe> tw(n / 2 ? n / 2 : 1);
    hfe cur = 1;
    for (size_t k = 0; k < n / 2; k++) { tw[k] = cur; cur = hf_mul(cur, w); }
    for (size_t half = 1; half < n; half <<= 1) {
        const size_t stride = n / (2 * half);
        for (size_t base = 0; base < n; base += 2 * half)
            for (size_t k = 0; k < half; k++) {
                const hfe u = a[base + k], v = hp_mul(a[base + k + half], tw[k * stride]);
                a[base + k] = hf_add(u, v);
                a[base + k + half] = hf_sub(u, v);
            }
    }
}

// v[i] <- 1 / v[i] for all n with ONE field inversion (Montgomery's trick); 0 stays 0 (galois' convention).
// in: canonical (a zero is recognised by hf_is_zero); out: canonical
static inline void host_batch_invert(hfe *v, size_t n) {
    std::vector<hfe> pre(n);
    hfe acc = 1;
    for (size_t i = 0; i < n; i++) { pre[i] = acc; if (!hf_is_zero(v[i])) acc = hf_mul(acc, v[i]); }
    hfe inv = hf_inv(acc);
    for (size_t i = n; i-- > 0;) {
        if (hf_is_zero(v[i])) continue;
        const hfe vi = v[i];
        v[i] = hf_mul(inv, pre[i]);
        inv = hf_mul(inv, vi);
    }
}
static inline void host_batch_invert(std::vector<hfe> &v) { host_batch_invert(v.data(), v.size()); }

// zp[0 .. m] <- the coefficients, lowest first, of the monic product of (X - xs[i]) over i < m (m = 0: the constant 1).  Multiplied
// out in place, one factor at a time: m^2 / 2 products.
// in: canonical (each point is negated); out: canonical
static inline void host_linear_product(const hfe *xs, size_t m, hfe *zp) {
    zp[0] = 1;
    for (size_t i = 0; i < m; i++) {
        const hfe nx = hf_sub(0, xs[i]);
        zp[i + 1] = 0;
        for (size_t d = i + 1; d >= 1; d--) zp[d] = hf_add_weak(zp[d - 1], hf_mul_weak(zp[d], nx));
        zp[0] = hf_mul_weak(zp[0], nx);
    }
    for (size_t d = 0; d <= m; d++) zp[d] = hf_canon(zp[d]);
}
static inline std::vector<hfe> host_linear_product(const std::vector<hfe> &xs) {
    std::vector<hfe> zp(xs.size() + 1);
    host_linear_product(xs.data(), xs.size(), zp.data());
    return zp;
}

// FiniteField.evalPolyAt, on host scalars (an empty polynomial is 0).  in: canonical; out: canonical
static inline hfe horner(const std::vector<hfe> &poly, hfe x) {
    hfe r = 0;
    for (size_t k = poly.size(); k-- > 0;) r = hf_add(hf_mul(r, x), poly[k]);
    return r;
}
// one polynomial at many points: the coefficient loop outside, so that the points' chains are independent work for the core (a public
// input register of an air-assembly component is a polynomial as long as the trace, and one serial chain per query is what verifying costs)
// in: any representatives; out: canonical
static inline std::vector<hfe> horner_many(const std::vector<hfe> &poly, const std::vector<hfe> &xs) {
    std::vector<hfe> r(xs.size(), (hfe)0);
    for (size_t k = poly.size(); k-- > 0;) {
        const hfe c = poly[k];
        for (size_t q = 0; q < xs.size(); q++) r[q] = hf_add_weak(hf_mul_weak(r[q], xs[q]), c);      // weak values inside the chain
    }
    for (hfe &v : r) v = hf_canon(v);
    return r;
}
