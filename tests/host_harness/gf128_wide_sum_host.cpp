// Host-side harness for tests/test_gf128_wide_sum.py: the sum-of-products forms of genstark_amd/csrc/gf128.h (fe_wide_add,
// fe_reduce_wide9) compiled for the host, so the device arithmetic is compared with Python integers without a GPU.  Not part of the product.
#include "../../genstark_amd/csrc/gf128.h"
#include <string.h>
extern "C" {
static fe ld(const uint8_t *p) { fe r; memcpy(&r, p, 16); return r; }
// o[i] = sum_{k < terms} a[terms * i + k] * b[terms * i + k], the 256-bit products added up and reduced once
void h_dot(const uint8_t *a, const uint8_t *b, uint8_t *o, int n, int terms) {
    for (int i = 0; i < n; i++) {
        uint32_t s[8], t[8], top = 0;
        fe_mul_wide(ld(a + 16 * (terms * i)), ld(b + 16 * (terms * i)), s);
        for (int k = 1; k < terms; k++) {
            fe_mul_wide(ld(a + 16 * (terms * i + k)), ld(b + 16 * (terms * i + k)), t);
            fe_wide_add(s, t, top);
        }
        const fe r = fe_reduce_wide9(s, top);
        memcpy(o + 16 * i, &r, 16);
    }
}
// o[i] = (x[i] + top[i] * 2^256) mod p, x[i] any 256-bit value (32 bytes, little endian)
void h_reduce9(const uint8_t *x, const uint32_t *top, uint8_t *o, int n) {
    for (int i = 0; i < n; i++) {
        uint32_t r[8];
        memcpy(r, x + 32 * i, 32);
        const fe v = fe_reduce_wide9(r, top[i]);
        memcpy(o + 16 * i, &v, 16);
    }
}
}
