// Host-side harness for tests/test_field_corners.py: the field arithmetic of one build flavour — the device header (gf128.h, gf_small.h,
// gf_wide.h) as it compiles for the host, the faster host product under the native driver and the verifier (host_field*.h) and, in the
// 128-bit flavour, the lazy-limb products of gf128_lazy.h — as a filter, so that operands chosen to take the rare carries of each
// reduction (tests/field_corners.py) are compared with Python integers on a machine without a GPU.  Not part of the product.
// Build: g++ -O2 [-DGS_WIDE_BITS=256|224|0 | -DGS_SMALL_Q=<q>ull] tests/host_harness/field_corners_host.cpp
// Run:   field_corners_host [modulus, 64 hex digits: the runtime flavour, GS_WIDE_BITS=0]
// stdin: lines "op a b" (64 hex digits each, big endian); stdout: one result per line (hex), "?" for an op this flavour does not have.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#if defined(GS_WIDE_BITS)
#include "../../genstark_amd/csrc/gf_wide.h"
#elif defined(GS_SMALL_Q)
#include "../../genstark_amd/csrc/gf_small.h"
#else
#include "../../genstark_amd/csrc/gf128_lazy.h"
#endif
#include "../../genstark_amd/csrc/host_field.h"

#define NB 32                                  // bytes of the widest element

static void parse(const char *h, uint8_t b[NB]) {
    const size_t n = strlen(h);
    for (int i = 0; i < NB; i++) {
        unsigned v = 0;
        if (n >= 2 * (size_t)(i + 1)) sscanf(h + n - 2 * (i + 1), "%2x", &v);
        b[i] = (uint8_t)v;
    }
}
static fe to_fe(const uint8_t b[NB]) { fe r; memcpy(&r, b, sizeof(fe)); return r; }
static void show_bytes(const uint8_t *b, int n) {
    for (int i = n - 1; i >= 0; i--) printf("%02x", b[i]);
    printf("\n");
}
static void show(const fe &x) { uint8_t b[sizeof(fe)]; memcpy(b, &x, sizeof(fe)); show_bytes(b, (int)sizeof(fe)); }
static void showh(hfe x) { uint8_t b[HF_ELT]; hf_store(b, x); show_bytes(b, HF_ELT); }

int main(int argc, char **argv) {
#if defined(GS_WIDE_BITS) && GS_WIDE_BITS == 0
    if (argc < 2) { fprintf(stderr, "the runtime flavour takes its modulus (hex) as the first argument\n"); return 2; }
    uint8_t pb[NB];
    uint32_t pl[GF_LIMBS];
    parse(argv[1], pb);
    memcpy(pl, pb, sizeof(pl));
    if (gf_rt_configure(pl) != 0) { fprintf(stderr, "modulus refused\n"); return 2; }
#else
    (void)argc; (void)argv;
#endif
    static char op[32], sa[80], sb[80];
    while (scanf("%31s %64s %64s", op, sa, sb) == 3) {
        uint8_t ba[NB], bb[NB];
        parse(sa, ba);
        parse(sb, bb);
        const fe a = to_fe(ba), b = to_fe(bb);
        const hfe x = hf_load(ba), y = hf_load(bb);
        if (!strcmp(op, "add")) show(fe_add(a, b));
        else if (!strcmp(op, "sub")) show(fe_sub(a, b));
        else if (!strcmp(op, "neg")) show(fe_neg(a));
        else if (!strcmp(op, "mul")) show(fe_mul(a, b));
        else if (!strcmp(op, "sqr")) show(fe_sqr(a));
        else if (!strcmp(op, "inv")) show(fe_inv(a));
        else if (!strcmp(op, "pow")) show(fe_pow(a, b));                    // b: the exponent
        else if (!strcmp(op, "pow2")) show(fe_pow_u64(a, 2));
        else if (!strcmp(op, "pow3")) show(fe_pow_u64(a, 3));
        else if (!strcmp(op, "pow5")) show(fe_pow_u64(a, 5));
        else if (!strcmp(op, "hadd")) showh(hf_add(x, y));
        else if (!strcmp(op, "hsub")) showh(hf_sub(x, y));
        else if (!strcmp(op, "hmul")) showh(hf_mul(x, y));
        else if (!strcmp(op, "hinv")) showh(hf_inv(x));
        else if (!strcmp(op, "hmulw")) showh(hf_canon(hf_mul_weak(x, y)));
        else if (!strcmp(op, "haddw")) showh(hf_canon(hf_add_weak(x, y)));
        else if (!strcmp(op, "hchain")) showh(hf_canon(hf_add_weak(hf_mul_weak(hf_mul_weak(x, y), y), x)));   // a b^2 + a, weak all the way
#if !defined(GS_WIDE_BITS) && !defined(GS_SMALL_Q)
        else if (!strcmp(op, "lzmul")) show(lz_pack(lz_mul_v(lz_unpack(a), lz_unpack(b), lzk_make())));
        else if (!strcmp(op, "lzsqr")) show(lz_pack(lz_sqr(lz_unpack(a), lzk_make())));
        else if (!strcmp(op, "lzmulu")) { lzw W; lz_wform(b, W); show(lz_pack(lz_mul_u(lz_unpack(a), W, lzk_make()))); }
        else if (!strcmp(op, "lzmulw")) show(lz_pack(lz_unpack(lz_pack_weak(lz_mul_v(lz_unpack(a), lz_unpack(b), lzk_make())))));
#endif
        else printf("?\n");
    }
    return 0;
}
