// host_poly_check.cpp — the host-side polynomial helpers and hashing glue of the library (csrc/host_poly.h, csrc/host_hash.h, and of
// csrc/host_field.h its hf_from_digest / hf_modulus_bytes) as a filter, so that tests/test_host_poly.py can compare them with Python
// integers on machines without a GPU.  Build: g++ -O2 [-DGS_WIDE_BITS=224|256 | -DGS_SMALL_Q=<q>ull] tools/host_poly_check.cpp
// stdin: one command per line, elements as 64 hex digits (big endian; the 128-bit flavour takes ANY 128-bit value where a helper's contract does);
// stdout: one line of hex per command.
//   T n w winv a_0 .. a_(n-1)    host_transform(a, w), then host_transform of that result with winv: 2 n elements
//   L m x_0 .. x_(m-1)           host_linear_product: m + 1 coefficients, lowest first
//   I n v_0 .. v_(n-1)           host_batch_invert: n elements
//   H n c_0 .. c_(n-1) k x_0 ..  horner(c, x_j) for the k points, then horner_many(c, x): 2 k elements
//   D <64 hex digits>            hf_from_digest of these 32 bytes
//   S <hex of a message>|-       hf_from_digest(host_sha256(message)) ("-": the empty message)
//   P                            hf_modulus_bytes, as an element-sized integer
//   B <hex bytes>                host_bigint_bytes of this big-endian value: the bytes it wrote ("-": none)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>
#if defined(GS_WIDE_BITS)
#include "../genstark_amd/csrc/gf_wide.h"
#endif
#include "../genstark_amd/csrc/host_field.h"
#include "../genstark_amd/csrc/host_poly.h"
#include "../genstark_amd/csrc/host_hash.h"

static char tok[4096];
static bool next_token() { return scanf("%4095s", tok) == 1; }
static size_t next_count() { return next_token() ? (size_t)strtoull(tok, nullptr, 10) : 0; }
static std::vector<uint8_t> next_bytes() {           // the token's hex digits as bytes, in order
    std::vector<uint8_t> b;
    if (!next_token() || !strcmp(tok, "-")) return b;
    for (size_t i = 0; i + 1 < strlen(tok); i += 2) { unsigned v = 0; sscanf(tok + i, "%2x", &v); b.push_back((uint8_t)v); }
    return b;
}
static hfe next_element() {
    uint8_t b[HF_ELT] = {0};
    if (next_token()) {
        const size_t n = strlen(tok);
        for (int i = 0; i < HF_ELT; i++) {
            unsigned v = 0;
            if (n >= 2 * (size_t)(i + 1)) sscanf(tok + n - 2 * (i + 1), "%2x", &v);
            b[i] = (uint8_t)v;
        }
    }
    return hf_load(b);
}
static std::vector<hfe> next_elements(size_t n) {
    std::vector<hfe> v(n);
    for (hfe &e : v) e = next_element();
    return v;
}
static void show_bytes(const uint8_t *b, int n) {    // most significant first
    for (int i = n - 1; i >= 0; i--) printf("%02x", b[i]);
    printf(" ");
}
static void show(hfe x) {
    uint8_t b[HF_ELT];
    hf_store(b, x);
    show_bytes(b, HF_ELT);
}

int main() {
    while (next_token()) {
        const char cmd = tok[0];
        if (cmd == 'T') {
            const size_t n = next_count();
            const hfe w = next_element(), winv = next_element();
            std::vector<hfe> a = next_elements(n);
            host_transform(a, w);
            for (hfe v : a) show(v);
            host_transform(a, winv);
            for (hfe v : a) show(v);
        } else if (cmd == 'L') {
            const size_t m = next_count();
            const std::vector<hfe> xs = next_elements(m);
            std::vector<hfe> zp(m + 1);
            host_linear_product(xs.data(), m, zp.data());
            for (hfe v : zp) show(v);
        } else if (cmd == 'I') {
            std::vector<hfe> v = next_elements(next_count());
            host_batch_invert(v);
            for (hfe e : v) show(e);
        } else if (cmd == 'H') {
            const std::vector<hfe> poly = next_elements(next_count()), xs = next_elements(next_count());
            for (hfe x : xs) show(horner(poly, x));
            for (hfe v : horner_many(poly, xs)) show(v);
        } else if (cmd == 'D' || cmd == 'S') {
            std::vector<uint8_t> m = next_bytes();
            uint8_t d[32] = {0};
            if (cmd == 'S') host_sha256(m.data(), m.size(), d);
            else if (!m.empty()) memcpy(d, m.data(), m.size() < 32 ? m.size() : 32);
            show(hf_from_digest(d));
        } else if (cmd == 'P') {
            uint8_t b[HF_ELT];
            hf_modulus_bytes(b);
            show_bytes(b, HF_ELT);
        } else if (cmd == 'B') {
            const std::vector<uint8_t> be = next_bytes();
            std::vector<uint8_t> out(be.size() + 1);
            const int n = host_bigint_bytes(be.data(), (int)be.size(), out.data());
            for (int i = 0; i < n; i++) printf("%02x", out[i]);
            if (!n) printf("-");
        } else {
            printf("unknown command %s", tok);
        }
        printf("\n");
    }
    return 0;
}
