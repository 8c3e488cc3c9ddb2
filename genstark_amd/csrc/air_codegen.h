// air_codegen.h — AIR programs turned into HIP source: the code generator of the compiled programs (air_jit.hip builds, caches and
// launches what this header writes).  Static-register offsets and periods become literals, exponents become fixed addition chains:
//   constraint programs (one thread per domain point, throughput-bound): VM registers become variables, straight-line code, or — when
//   linear layers fuse — the program's SSA form node by node (ssa_emit_flat);
//   trace programs (a few thousand independent segments at most: one wave per SIMD, every dependent product paid at full latency): SSA
//   form, products scheduled by depth and spread over the 2-16 lanes that share a segment, S-box layers one member per lane, results
//   exchanged through LDS (see "trace programs" below).
// Plain C++: strings in, strings out.  No HIP, no context, no field arithmetic — the field flavour the source is written for is a VALUE
// (JitFlavour), so one host program can generate for every flavour (tests/host_harness/air_codegen_host.cpp does, also under
// -fsanitize=address,undefined).  The programs are VALIDATED ones (air_program.h: air_validate): no index is checked again here.
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "air_program.h"

// The field flavour a source is generated for.
struct JitFlavour {
    uint32_t elt;              // bytes of an element
    bool lazy;                 // the 128-bit field: long chains and fused rows run in the lazy five-limb form (gf128_lazy.h), 0/1 tables select
    bool wide;                 // multi-limb elements (gf_wide.h): products are calls, element arrays are read through gs_top0
    std::string define;        // the line the source starts with: "#define GS_SMALL_Q <q>\n", "#define GS_WIDE_BITS <bits>\n" or nothing
};

// text with every '@' replaced by the next argument (a number in decimal, or a string): no buffer, nothing to truncate
inline void jit_put(std::string &s, const std::string &v) { s += v; }
inline void jit_put(std::string &s, const char *v) { s += v; }
template <class T>
inline void jit_put(std::string &s, T v) { s += std::to_string(v); }
inline void fmt_to(std::string &s, const char *f) { s += f; }
template <class T, class... A>
inline void fmt_to(std::string &s, const char *f, const T &v, const A &...a) {
    const char *at = f;
    while (*at && *at != '@') at++;
    s.append(f, at);
    if (!*at) return;
    jit_put(s, v);
    fmt_to(s, at + 1, a...);
}
template <class... A>
inline std::string fmt(const char *f, const A &...a) {
    std::string s;
    fmt_to(s, f, a...);
    return s;
}

inline std::string jit_preamble(const JitFlavour &fl) {
    std::string s = fl.define;
    s += fl.lazy ? "#include \"gf128_lazy.h\"\n"        // brings gf128.h with it
                 : "#include \"gs_field.h\"\n";
    // the straight-line products: a call in the multi-limb fields (a product is ~400 instructions there; inlining a hundred of
    // them costs minutes of compilation and buys nothing), inlined in the others
    if (fl.wide)
        // A field narrower than its storage (224 bits in eight limbs: GF_NL = 7): the products read seven limbs of an element, the sums and
        // the stores eight, so the top limb of a value is live only here and there.  hipcc (ROCm 7.2) then spills such an element as 16 + 12
        // bytes and has been seen to store the 16-byte tuple of the upper half again after the 12-byte reload: 33 trace registers came back
        // with limb 7 of register 0 holding its limb 3.  Every element the generated code loads or computes therefore has its unused limbs
        // set to the constant they hold by definition (gs_top0): they are no values any more, nothing of them is kept, spilled or reloaded.
        s += "__device__ __forceinline__ fe gs_top0(fe x) {\n"
             "#pragma unroll\n"
             "    for (int i = GF_NL; i < GF_LIMBS; i++) x.w[i] = 0u;\n"
             "    return x;\n"
             "}\n"
             "struct gs_elts {      // an array of elements in memory, read through gs_top0\n"
             "    const fe *p;\n"
             "    __device__ __forceinline__ fe operator[](unsigned long long i) const { return gs_top0(p[i]); }\n"
             "};\n"
             "static __device__ __noinline__ fe gs_mul_call(const fe &a, const fe &b) { return fe_mul(a, b); }\n"
             "__device__ __forceinline__ fe gs_mul(const fe &a, const fe &b) { return gs_top0(gs_mul_call(a, b)); }\n"
             "__device__ __forceinline__ fe gs_sqr(const fe &a) { return gs_top0(gs_mul_call(a, a)); }\n"
             "__device__ __forceinline__ fe gs_add(const fe &a, const fe &b) { return gs_top0(fe_add(a, b)); }\n"
             "__device__ __forceinline__ fe gs_sub(const fe &a, const fe &b) { return gs_top0(fe_sub(a, b)); }\n"
             "#define fe_add gs_add\n"
             "#define fe_sub gs_sub\n";
    else
        s += "#define gs_mul fe_mul\n"
             "#define gs_sqr fe_sqr\n";
    // c ? a : b limb by limb: written as a conditional copy of the struct, the compiler parks the candidates in scratch memory and
    // loads through a selected pointer (seen in the ISA: 64 scratch accesses per Poseidon step)
    s += "__device__ __forceinline__ fe gs_pick(bool c, fe a, const fe b) {\n"
         "    unsigned int *pa = reinterpret_cast<unsigned int *>(&a);\n"
         "    const unsigned int *pb = reinterpret_cast<const unsigned int *>(&b);\n"
         "#pragma unroll\n"
         "    for (int i = 0; i < (int)(sizeof(fe) / 4); i++) pa[i] = c ? pa[i] : pb[i];\n"
         "    return a;\n"
         "}\n";
    if (!fl.lazy) {
        // sum_k x_k * c_k on ONE lane (a fused row of a linear layer, ssa_fuse_dots)
        s += "typedef fe gs_dotk;\n"
             "__device__ __forceinline__ void gs_dotk_make(fe &k, const fe c) { k = c; }\n"
             "struct gs_dot_t { fe acc; };\n"
             "__device__ __forceinline__ void gs_dot_begin(gs_dot_t &a) { a.acc = fe_zero(); }\n"
             "__device__ __forceinline__ void gs_dot_acc(gs_dot_t &a, const fe x, const fe &k) { a.acc = fe_add(a.acc, gs_mul(x, k)); }\n"
             "__device__ __forceinline__ void gs_dot_flush(gs_dot_t &) {}\n"
             "__device__ __forceinline__ fe gs_dot_end(gs_dot_t &a) { return a.acc; }\n"
             "typedef gs_dot_t gs_dot9_t;\n"
             "__device__ __forceinline__ void gs_dot9_begin(gs_dot_t &a) { a.acc = fe_zero(); }\n"
             "__device__ __forceinline__ void gs_dot9_acc(gs_dot_t &a, const fe x, const fe k) { a.acc = fe_add(a.acc, gs_mul(x, k)); }\n"
             "__device__ __forceinline__ void gs_dot9_flush(gs_dot_t &) {}\n"
             "__device__ __forceinline__ fe gs_dot9_end(gs_dot_t &a) { return a.acc; }\n";
        return s;
    }
    // f * x for a selector f (a static register whose table is all 0 / 1 when the source is generated): a select; any other value of
    // f — the table is data, it may change without the program changing — takes the product, so the result never depends on the guess
    s += "__device__ __forceinline__ fe gs_blend(const fe f, const fe x) {\n"
         "    if (__builtin_expect((f.w1 | f.w2 | f.w3) != 0u || f.w0 > 1u, 0)) return gs_mul(f, x);\n"
         "    return gs_pick(f.w0 == 1u, x, fe_zero());\n"
         "}\n";
    // sum_k x_k * c_k on ONE lane (a fused row of a linear layer, ssa_fuse_dots)
    // 128-bit field: the constants in W-form (five pre-shifted copies: no high columns), every term 25 v_mad into five shared 64-bit
    // columns, ONE fold for up to six terms (columns stay below 2^57: 6 * 5 * 2^52).  The rows of a W-form built in registers are
    // laundered through an empty asm: with their value ranges visible hipcc (ROCm 7.2) miscompiles the products (ntt.hip has the same note)
    s += "typedef lzw gs_dotk;\n"
         "__device__ __forceinline__ void gs_dotk_make(lzw &W, const fe c) {\n"
         "    lz_wform(c, W);\n"
         "#pragma unroll\n"
         "    for (int i = 0; i < 5; i++)\n"
         "#pragma unroll\n"
         "        for (int j = 0; j < 5; j++) asm volatile(\"\" : \"+v\"(W.w[i][j]));\n"
         "}\n"
         "struct gs_dot_t { long long c[5]; fe partial; bool has; };\n"
         "__device__ __forceinline__ void gs_dot_begin(gs_dot_t &a) { for (int j = 0; j < 5; j++) a.c[j] = 0; a.has = false; }\n"
         "__device__ __forceinline__ void gs_dot_acc(gs_dot_t &a, const fe x, const lzw &W) {\n"
         "    const lz u = lz_unpack(x);\n"
         "#pragma unroll\n"
         "    for (int j = 0; j < 5; j++) {\n"
         "        long long t = a.c[j];\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < 5; i++) t += (long long)u.l[i] * W.w[i][j];\n"
         "        a.c[j] = t;\n"
         "    }\n"
         "}\n"
         "__device__ __forceinline__ fe gs_dot_fold(gs_dot_t &a) {\n"
         "    const lzk K = lzk_make();\n"
         "    int64_t c[5];\n"
         "    for (int j = 0; j < 5; j++) c[j] = a.c[j];\n"
         "    return lz_pack(lz_fold_columns(c, K));\n"
         "}\n"
         "__device__ __forceinline__ void gs_dot_flush(gs_dot_t &a) {\n"
         "    const fe v = gs_dot_fold(a);\n"
         "    a.partial = a.has ? fe_add(a.partial, v) : v;\n"
         "    a.has = true;\n"
         "    for (int j = 0; j < 5; j++) a.c[j] = 0;\n"
         "}\n"
         "__device__ __forceinline__ fe gs_dot_end(gs_dot_t &a) { const fe v = gs_dot_fold(a); return a.has ? fe_add(a.partial, v) : v; }\n"
         // the same with the constant as an ordinary element (lane-uniform in the constraint kernels: its limbs are scalar values):
         // nine shared columns, the four high ones folded once (lz_fold9)
         "struct gs_dot9_t { long long c[9]; fe partial; bool has; };\n"
         "__device__ __forceinline__ void gs_dot9_begin(gs_dot9_t &a) { for (int k = 0; k < 9; k++) a.c[k] = 0; a.has = false; }\n"
         "__device__ __forceinline__ void gs_dot9_acc(gs_dot9_t &a, const fe x, const fe w) {\n"
         "    const lz u = lz_unpack(x), v = lz_unpack(w);\n"
         "#pragma unroll\n"
         "    for (int k = 0; k < 9; k++) {\n"
         "        long long t = a.c[k];\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < 5; i++) { const int j = k - i; if (j >= 0 && j < 5) t += (long long)u.l[i] * v.l[j]; }\n"
         "        a.c[k] = t;\n"
         "    }\n"
         "}\n"
         "__device__ __forceinline__ fe gs_dot9_fold(gs_dot9_t &a) {\n"
         "    const lzk K = lzk_make();\n"
         "    int64_t c[9];\n"
         "    for (int k = 0; k < 9; k++) c[k] = a.c[k];\n"
         "    return lz_pack(lz_fold9(c, K));\n"
         "}\n"
         "__device__ __forceinline__ void gs_dot9_flush(gs_dot9_t &a) {\n"
         "    const fe v = gs_dot9_fold(a);\n"
         "    a.partial = a.has ? fe_add(a.partial, v) : v;\n"
         "    a.has = true;\n"
         "    for (int k = 0; k < 9; k++) a.c[k] = 0;\n"
         "}\n"
         "__device__ __forceinline__ fe gs_dot9_end(gs_dot9_t &a) { const fe v = gs_dot9_fold(a); return a.has ? fe_add(a.partial, v) : v; }\n";
    return s;
}
// the read-only element arrays of a generated kernel: plain pointers, or (multi-limb flavours) gs_elts over the renamed argument
inline std::string jit_arg(const JitFlavour &fl, const char *name) { return fl.wide ? std::string(name) + "_" : name; }
inline std::string jit_wrap(const JitFlavour &fl, const char *name) { return fl.wide ? fmt("    const gs_elts @ = {@_};\n", name, name) : ""; }

// What the generator knows besides the program (an AirProgram: its constant pool is where exponents become addition chains at generation
// time): the flavour; in the trace kernel, how many lanes work on one segment, and the tables of the static registers.
struct JitGen {
    const JitFlavour &fl;
    uint32_t lanes = 1;                // 1, 2 or 4 consecutive lanes per segment (trace kernel only)
    // trace programs: host copy of the static registers' tables (element p.sd.offset[s] + i), or null.  A static register whose table
    // holds only 0 and 1 is a SELECTOR (Poseidon's full / partial round flag): products by it are emitted as selects (SsaNode::BLEND)
    const uint8_t *statics = nullptr;
    bool static_is_binary(const AirProgram &p, uint32_t reg) const {
        if (!fl.lazy || !statics || reg >= p.nstatic) return false;
        for (uint64_t i = 0; i < p.sd.len[reg]; i++) {
            const uint8_t *v = statics + (p.sd.offset[reg] + i) * fl.elt;
            if (v[0] > 1) return false;
            for (uint32_t b = 1; b < fl.elt; b++) if (v[b]) return false;
        }
        return p.sd.len[reg] > 0;
    }
};
// an exponent as little-endian 32-bit limbs: constant `v` of the pool, or (pooled = false) the number v itself
inline std::vector<uint32_t> jit_exponent(const JitFlavour &fl, const AirProgram &p, bool pooled, uint32_t v) {
    std::vector<uint32_t> e(fl.elt / 4, 0u);
    if (!pooled) e[0] = v;
    else for (uint32_t i = 0; i < fl.elt; i++) e[i / 4] |= (uint32_t)p.consts[(size_t)v * fl.elt + i] << (8 * (i % 4));
    return e;
}
// element `at` (an expression) of static register a's table, which is read cyclically
inline std::string jit_static_at(const AirProgram &p, uint32_t a, const std::string &at) {
    const uint64_t off = p.sd.offset[a], len = p.sd.len[a];
    return len & (len - 1) ? fmt("statics[@ull + @ % @ull]", off, at, len) : fmt("statics[@ull + (@ & @ull)]", off, at, len - 1);
}

// x <- x^e as a fixed addition chain: left-to-right sliding windows over the bits of e (little-endian 32-bit limbs), the window
// width chosen by counting products.  The inverse S-box of Rescue (a 128-bit exponent) is 127 squarings + 32 products instead of
// the 127 + 64 of square-and-multiply; a Fermat inversion in the 224-bit field 224 + 53 instead of 224 + 222.  (Right to left the
// squarings and the running product are independent chains, but a wave issues in order and a loop does not interleave them: measured
// in the trace kernel, 2.2 ms against 1.8 ms for the windows.)
struct PowPlan {
    uint32_t table_max = 1;                                    // odd powers x^1 .. x^table_max are needed
    std::vector<std::pair<uint32_t, uint32_t>> steps;          // (squarings, odd power to multiply by; 0 = none); first: (0, start)
    uint32_t cost = 0;
};
inline PowPlan pow_plan(const std::vector<uint32_t> &e, int nbits, int w) {
    PowPlan pl;
    auto bit = [&](int i) { return (e[i / 32] >> (i % 32)) & 1u; };
    int i = nbits - 1;
    uint32_t pending = 0;
    bool first = true;
    while (i >= 0) {
        if (!bit(i)) { pending++; i--; continue; }
        int j = i - w + 1 < 0 ? 0 : i - w + 1;
        while (!bit(j)) j++;
        uint32_t val = 0;
        for (int k = i; k >= j; k--) val = 2 * val + bit(k);
        if (first) pl.steps.push_back({0, val});
        else { pl.steps.push_back({pending + (uint32_t)(i - j + 1), val}); pl.cost += pending + (i - j + 1) + 1; }
        first = false;
        pending = 0;
        if (val > pl.table_max) pl.table_max = val;
        i = j - 1;
    }
    if (pending) { pl.steps.push_back({pending, 0}); pl.cost += pending; }
    if (pl.table_max > 1) pl.cost += 1 + (pl.table_max - 1) / 2;
    return pl;
}
// Exponents whose top bits repeat "10" — (2p - 1)/3, the inverse of the cube, is 1010...10 over its top 92 bits in the 128-bit field —
// have a much shorter chain than windows give: with r_k = x^("10" k times), r_{a+b} = r_a^(4^b) * r_b, so r_k costs 2k - 1 squarings and
// about log2 k + popcount k products (k = 46: 91 + 8, where five-bit windows spend 23 products on the same 92 bits), and the r_j met on
// the way are dictionary words for the remaining low bits (greedy longest match among them, x and x^3).  ops: (squarings, word to
// multiply by; "" = none); words are variable names: "p1", "p3", "g<j>" = r_j.  Returns false when the exponent has no such run.
struct PatOp { uint32_t sq; std::string word; };
struct PatPlan {
    uint32_t k = 0;                                            // pairs of the leading run
    std::vector<std::pair<uint32_t, uint32_t>> doubling;       // (j, 0): g_{2j} = g_j^(4^j) g_j;  (j, 1): g_{j+1} = g_j^4 g_1
    std::vector<PatOp> ops;                                    // after acc = g_k
    bool needs_p3 = false;
    uint32_t cost = 0;
};
inline bool pattern_plan(const std::vector<uint32_t> &e, int nbits, PatPlan &pl) {
    auto bit = [&](int i) { return i >= 0 ? (e[i / 32] >> (i % 32)) & 1u : 0u; };
    int i = nbits - 1;
    while (i >= 1 && bit(i) && !bit(i - 1)) { pl.k++; i -= 2; }
    if (pl.k < 8) return false;
    std::vector<uint32_t> have = {1};                          // the r_j that exist, ascending
    pl.cost = 1;                                               // g1 = x^2
    {
        int top = 31;
        while (!((pl.k >> top) & 1u)) top--;
        uint32_t j = 1;
        for (int b = top - 1; b >= 0; b--) {
            pl.doubling.push_back({j, 0}); pl.cost += 2 * j + 1; j *= 2; have.push_back(j);
            if ((pl.k >> b) & 1u) { pl.doubling.push_back({j, 1}); pl.cost += 3; j += 1; have.push_back(j); }
        }
    }
    uint32_t pending = 0;
    while (i >= 0) {
        if (!bit(i)) { pending++; i--; continue; }
        // longest dictionary word that matches the bits from i down: "10" x j (needs 2j bits), "11" (x^3), "1" (x)
        uint32_t best_j = 0;
        for (uint32_t j : have) {
            if ((int)(2 * j) > i + 1) continue;
            bool ok = true;
            for (uint32_t t = 0; ok && t < j; t++) ok = bit(i - 2 * (int)t) && !bit(i - 2 * (int)t - 1);
            if (ok) best_j = j;
        }
        std::string w = "p1";
        uint32_t len = 1;
        if (best_j) { w = fmt("g@", best_j); len = 2 * best_j; }
        else if (i >= 1 && bit(i - 1)) { w = "p3"; len = 2; pl.needs_p3 = true; }
        pl.ops.push_back({pending + len, w});
        pl.cost += pending + len + 1;
        pending = 0;
        i -= (int)len;
    }
    if (pending) { pl.ops.push_back({pending, ""}); pl.cost += pending; }
    if (pl.needs_p3) pl.cost += 1;
    return true;
}

// The form a chain runs in: canonical elements, or the lazy five-limb form from end to end — one unpack, lz_sqr (15 products + fold:
// ~53 instructions against the 84 of a canonical fe_mul) and lz_mul_v, one pack.
struct ChainForm { const char *type, *sqr, *mul, *k, *open, *unpack, *pack; };
static const ChainForm kCanonicalChain = {"fe", "gs_sqr", "gs_mul", "", "", "", ""};
static const ChainForm kLazyChain = {"lz", "lz_sqr", "lz_mul_v", ", K", "                const lzk K = lzk_make();\n", "lz_unpack", "lz_pack"};
inline std::string chain_call(const char *fn, const std::string &x) { return fn[0] ? fmt("@(@)", fn, x) : x; }
inline void chain_open(std::string &s, const ChainForm &f, const std::string &x) {
    s += fmt("            {\n@                const @ p1 = @;\n", f.open, f.type, chain_call(f.unpack, x));
}
inline void chain_close(std::string &s, const ChainForm &f, const std::string &x) { s += fmt("                @ = @;\n            }\n", x, chain_call(f.pack, "acc")); }
// n squarings of v; four or more are a loop
inline void chain_squarings(std::string &s, const ChainForm &f, const char *v, uint32_t n) {
    const std::string one = fmt("@ = @(@@);\n", v, f.sqr, v, f.k);
    if (n >= 4) s += fmt("#pragma nounroll\n                for (int q = 0; q < @; q++) ", n) + one;
    else for (uint32_t q = 0; q < n; q++) s += "                " + one;
}
inline void chain_product(std::string &s, const ChainForm &f, const std::string &dst, const std::string &a, const std::string &b) {
    s += fmt("                @ = @(@, @@);\n", dst, f.mul, a, b, f.k);
}
// the sliding-window chain of a plan, in either form
inline void chain_windows(std::string &s, const ChainForm &f, const std::string &x, const PowPlan &pl) {
    chain_open(s, f, x);
    if (pl.table_max > 1) {
        s += fmt("                const @ p2 = @(p1@);\n", f.type, f.sqr, f.k);
        for (uint32_t v = 3; v <= pl.table_max; v += 2) chain_product(s, f, fmt("const @ p@", f.type, v), fmt("p@", v - 2), "p2");
    }
    s += fmt("                @ acc = p@;\n", f.type, pl.steps[0].second);
    for (size_t k = 1; k < pl.steps.size(); k++) {
        chain_squarings(s, f, "acc", pl.steps[k].first);
        if (pl.steps[k].second) chain_product(s, f, "acc", "acc", fmt("p@", pl.steps[k].second));
    }
    chain_close(s, f, x);
}
// the "10"-run chain of a PatPlan (lazy form only)
inline void chain_pattern(std::string &s, const std::string &x, const PatPlan &pat) {
    const ChainForm &f = kLazyChain;
    chain_open(s, f, x);
    s += "                const lz g1 = lz_sqr(p1, K);\n";
    if (pat.needs_p3) chain_product(s, f, "const lz p3", "g1", "p1");
    s += "                lz acc;\n";
    for (auto &d : pat.doubling) {
        const uint32_t j = d.first;
        s += fmt("                acc = g@;\n", j);
        chain_squarings(s, f, "acc", d.second ? 2 : 2 * j);
        if (d.second) chain_product(s, f, fmt("const lz g@", j + 1), "acc", "g1");
        else chain_product(s, f, fmt("const lz g@", 2 * j), "acc", fmt("g@", j));
    }
    s += fmt("                acc = g@;\n", pat.k);
    for (auto &o : pat.ops) {
        chain_squarings(s, f, "acc", o.sq);
        if (!o.word.empty()) chain_product(s, f, "acc", "acc", o.word);
    }
    chain_close(s, f, x);
}

inline void emit_pow(std::string &s, const JitFlavour &fl, const std::string &x, const std::vector<uint32_t> &e) {
    int nbits = 0;
    for (int i = (int)e.size() * 32 - 1; i >= 0 && !nbits; i--)
        if ((e[i / 32] >> (i % 32)) & 1u) nbits = i + 1;
    if (!nbits) { s += fmt("            @ = fe_one();\n", x); return; }
    PowPlan best = pow_plan(e, nbits, 1);
    for (int w = 2; w <= 5; w++) {
        PowPlan pl = pow_plan(e, nbits, w);
        if (pl.cost < best.cost) best = pl;
    }
    if (best.steps.size() == 1 && best.steps[0].second == 1) return;     // x^1
    // A long chain (Rescue's inverse S-box: 127 squarings + 32 products) runs in the lazy five-limb form from end to end.  On a single
    // wave per SIMD a chain of dependent products costs its instruction count, so this is the length of the trace kernel's critical path.
    PatPlan pat;
    if (fl.lazy && pattern_plan(e, nbits, pat) && pat.cost < best.cost) chain_pattern(s, x, pat);
    else chain_windows(s, fl.lazy && best.cost >= 8 ? kLazyChain : kCanonicalChain, x, best);
}

// straight-line statements for `ninstr` instructions at `code` of the constraint program p (one thread per domain point:
// throughput-bound, no lanes); `index` names the loop variable static tables are indexed by
inline bool jit_body(std::string &s, const JitFlavour &fl, const AirProgram &p, const uint32_t *code, uint32_t ninstr, bool allow_statics, const char *cur,
                     const char *nxt, const char *index, const char *sink) {
    for (uint32_t pc = 0; pc < ninstr; pc++) {
        const uint32_t op = code[4 * pc], d = code[4 * pc + 1], a = code[4 * pc + 2], b = code[4 * pc + 3];
        switch (op) {
            case OP_LOADC: s += fmt("        t@ = consts[@];\n", d, a); break;
            case OP_LOADR: s += fmt("        t@ = @@;\n", d, cur, a); break;
            case OP_LOADN:
                if (!nxt) return false;
                s += fmt("        t@ = @@;\n", d, nxt, a);
                break;
            case OP_LOADS:
                if (!allow_statics) return false;
                s += fmt("        t@ = @;\n", d, jit_static_at(p, a, index));
                break;
            case OP_ADDV: s += fmt("        t@ = fe_add(t@, t@);\n", d, a, b); break;
            case OP_SUBV: s += fmt("        t@ = fe_sub(t@, t@);\n", d, a, b); break;
            case OP_MULV: s += fmt("        t@ = gs_mul(t@, t@);\n", d, a, b); break;
            case OP_POW:
            case OP_POWC: {
                const std::vector<uint32_t> e = jit_exponent(fl, p, op == OP_POWC, b);
                const uint32_t g = air_pow_group(code, ninstr, pc);
                s += "        {\n";
                for (uint32_t i = 0; i < g; i++) s += fmt("            fe x@ = t@;\n", i, code[4 * (pc + i) + 2]);
                for (uint32_t i = 0; i < g; i++) emit_pow(s, fl, fmt("x@", i), e);
                for (uint32_t i = 0; i < g; i++) s += fmt("            t@ = x@;\n", code[4 * (pc + i) + 1], i);
                s += "        }\n";
                pc += g - 1;
                break;
            }
            case OP_OUT: s += fmt("        @@ = t@;\n", sink, d, a); break;
            default: return false;
        }
    }
    return true;
}

// ---- trace programs: products scheduled by depth and spread over the lanes of a segment ------------------------------------------
// A thread of the trace kernel has its SIMD to itself, so it pays the full latency of every product it waits for, and the compiler
// does not overlap inlined 128-bit products either: a compiled Poseidon round (36 MDS products + 18 S-box products) costs
// 54 x ~750 cycles.  The program is therefore put in SSA form and every product gets a depth (1 + the depth of its operands;
// additions, loads and outputs do not add depth): products of one depth are independent, and L of them run as ONE round — lane i of
// the segment's group multiplies the i-th pair, the results are broadcast with shuffles, every lane continues with all values.
// Cheap operations run redundantly on all lanes.  Long exponentiations of one depth and exponent are rounds of their own (one
// member per lane).  L = 1, 2, 4 or 8 by the widest depth.
struct SsaNode {
    enum Kind { ZERO, CONSTV, ROW, ROWN, STATICV, ADD, SUB, MUL, POWLONG, POWSHORT, OUT, DOT, DEAD, BLEND } kind = ZERO;
    int a = -1, b = -1;        // operand nodes (MUL/ADD/SUB/POWLONG/OUT: a; b for binary; BLEND: a = the selector, b = the value) or the index of a constant/register/static
    uint32_t aux = 0;          // POWLONG: constant index of the exponent; POWSHORT: the exponent; OUT: destination register
    int depth = 0;
    // DOT: sum_k value(tx[k]) * consts[tc[k]]  (tc[k] = -1: the literal one) — a linear layer's row (an MDS matrix times the state) fused
    // into ONE unit of work for ONE lane (ssa_fuse_dots)
    std::vector<int> tx, tc;
    bool is_product() const { return kind == MUL || kind == POWLONG || kind == POWSHORT || kind == DOT; }      // one level of depth
    bool is_pow() const { return kind == POWLONG || kind == POWSHORT; }
};
inline void ssa_operands(const SsaNode &x, std::vector<int> &out) {
    out.clear();
    switch (x.kind) {
        case SsaNode::ADD: case SsaNode::SUB: case SsaNode::MUL: case SsaNode::BLEND: out.push_back(x.a); out.push_back(x.b); break;
        case SsaNode::POWLONG: case SsaNode::POWSHORT: case SsaNode::OUT: out.push_back(x.a); break;
        case SsaNode::DOT: out = x.tx; break;
        default: break;
    }
}
// depth of every node from its operands'; `forced`: a floor per node (ssa_align_pows)
inline void ssa_recompute_depths(std::vector<SsaNode> &nodes, const std::vector<int> *forced = nullptr) {
    std::vector<int> ops;
    for (size_t id = 0; id < nodes.size(); id++) {
        SsaNode &n = nodes[id];
        ssa_operands(n, ops);
        int d = 0;
        for (int o : ops) d = std::max(d, nodes[o].depth);
        if (n.is_product()) d++;
        n.depth = forced ? std::max(d, (*forced)[id]) : d;
    }
}
// a constant of the pool (not the literal one)
inline bool ssa_is_const(const std::vector<SsaNode> &nodes, int id) { return nodes[id].kind == SsaNode::CONSTV && nodes[id].a >= 0; }
// Sums of products by constants — the rows of a linear layer, y_j = sum_k m_jk x_k: an ADD tree whose leaves are MUL(value, constant)
// nodes used nowhere else — become ONE node each.  Spread over the lanes product by product such a layer costs a round per L products,
// a select chain per operand, an LDS read-back per product and, on every lane, the whole tree of additions (a Poseidon step: 36
// products in 2.25 rounds + 30 additions x 16 lanes); as a DOT node a row is one lane's work — in the 128-bit field K x 25 v_mad into
// five shared 64-bit columns and ONE fold (gf128_lazy.h: the W-forms of the row's constants are built before the step loop), the rows
// of a layer side by side on K lanes, one exchange for the whole layer.  Leaves that are not products by constants ride along with the
// constant one.  Trees with fewer than two genuine products are left alone.
inline void ssa_fuse_dots(std::vector<SsaNode> &nodes) {
    const int n = (int)nodes.size();
    std::vector<int> uses(n, 0), ops;
    for (const SsaNode &x : nodes) { ssa_operands(x, ops); for (int o : ops) uses[o]++; }
    auto is_const = [&](int id) { return ssa_is_const(nodes, id); };
    std::vector<bool> absorbed(n, false);
    for (int id = n - 1; id >= 0; id--) {
        if (nodes[id].kind != SsaNode::ADD || absorbed[id]) continue;
        // leaves of the maximal ADD tree rooted here (inner ADDs must have no other user)
        std::vector<int> leaves, inner, stack = {nodes[id].a, nodes[id].b};
        while (!stack.empty()) {
            const int v = stack.back();
            stack.pop_back();
            if (nodes[v].kind == SsaNode::ADD && uses[v] == 1 && !absorbed[v]) { inner.push_back(v); stack.push_back(nodes[v].a); stack.push_back(nodes[v].b); }
            else leaves.push_back(v);
        }
        std::vector<int> tx, tc, dead;
        int products = 0;
        for (int v : leaves) {
            const SsaNode &m = nodes[v];
            if (m.kind == SsaNode::MUL && uses[v] == 1 && (is_const(m.a) != is_const(m.b))) {
                tx.push_back(is_const(m.a) ? m.b : m.a);
                tc.push_back(nodes[is_const(m.a) ? m.a : m.b].a);
                dead.push_back(v);
                products++;
            } else { tx.push_back(v); tc.push_back(-1); }
        }
        if (products < 2 || tx.size() > 64) continue;
        // operands in a canonical order: the rows of one layer then line up position by position (shared operands need no selects)
        std::vector<size_t> order(tx.size());
        for (size_t k = 0; k < order.size(); k++) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return tx[x] < tx[y]; });
        SsaNode &r = nodes[id];
        r.kind = SsaNode::DOT;
        r.a = r.b = -1;
        for (size_t k : order) { r.tx.push_back(tx[k]); r.tc.push_back(tc[k]); }
        for (int v : dead) { nodes[v].kind = SsaNode::DEAD; absorbed[v] = true; }
        for (int v : inner) { nodes[v].kind = SsaNode::DEAD; absorbed[v] = true; }
    }
    ssa_recompute_depths(nodes);
}

// false: the program has something this route does not generate code for (what is ill-formed the validator has refused before)
inline bool ssa_build(std::vector<SsaNode> &nodes, const JitGen &gen, const AirProgram &p, bool allow_statics, bool allow_next = false) {
    std::vector<int> cur(p.vm_regs, -1);
    std::map<uint32_t, int> last_out;      // destination -> its latest OUT node (the machine is sequential: the last write wins)
    auto add = [&](SsaNode n) { nodes.push_back(n); return (int)nodes.size() - 1; };
    auto use = [&](uint32_t r) {
        if (cur[r] < 0) { SsaNode z; cur[r] = add(z); }
        return cur[r];
    };
    auto binary = [&](SsaNode::Kind k, int x, int y) {
        SsaNode n;
        n.kind = k; n.a = x; n.b = y;
        n.depth = std::max(nodes[x].depth, nodes[y].depth) + (k == SsaNode::MUL ? 1 : 0);
        return add(n);
    };
    for (uint32_t pc = 0; pc < p.ninstr; pc++) {
        const uint32_t op = p.code[4 * pc], d = p.code[4 * pc + 1], a = p.code[4 * pc + 2], b = p.code[4 * pc + 3];
        SsaNode n;
        switch (op) {
            case OP_LOADC: n.kind = SsaNode::CONSTV; n.a = (int)a; cur[d] = add(n); break;
            case OP_LOADR: n.kind = SsaNode::ROW; n.a = (int)a; cur[d] = add(n); break;
            case OP_LOADN:
                if (!allow_next) return false;       // (does not occur in trace programs)
                n.kind = SsaNode::ROWN; n.a = (int)a; cur[d] = add(n);
                break;
            case OP_LOADS:
                if (!allow_statics) return false;
                n.kind = SsaNode::STATICV; n.a = (int)a; cur[d] = add(n);
                break;
            case OP_ADDV: case OP_SUBV: case OP_MULV: {
                const int x = use(a), y = use(b);
                if (op == OP_MULV) {
                    // a product by a 0/1 selector is a select: cheap, on every lane, no round of its own (gs_blend still multiplies
                    // should the table ever hold anything else)
                    const bool fx = nodes[x].kind == SsaNode::STATICV && gen.static_is_binary(p, (uint32_t)nodes[x].a);
                    const bool fy = nodes[y].kind == SsaNode::STATICV && gen.static_is_binary(p, (uint32_t)nodes[y].a);
                    if (fx || fy) {
                        SsaNode bl;
                        bl.kind = SsaNode::BLEND; bl.a = fx ? x : y; bl.b = fx ? y : x;
                        bl.depth = std::max(nodes[x].depth, nodes[y].depth);
                        cur[d] = add(bl);
                        break;
                    }
                }
                cur[d] = binary(op == OP_ADDV ? SsaNode::ADD : (op == OP_SUBV ? SsaNode::SUB : SsaNode::MUL), x, y);
                break;
            }
            case OP_POW: case OP_POWC: {
                const int x = use(a);
                uint64_t e = b;
                if (op == OP_POWC) {
                    const uint8_t *eb = p.consts + (size_t)b * gen.fl.elt;
                    bool wide_exponent = false;
                    for (uint32_t i = 4; i < gen.fl.elt; i++) wide_exponent |= eb[i] != 0;
                    if (wide_exponent) {
                        n.kind = SsaNode::POWLONG; n.a = x; n.aux = b; n.depth = nodes[x].depth + 1;
                        cur[d] = add(n);
                        break;
                    }
                    e = (uint64_t)eb[0] | ((uint64_t)eb[1] << 8) | ((uint64_t)eb[2] << 16) | ((uint64_t)eb[3] << 24);
                }
                if (e == 0) { n.kind = SsaNode::CONSTV; n.a = -1; cur[d] = add(n); break; }      // x^0 = 1 (a = -1: the literal one)
                if (e == 1) { cur[d] = x; break; }
                if (e >> 32) return false;
                // an S-box: a short chain of products that stays on ONE lane (x^5: square, square, multiply) — a round of its own
                // kind, so that the lanes exchange the powers only, not every intermediate square
                n.kind = SsaNode::POWSHORT; n.a = x; n.aux = (uint32_t)e; n.depth = nodes[x].depth + 1;
                cur[d] = add(n);
                break;
            }
            case OP_OUT:
                n.kind = SsaNode::OUT; n.a = use(a); n.aux = d; n.depth = nodes[n.a].depth;
                // outputs are emitted depth by depth, not in program order: an earlier OUT to the same destination is dropped here,
                // or it would overwrite this one whenever its value is the deeper of the two
                if (last_out.count(d)) nodes[last_out[d]].kind = SsaNode::DEAD;
                last_out[d] = add(n);
                break;
            default: return false;      // OP_LOADN does not occur in trace programs
        }
    }
    return true;
}

// Long exponentiations that do not depend on each other should share a round even when their operands are ready at different depths
// (the two slopes of a point addition: one inversion waits for the doubled point, the other does not): the earlier one is delayed to
// the depth of the later one — a delay of a few products against a whole exponentiation saved — and the depths are recomputed.
inline void ssa_align_pows(std::vector<SsaNode> &nodes) {
    const int n = (int)nodes.size();
    std::vector<int> pows;
    for (int id = 0; id < n; id++)
        if (nodes[id].kind == SsaNode::POWLONG) pows.push_back(id);
    if (pows.size() < 2) return;
    std::vector<int> op;
    // reach[k][id]: node id depends on pows[k]
    std::vector<std::vector<bool>> reach(pows.size(), std::vector<bool>(n, false));
    for (size_t k = 0; k < pows.size(); k++)
        for (int id = pows[k] + 1; id < n; id++) {
            ssa_operands(nodes[id], op);
            for (int o : op)
                if (o == pows[k] || reach[k][o]) reach[k][id] = true;
        }
    std::vector<int> forced(n, 0);
    std::vector<bool> grouped(pows.size(), false);
    for (size_t k = 0; k < pows.size(); k++) {
        if (grouped[k]) continue;
        std::vector<size_t> group = {k};
        grouped[k] = true;
        for (size_t j = k + 1; j < pows.size() && group.size() < 8; j++) {
            if (grouped[j] || nodes[pows[j]].aux != nodes[pows[k]].aux) continue;
            bool independent = true;
            for (size_t g : group) independent &= !reach[g][pows[j]] && !reach[j][pows[g]];
            if (independent) { group.push_back(j); grouped[j] = true; }
        }
        int depth = 0;
        for (size_t g : group) depth = std::max(depth, nodes[pows[g]].depth);
        for (size_t g : group) forced[pows[g]] = depth;
        ssa_recompute_depths(nodes, &forced);      // the delay moves everything behind the group: before the next group is formed
    }
}

inline uint32_t ssa_lanes(const JitFlavour &fl, const std::vector<SsaNode> &nodes) {
    std::map<int, uint32_t> per_depth;
    uint32_t widest = 1;
    for (const SsaNode &n : nodes) {
        // multi-limb flavours: the group is as wide as the layer of long exponentiations (a step is their chain of ~280 products;
        // more lanes for the sake of the few single products changes nothing: point multiplication 79.5 vs 79.7 ms)
        if (fl.wide && (n.kind == SsaNode::MUL || n.kind == SsaNode::POWSHORT)) continue;
        if (n.is_product())
            widest = std::max(widest, ++per_depth[n.depth * 4 + (n.kind == SsaNode::POWLONG ? 1 : (n.kind == SsaNode::POWSHORT ? 2 : (n.kind == SsaNode::DOT ? 3 : 0)))]);
    }
    return widest >= 12 ? 16 : (widest >= 5 ? 8 : (widest >= 3 ? 4 : widest));
}

// How an emitter names a node's value.  The trace kernel (hoisted != null) keeps the current row in r<n> and declares the constants it
// uses before the step loop, once; the constraint kernel reads a constant where it is used.  Naming a constant may therefore append to
// *hoisted: name operands one statement at a time, in the order they appear in the emitted text.
struct SsaNames {
    const std::vector<SsaNode> &nodes;
    const char *tag;
    std::string *hoisted = nullptr;
    std::vector<bool> *const_declared = nullptr;
    std::string operator()(int id) const {
        const SsaNode &n = nodes[id];
        if (n.kind == SsaNode::ZERO) return "fe_zero()";
        if (n.kind == SsaNode::ROW && hoisted) return fmt("r@", n.a);
        if (n.kind == SsaNode::CONSTV) {
            if (n.a < 0) return "fe_one()";
            if (!hoisted) return fmt("consts[@]", n.a);
            if (!(*const_declared)[n.a]) {
                *hoisted += fmt("    const fe c@ = consts[@];\n", n.a, n.a);
                (*const_declared)[n.a] = true;
            }
            return fmt("c@", n.a);
        }
        return fmt("@@", tag, id);
    }
    // "        const fe <id> = fn(<a>, <b>);"
    std::string binary(int id, const char *fn) const {
        const std::string d = (*this)(id), a = (*this)(nodes[id].a), b = (*this)(nodes[id].b);
        return fmt("        const fe @ = @(@, @);\n", d, fn, a, b);
    }
    // "<var> = first;" then one limb-wise select per further lane whose operand differs
    std::string picked(const char *indent, const char *var, const std::vector<int> &ids, bool skip_same) const {
        std::string s = fmt("@fe @ = @;\n", indent, var, (*this)(ids[0]));
        for (size_t i = 1; i < ids.size(); i++)
            if (!skip_same || ids[i] != ids[0]) s += fmt("@@ = gs_pick(sub == @u, @, @);\n", indent, var, i, (*this)(ids[i]), var);      // (the lanes that keep the default need no select)
        return s;
    }
};
// the results of a round change lanes through LDS: every lane writes `value`, member i's comes back from lane i of the group
inline void emit_exchange(std::string &s, const SsaNames &name, const char *value, const std::vector<int> &members) {
    s += fmt("            gs_swap[threadIdx.x] = @;\n            __syncthreads();\n", value);
    for (size_t i = 0; i < members.size(); i++) s += fmt("            @ = gs_swap[gs_group + @];\n", name(members[i]), i);
    s += "            __syncthreads();\n";
}

// `hoisted` receives declarations that belong before the step loop: the constants the body uses, and per round of products by
// constants the ONE constant each lane needs (a lane-dependent, step-independent load instead of L loads and selects per step).
inline void ssa_emit(std::string &s, std::string &hoisted, std::vector<bool> &const_declared, const std::vector<SsaNode> &nodes, const JitFlavour &fl,
                     const AirProgram &p, const uint32_t L, const char *index, const char *sink, const char *tag) {
    int max_depth = 0;
    for (const SsaNode &n : nodes) max_depth = std::max(max_depth, n.depth);
    const SsaNames name{nodes, tag, &hoisted, &const_declared};
    auto is_const = [&](int id) { return ssa_is_const(nodes, id); };
    int round_no = 0;
    const bool spread = L > 1;
    for (int depth = 0; depth <= max_depth; depth++) {
        // the products of this depth, L per round
        std::vector<int> muls, pows, dots;
        for (int id = 0; id < (int)nodes.size(); id++) {
            if (nodes[id].depth != depth) continue;
            if (nodes[id].kind == SsaNode::MUL) muls.push_back(id);
            if (nodes[id].is_pow()) pows.push_back(id);
            if (nodes[id].kind == SsaNode::DOT) dots.push_back(id);
        }
        if (spread) {   // products by constants first, so that rounds are all-constant where they can be
            std::stable_partition(muls.begin(), muls.end(), [&](int id) { return is_const(nodes[id].a) || is_const(nodes[id].b); });
        }
        for (size_t base = 0; base < muls.size(); base += spread ? L : 1) {
            const size_t m = std::min<size_t>(L, muls.size() - base);
            if (!spread) { s += name.binary(muls[base], "gs_mul"); continue; }
            // operands: (variable, constant) when every product of the round has a constant side
            const std::vector<int> members(muls.begin() + base, muls.begin() + base + m);
            std::vector<int> xa(m), xb(m);
            bool by_consts = true, squares = true;
            for (size_t i = 0; i < m; i++) {
                const SsaNode &n = nodes[members[i]];
                xa[i] = n.a; xb[i] = n.b;
                if (is_const(xa[i]) && !is_const(xb[i])) std::swap(xa[i], xb[i]);
                by_consts &= is_const(xb[i]);
                squares &= n.a == n.b;
            }
            for (int id : members) s += "        fe " + name(id) + ";\n";
            s += "        {\n" + name.picked("            ", "xa", xa, true);
            if (squares) s += "            const fe xr = gs_sqr(xa);\n";
            else if (by_consts) {
                hoisted += fmt("    const fe @k@ = consts[", tag, round_no);
                for (size_t i = m - 1; i >= 1; i--) hoisted += fmt("sub == @u ? @u : ", i, nodes[xb[i]].a);
                hoisted += fmt("@u];\n", nodes[xb[0]].a);
                s += fmt("            const fe xr = gs_mul(xa, @k@);\n", tag, round_no);
            } else s += name.picked("            ", "xb", xb, true) + "            const fe xr = gs_mul(xa, xb);\n";
            emit_exchange(s, name, "xr", members);
            s += "        }\n";
            round_no++;
        }
        // long exponentiations of this depth: one member per lane, grouped by exponent
        std::vector<bool> done(pows.size(), false);
        for (size_t first = 0; first < pows.size(); first++) {
            if (done[first]) continue;
            const SsaNode &lead = nodes[pows[first]];
            std::vector<int> members, bases;
            for (size_t k = first; k < pows.size() && members.size() < L; k++)
                if (!done[k] && nodes[pows[k]].kind == lead.kind && nodes[pows[k]].aux == lead.aux) { members.push_back(pows[k]); bases.push_back(nodes[pows[k]].a); done[k] = true; }
            for (int id : members) s += "        fe " + name(id) + ";\n";
            s += "        {\n" + name.picked("            ", "x", bases, false);
            emit_pow(s, fl, "x", jit_exponent(fl, p, lead.kind == SsaNode::POWLONG, lead.aux));
            if (spread) emit_exchange(s, name, "x", members);
            else for (int id : members) s += "            " + name(id) + " = x;\n";
            s += "        }\n";
        }
        // the fused rows of this depth (ssa_fuse_dots): one row per lane, rows with the same number of terms side by side
        std::vector<bool> dot_done(dots.size(), false);
        for (size_t first = 0; first < dots.size(); first++) {
            if (dot_done[first]) continue;
            std::vector<int> members;
            const size_t K = nodes[dots[first]].tx.size();
            for (size_t k = first; k < dots.size() && members.size() < (spread ? L : 1); k++)
                if (!dot_done[k] && nodes[dots[k]].tx.size() == K) { members.push_back(dots[k]); dot_done[k] = true; }
            const size_t m = members.size();
            for (int id : members) s += "        fe " + name(id) + ";\n";
            // the constants of position k, one per lane, in the form the accumulation wants (before the step loop)
            auto constant = [&](size_t i, size_t k) { const int c = nodes[members[i]].tc[k]; return c < 0 ? std::string("fe_one()") : fmt("consts[@]", c); };
            for (size_t k = 0; k < K; k++) {
                hoisted += fmt("    gs_dotk @d@_@; gs_dotk_make(@d@_@, ", tag, round_no, k, tag, round_no, k);
                for (size_t i = m - 1; i >= 1; i--) hoisted += fmt("sub == @u ? @ : ", i, constant(i, k));
                hoisted += constant(0, k) + ");\n";
            }
            s += "        {\n            gs_dot_t acc;\n            gs_dot_begin(acc);\n";
            for (size_t k = 0; k < K; k++) {
                if (k && k % 6 == 0) s += "            gs_dot_flush(acc);\n";      // (128-bit field: six terms per fold keep the 64-bit columns below 2^57)
                std::vector<int> terms(m);
                bool shared = true;
                for (size_t i = 0; i < m; i++) { terms[i] = nodes[members[i]].tx[k]; shared &= terms[i] == terms[0]; }
                if (shared) s += fmt("            gs_dot_acc(acc, @, @d@_@);\n", name(terms[0]), tag, round_no, k);
                else s += "            {\n" + name.picked("                ", "xo", terms, false) + fmt("                gs_dot_acc(acc, xo, @d@_@);\n            }\n", tag, round_no, k);
            }
            s += "            const fe xr = gs_dot_end(acc);\n";
            if (spread) emit_exchange(s, name, "xr", members);
            else s += "            " + name(members[0]) + " = xr;\n";
            s += "        }\n";
            round_no++;
        }
        // everything cheap of this depth, in program order
        for (int id = 0; id < (int)nodes.size(); id++) {
            const SsaNode &n = nodes[id];
            if (n.depth != depth) continue;
            switch (n.kind) {
                case SsaNode::STATICV:
                    // the value of the NEXT step is requested now and used one iteration later: nothing hides a load's latency here
                    hoisted += fmt("    fe @q@ = @;\n", tag, id, jit_static_at(p, n.a, "(g * seglen)"));
                    s += fmt("        const fe @ = @q@;\n        @q@ = @;\n", name(id), tag, id, tag, id, jit_static_at(p, n.a, fmt("(@ + 1ull)", index)));
                    break;
                case SsaNode::ADD: s += name.binary(id, "fe_add"); break;
                case SsaNode::SUB: s += name.binary(id, "fe_sub"); break;
                case SsaNode::BLEND: s += name.binary(id, "gs_blend"); break;
                case SsaNode::OUT: s += fmt("        @@ = @;\n", sink, n.aux, name(n.a)); break;
                default: break;
            }
        }
    }
}

inline bool jit_trace_source(std::string &s, JitGen &gen, const AirProgram &p, const AirProgram &init) {
    const JitFlavour &fl = gen.fl;
    s = jit_preamble(fl);
    const uint32_t registers = p.registers, init_ninstr = init.ninstr;
    std::vector<SsaNode> main_nodes, init_nodes;
    if (!ssa_build(main_nodes, gen, p, true)) return false;
    if (init_ninstr && !ssa_build(init_nodes, gen, init, false)) return false;
    ssa_fuse_dots(main_nodes);
    ssa_fuse_dots(init_nodes);
    ssa_align_pows(main_nodes);
    ssa_align_pows(init_nodes);
    gen.lanes = std::max(ssa_lanes(fl, main_nodes), ssa_lanes(fl, init_nodes));
    s += fmt("#define GS_LANES @u\n", gen.lanes);
    s += "extern \"C\" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void gs_jit_trace(const fe *__restrict__ " + jit_arg(fl, "consts") +
         ", const fe *__restrict__ " + jit_arg(fl, "statics") + ", const fe *__restrict__ " + jit_arg(fl, "first_rows") + ",\n"
         "                                         unsigned long long segments, unsigned long long seglen, fe *__restrict__ out) {\n" +
         jit_wrap(fl, "consts") + jit_wrap(fl, "statics") + jit_wrap(fl, "first_rows") +
         "    const unsigned long long tid = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x;\n"
         "    // every thread runs every step (and reaches every barrier): the lanes past the last segment recompute it and store nothing\n"
         "    const bool gs_live = tid / GS_LANES < segments;\n"
         "    const unsigned long long g = gs_live ? tid / GS_LANES : segments - 1ull;\n"
         "    const unsigned int sub = (unsigned int)(tid % GS_LANES);\n"
         "    // results of a round change lanes through LDS: one 16-byte write per lane, one read per result (a block is one wave:\n"
         "    // the barriers only order the accesses)\n"
         "    __shared__ fe gs_swap[64];\n"
         "    const unsigned int gs_group = threadIdx.x & ~(GS_LANES - 1u);\n"
         "    const unsigned long long steps = segments * seglen;\n";
    for (uint32_t r = 0; r < registers; r++) s += fmt("    fe r@ = first_rows[g * @ull + @ull], n@;\n", r, registers, r, r);
    std::string to_next, to_row;      // n<r> = r<r>; before a block of the program, r<r> = n<r>; after it
    for (uint32_t r = 0; r < registers; r++) { to_next += fmt("        n@ = r@;\n", r, r); to_row += fmt("        r@ = n@;\n", r, r); }
    std::vector<bool> const_declared(p.nconsts, false);
    std::string hoisted, init_body, main_body;
    if (init_ninstr) ssa_emit(init_body, hoisted, const_declared, init_nodes, fl, init, gen.lanes, "0ull", "n", "u");
    ssa_emit(main_body, hoisted, const_declared, main_nodes, fl, p, gen.lanes, "i", "n", "v");
    s += hoisted;
    if (init_ninstr) s += "    {\n" + to_next + init_body + to_row + "    }\n";
    s += "    for (unsigned long long k = 0; k < seglen; k++) {\n"
         "        const unsigned long long i = g * seglen + k;\n";
    for (uint32_t r = 0; r < registers; r++) s += fmt("        if (gs_live && sub == @u) out[@ull * steps + i] = r@;\n", r % gen.lanes, r, r);
    s += "        if (k + 1 == seglen) break;\n" + to_next + main_body + to_row + "    }\n}\n";
    return true;
}

// ---- constraints -----------------------------------------------------------------------------------------------------------------
// A constraint program whose linear layers fuse (ssa_fuse_dots) is emitted from its SSA form, node by node: one thread per domain
// point, no lanes.  A fused row is K x 25 v_mad into nine shared columns and ONE fold (gs_dot9: the constants are lane-uniform, their
// limbs come out of scalar loads) instead of K products of 84 instructions and K - 1 additions: the 36 MDS products of a Poseidon
// round are 6 x ~300 instructions instead of 36 x 84 + 30 x 12.
inline void ssa_emit_flat(std::string &s, const std::vector<SsaNode> &nodes, const JitFlavour &fl, const AirProgram &p) {
    const SsaNames name{nodes, "v"};
    for (int id = 0; id < (int)nodes.size(); id++) {
        const SsaNode &n = nodes[id];
        switch (n.kind) {
            case SsaNode::ROW: s += fmt("        const fe v@ = p[@ull * prow + jp];\n", id, n.a); break;
            case SsaNode::ROWN: s += fmt("        const fe v@ = p[@ull * prow + jnp];\n", id, n.a); break;
            case SsaNode::STATICV: s += fmt("        const fe v@ = @;\n", id, jit_static_at(p, n.a, "j")); break;
            case SsaNode::ADD: s += name.binary(id, "fe_add"); break;
            case SsaNode::SUB: s += name.binary(id, "fe_sub"); break;
            case SsaNode::MUL: s += name.binary(id, "gs_mul"); break;
            case SsaNode::POWSHORT: case SsaNode::POWLONG:
                s += fmt("        fe @ = @;\n        {\n", name(id), name(n.a));
                emit_pow(s, fl, name(id), jit_exponent(fl, p, n.kind == SsaNode::POWLONG, n.aux));
                s += "        }\n";
                break;
            case SsaNode::DOT:
                s += fmt("        fe @;\n        {\n            gs_dot9_t acc;\n            gs_dot9_begin(acc);\n", name(id));
                for (size_t k = 0; k < n.tx.size(); k++) {
                    if (k && k % 6 == 0) s += "            gs_dot9_flush(acc);\n";
                    s += fmt("            gs_dot9_acc(acc, @, @);\n", name(n.tx[k]), n.tc[k] < 0 ? std::string("fe_one()") : fmt("consts[@]", n.tc[k]));
                }
                s += fmt("            @ = gs_dot9_end(acc);\n        }\n", name(id));
                break;
            case SsaNode::OUT: s += fmt("        out[@ull * nc + j] = @;\n", n.aux, name(n.a)); break;
            default: break;      // CONSTV / ZERO are named in place, DEAD nodes were absorbed
        }
    }
}

inline bool jit_constraints_source(std::string &s, const JitFlavour &fl, const AirProgram &p) {
    s = jit_preamble(fl);
    const uint32_t *const code = p.code, ninstr = p.ninstr;
    // register r at point j is p[r * prow + j * pstride]: the columns may be those of a larger domain read with a stride (the composition
    // domain inside the evaluation domain: gs_air_constraints_strided) — no plucked copy of the trace extension
    s += "extern \"C\" __global__ __launch_bounds__(128) void gs_jit_constraints(const fe *__restrict__ " + jit_arg(fl, "consts") + ", const fe *__restrict__ " +
         jit_arg(fl, "p") + ", unsigned long long nc,\n"
         "                                               unsigned long long shift, const fe *__restrict__ " + jit_arg(fl, "statics") + ", fe *__restrict__ out,\n"
         "                                               unsigned long long prow, unsigned long long pstride) {\n" +
         jit_wrap(fl, "consts") + jit_wrap(fl, "p") + jit_wrap(fl, "statics");
    for (uint32_t t = 0; t < p.vm_regs; t++) s += fmt("    fe t@;\n", t);
    s += "    for (unsigned long long j = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; j < nc; j += (unsigned long long)gridDim.x * blockDim.x) {\n"
         "        unsigned long long jn = j + shift;\n"
         "        if (jn >= nc) jn -= nc;\n"
         "        const unsigned long long jp = j * pstride, jnp = jn * pstride;\n";
    {   // linear layers present: the SSA route with fused rows (everything else: the register-by-register generator below)
        std::vector<SsaNode> nodes;
        if (ssa_build(nodes, JitGen{fl}, p, true, true)) {
            ssa_fuse_dots(nodes);
            if (std::any_of(nodes.begin(), nodes.end(), [](const SsaNode &n) { return n.kind == SsaNode::DOT; })) {
                ssa_emit_flat(s, nodes, fl, p);
                s += "    }\n}\n";
                return true;
            }
        }
    }
    // loads of trace registers and outputs are memory operations here: rewrite them on the fly
    for (uint32_t pc = 0; pc < ninstr; pc++) {
        const uint32_t op = code[4 * pc], d = code[4 * pc + 1], a = code[4 * pc + 2];
        if (op == OP_LOADR) s += fmt("        t@ = p[@ull * prow + jp];\n", d, a);
        else if (op == OP_LOADN) s += fmt("        t@ = p[@ull * prow + jnp];\n", d, a);
        else if (op == OP_OUT) s += fmt("        out[@ull * nc + j] = t@;\n", d, a);
        else {
            // runs of arithmetic go through the common generator (so that exponentiation groups are found)
            uint32_t end = pc;
            while (end < ninstr && code[4 * end] != OP_LOADR && code[4 * end] != OP_LOADN && code[4 * end] != OP_OUT) end++;
            if (!jit_body(s, fl, p, code + 4 * pc, end - pc, true, "r", nullptr, "j", "n")) return false;
            pc = end - 1;
        }
    }
    s += "    }\n}\n";
    return true;
}

// everything of a program the generated source depends on (the init block shares all but its instructions)
inline void jit_key_add(std::string &k, const void *p, size_t n) { const uint64_t len = n; k.append((const char *)&len, 8); if (n) k.append((const char *)p, n); }
inline std::string jit_key(const JitFlavour &fl, const char *kind, const AirProgram &p, const AirProgram *init) {
    std::string key(kind);
    jit_key_add(key, p.code, (size_t)p.ninstr * 16);
    if (init) jit_key_add(key, init->code, (size_t)init->ninstr * 16);
    jit_key_add(key, p.consts, (size_t)p.nconsts * fl.elt);
    jit_key_add(key, &p.sd, sizeof p.sd);
    const uint32_t shape[3] = {p.vm_regs, p.registers, p.nstatic};
    jit_key_add(key, shape, sizeof shape);
    return key;
}
