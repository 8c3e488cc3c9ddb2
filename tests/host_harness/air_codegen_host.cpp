// air_codegen_host.cpp — the code generator of csrc/air_codegen.h as a filter, for all six fixed field flavours in one program, so that
// tests/test_air_codegen_host.py can compare the sources it writes with recorded ones on machines without a GPU, also in a build with
// -fsanitize=address,undefined.  Nothing is compiled for the device.  Build: g++ -O2 -std=c++17 tests/host_harness/air_codegen_host.cpp
// stdin, per program (numbers decimal, white space between tokens; the first three lines after `flavour` are air_program_host.cpp's):
//   flavour <p128|q64|q32|q17|p256|p224>
//   prog <kind: trace|constraints> <ninstr> <init_ninstr> <nconsts> <vm_regs> <registers> <nstatic> <nout>
//   4 * ninstr code words, 4 * init_ninstr words, nstatic table lengths
//   consts <nconsts elements as hex digits, little-endian bytes | ->
//   statics <every table's elements likewise (trace programs: the selector rule reads them) | ->
// stdout, per program: "refused <message>" (the validator's: the generator never sees such a program), "declined" (the generator has no
// code for the program: it is interpreted) or "<sha-256 of the source> <lanes>".  With --source the source follows, then a line "----".
#include <stdio.h>
#include <stdint.h>
#include <string.h>

#include <vector>
#include "../../genstark_amd/csrc/air_codegen.h"
#include "../../genstark_amd/csrc/host_hash.h"

static const struct { const char *name; JitFlavour fl; } kFlavours[] = {
    {"p128", {16, true, false, ""}},
    {"q64", {16, false, false, "#define GS_SMALL_Q 18446744051160973313ull\n"}},
    {"q32", {16, false, false, "#define GS_SMALL_Q 4194304001ull\n"}},
    {"q17", {16, false, false, "#define GS_SMALL_Q 96769ull\n"}},
    {"p256", {32, false, true, "#define GS_WIDE_BITS 256\n"}},
    {"p224", {32, false, true, "#define GS_WIDE_BITS 224\n"}},
};

static bool read_u(uint64_t &v) { unsigned long long x; if (scanf("%llu", &x) != 1) return false; v = x; return true; }
static std::vector<uint32_t> read_words(size_t n) {
    std::vector<uint32_t> w(n ? n : 1);
    uint64_t v;
    for (size_t i = 0; i < n && read_u(v); i++) w[i] = (uint32_t)v;
    return w;
}
// "<label> <hex digits | ->": the bytes, padded with zeros to at least `least`; false: another label, or an odd digit
static bool read_bytes(const char *label, size_t least, std::vector<uint8_t> &out) {
    char word[32];
    if (scanf("%31s", word) != 1 || strcmp(word, label) != 0) return false;
    int c = getchar();
    while (c == ' ' || c == '\n') c = getchar();
    auto digit = [](int ch) { return ch >= '0' && ch <= '9' ? ch - '0' : (ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1); };
    for (; digit(c) >= 0; c = getchar()) {
        const int lo = getchar();
        if (digit(lo) < 0) return false;
        out.push_back((uint8_t)(16 * digit(c) + digit(lo)));
    }
    if (out.size() < least) out.resize(least, 0);
    return true;
}

int main(int argc, char **argv) {
    const bool print_source = argc > 1 && strcmp(argv[1], "--source") == 0;
    static char word[32], kind[32];
    while (scanf("%31s", word) == 1) {
        if (strcmp(word, "flavour") != 0 || scanf("%31s", word) != 1) { printf("unexpected token %s\n", word); return 1; }
        const JitFlavour *fl = nullptr;
        for (const auto &f : kFlavours) if (strcmp(f.name, word) == 0) fl = &f.fl;
        if (!fl || scanf("%31s", word) != 1 || strcmp(word, "prog") != 0) { printf("unexpected token %s\n", word); return 1; }
        uint64_t ninstr, init_ninstr, nconsts, vm_regs, registers, nstatic, nout;
        if (scanf("%31s", kind) != 1 || !read_u(ninstr) || !read_u(init_ninstr) || !read_u(nconsts) || !read_u(vm_regs) || !read_u(registers) ||
            !read_u(nstatic) || !read_u(nout)) return 1;
        const bool trace = strcmp(kind, "trace") == 0;
        const std::vector<uint32_t> code = read_words(4 * ninstr), icode = read_words(4 * init_ninstr);
        std::vector<uint64_t> lens(nstatic ? nstatic : 1);
        for (uint64_t s = 0; s < nstatic; s++) read_u(lens[s]);
        std::vector<uint8_t> consts, statics;
        if (!read_bytes("consts", nconsts * fl->elt, consts) || !read_bytes("statics", 0, statics)) { printf("unexpected bytes\n"); return 1; }
        AirProgram p{code.data(), (uint32_t)ninstr, consts.data(), (uint32_t)nconsts, (uint32_t)vm_regs, (uint32_t)registers, (uint32_t)nstatic, (uint32_t)nout};
        const AirProgram init = p.with_code(icode.data(), trace ? (uint32_t)init_ninstr : 0);
        char msg[96] = "";
        bool ok = air_validate(p, !trace, true, msg, sizeof msg) && (!init.ninstr || air_validate(init, false, false, msg, sizeof msg));
        uint64_t total = 0;
        if (ok && !air_static_layout(lens.data(), p.nstatic, p.sd, &total)) { ok = false; snprintf(msg, sizeof msg, "air program: empty static table"); }
        if (ok && !statics.empty() && statics.size() != total * fl->elt) { ok = false; snprintf(msg, sizeof msg, "the static tables' values do not fit their lengths"); }
        if (!ok) { printf("refused %s\n", msg); continue; }
        const AirProgram init_laid_out = p.with_code(init.code, init.ninstr);
        JitGen gen{*fl, 1, trace && !statics.empty() ? statics.data() : nullptr};
        std::string src;
        if (!(trace ? jit_trace_source(src, gen, p, init_laid_out) : jit_constraints_source(src, *fl, p))) { printf("declined\n"); continue; }
        (void)jit_key(*fl, trace ? "T" : "C", p, trace ? &init_laid_out : nullptr);      // reads everything a source depends on
        uint8_t d[32];
        host_sha256((const uint8_t *)src.data(), src.size(), d);
        for (int i = 0; i < 32; i++) printf("%02x", d[i]);
        printf(" %u\n", gen.lanes);
        if (print_source) printf("%s----\n", src.c_str());
    }
    return 0;
}
