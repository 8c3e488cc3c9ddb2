// air_program_host.cpp — the validator of csrc/air_program.h (with the static-layout builder) as a filter, so that
// tests/test_air_program_header.py can put a table of malformed programs through it on machines without a GPU, also in a build with
// -fsanitize=address,undefined.  Build: g++ -O2 -std=c++17 tests/host_harness/air_program_host.cpp (no field arithmetic: one flavour)
// stdin, per program (numbers decimal, white space between tokens):
//   prog <kind: trace|constraints> <ninstr> <init_ninstr> <nconsts> <vm_regs> <registers> <nstatic> <nout>
//   4 * ninstr code words, 4 * init_ninstr words, nstatic table lengths
// stdout, per program: "ok" or "refused <message>".
#include <stdio.h>
#include <stdint.h>
#include <string.h>

#include <vector>
#include "../../genstark_amd/csrc/air_program.h"

static bool read_u(uint64_t &v) { unsigned long long x; if (scanf("%llu", &x) != 1) return false; v = x; return true; }
static std::vector<uint32_t> read_words(size_t n) {
    std::vector<uint32_t> w(n ? n : 1);
    uint64_t v;
    for (size_t i = 0; i < n && read_u(v); i++) w[i] = (uint32_t)v;
    return w;
}
int main() {
    static char word[32], kind[32];
    while (scanf("%31s", word) == 1) {
        if (strcmp(word, "prog") != 0) { printf("unexpected token %s\n", word); return 1; }
        uint64_t ninstr, init_ninstr, nconsts, vm_regs, registers, nstatic, nout;
        if (scanf("%31s", kind) != 1 || !read_u(ninstr) || !read_u(init_ninstr) || !read_u(nconsts) || !read_u(vm_regs) || !read_u(registers) ||
            !read_u(nstatic) || !read_u(nout)) return 1;
        const bool trace = strcmp(kind, "trace") == 0;
        const std::vector<uint32_t> code = read_words(4 * ninstr), icode = read_words(4 * init_ninstr);
        const std::vector<uint8_t> consts(nconsts * 32 + 1, 0);      // (the validator looks at no constant's value)
        std::vector<uint64_t> lens(nstatic ? nstatic : 1);
        for (uint64_t s = 0; s < nstatic; s++) read_u(lens[s]);
        AirProgram p{code.data(), (uint32_t)ninstr, consts.data(), (uint32_t)nconsts, (uint32_t)vm_regs, (uint32_t)registers, (uint32_t)nstatic, (uint32_t)nout};
        const AirProgram init = p.with_code(icode.data(), (uint32_t)init_ninstr);
        char msg[96] = "ok";
        bool ok = air_validate(p, !trace, true, msg, sizeof msg) && (!init_ninstr || air_validate(init, false, false, msg, sizeof msg));
        if (ok && !air_static_layout(lens.data(), p.nstatic, p.sd)) { ok = false; snprintf(msg, sizeof msg, "air program: empty static table"); }
        printf(ok ? "%s\n" : "refused %s\n", msg);
    }
    return 0;
}
