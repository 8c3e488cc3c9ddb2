// air_program.h — what the native consumers of an AIR program (include/gstark.h, "AIR ... generic straight-line programs") must agree on,
// stated once: the opcodes, the decoder, the program as one value, the layout of the static registers, the validator and the grouping
// rule for exponentiations.  For the interpreters of air_vm.hip, the code generator of air_codegen.h and the verifier (verifier.h, built by
// g++).  Plain C++: no HIP runtime, no context.  What an instruction DOES stays with each interpreter: a shared executor compiled to the
// same kernel resources and ran the interpreted traces up to 10% slower (profiles/air_program.md).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/gstark.h"

enum { OP_LOADC = 0, OP_LOADR = 1, OP_LOADN = 2, OP_LOADS = 3, OP_ADDV = 4, OP_SUBV = 5, OP_MULV = 6, OP_POW = 7, OP_POWC = 8, OP_OUT = 9 };

struct AirIns { uint32_t op, dst, a, b; };
inline AirIns air_decode(const uint32_t *code, uint32_t pc) { return AirIns{code[4 * pc], code[4 * pc + 1], code[4 * pc + 2], code[4 * pc + 3]}; }

// static register s of a program: elements [offset[s], offset[s] + len[s]) of the concatenated table, read cyclically
struct StaticDesc {
    uint64_t offset[GS_AIR_MAX_REGISTERS];  // element offset into the concatenated table
    uint64_t len[GS_AIR_MAX_REGISTERS];
};
// lengths -> layout (registers past nstatic: length 1, so that no reader divides by zero); false: too many tables, or an empty one
template <class Len>
inline bool air_static_layout(const Len *lens, uint32_t nstatic, StaticDesc &sd, uint64_t *total = nullptr) {
    if (nstatic > GS_AIR_MAX_REGISTERS) return false;
    uint64_t off = 0;
    for (uint32_t s = 0; s < GS_AIR_MAX_REGISTERS; s++) {
        sd.offset[s] = off;
        sd.len[s] = s < nstatic ? lens[s] : 1;
        if (s < nstatic && !lens[s]) return false;
        if (s < nstatic) off += lens[s];
    }
    if (total) *total = off;
    return true;
}

// a program with everything it is checked against and translated with (host pointers; the constants as nconsts elements of the ABI)
struct AirProgram {
    const uint32_t *code = nullptr;
    uint32_t ninstr = 0;
    const uint8_t *consts = nullptr;
    uint32_t nconsts = 0, vm_regs = 0, registers = 0, nstatic = 0;
    uint32_t nout = 0;          // OUT destinations: next-row registers of a trace program, constraints of an evaluator
    StaticDesc sd = {};         // of the nstatic static registers (air_static_layout)
    AirIns at(uint32_t pc) const { return air_decode(code, pc); }
    // the `init { ... }` block of a trace program: same pool, same scratch file, other instructions
    AirProgram with_code(const uint32_t *c, uint32_t n) const { AirProgram p = *this; p.code = c; p.ninstr = n; return p; }
};
// Is the program well formed?  allow_next: LOADN (constraint evaluators); allow_statics: LOADS (not in an init block).  false: `msg`
// says why, naming the first offending instruction.
inline bool air_validate(const AirProgram &p, bool allow_next, bool allow_statics, char *msg, size_t cap) {
    const uint32_t vm = p.vm_regs;
    if (!p.code || !p.ninstr) { snprintf(msg, cap, "air program: empty"); return false; }
    if (vm == 0 || vm > GS_AIR_MAX_VM_REGS) { snprintf(msg, cap, "air program: vm_regs must be in 1..%d", GS_AIR_MAX_VM_REGS); return false; }
    if (p.registers == 0 || p.registers > GS_AIR_MAX_REGISTERS || p.nstatic > GS_AIR_MAX_REGISTERS) { snprintf(msg, cap, "air program: too many registers"); return false; }
    for (uint32_t pc = 0; pc < p.ninstr; pc++) {
        const AirIns i = p.at(pc);
        bool ok = true;
        switch (i.op) {
            case OP_LOADC: ok = i.dst < vm && i.a < p.nconsts; break;
            case OP_LOADR: ok = i.dst < vm && i.a < p.registers; break;
            case OP_LOADN: ok = allow_next && i.dst < vm && i.a < p.registers; break;
            case OP_LOADS: ok = allow_statics && i.dst < vm && i.a < p.nstatic; break;
            case OP_ADDV: case OP_SUBV: case OP_MULV: ok = i.dst < vm && i.a < vm && i.b < vm; break;
            case OP_POW: ok = i.dst < vm && i.a < vm; break;
            case OP_POWC: ok = i.dst < vm && i.a < vm && i.b < p.nconsts; break;
            case OP_OUT: ok = i.dst < p.nout && i.a < vm; break;
            default: ok = false;
        }
        if (!ok) { snprintf(msg, cap, "air program: invalid instruction %u (op %u)", pc, i.op); return false; }
    }
    return true;
}

// How many exponentiations form a group at pc (a POW or POWC): adjacent ones with the same opcode and exponent whose results do not
// feed each other — no source is an earlier member's result — (the compiler puts the S-boxes of a round next to each other), at most four
inline uint32_t air_pow_group(const uint32_t *code, uint32_t ninstr, uint32_t pc) {
    const AirIns first = air_decode(code, pc);
    uint32_t g = 1;
    while (g < 4 && pc + g < ninstr) {
        const AirIns nx = air_decode(code, pc + g);
        bool ok = nx.op == first.op && nx.b == first.b;
        for (uint32_t i = 0; ok && i < g; i++) ok = nx.a != air_decode(code, pc + i).dst;
        if (!ok) break;
        g++;
    }
    return g;
}
