"""AIR programs for the register machine of include/gstark.h, with a model of that machine on Python integers.

The machine has four native implementations, each with optimisations of its own (the code generator of csrc/air_codegen.h, the device
interpreters of csrc/air_vm.hip, its host_run and the verifier's run_program) beside the oracle's loop; what they must agree on before
they run — opcodes, validator, static layout, grouping rule — is stated once in csrc/air_program.h.  This module holds what
tests/test_air_programs.py and tests/test_air_program_header.py compare them with and on:
  - run_trace / run_constraints: the machine written straight from the header's comment (about forty lines);
  - one builder per branch of the generator and the interpreters (targeted_programs, constraint_programs);
  - a seeded generator of programs at instruction level (generated_program);
  - runners for a backend (trace_on, constraints_on) and for the compile-only hook (generated_source);
  - chain_exponent: the exponent an emitted addition chain computes, followed on integers."""
import ctypes as C
import random
import re
from types import SimpleNamespace

from conftest import rand_elements
from field_corners import FIXED, cases_for, edge_list, product_pairs

LOADC, LOADR, LOADN, LOADS, ADD, SUB, MUL, POW, POWC, OUT = range(10)
FLAVOURS = {name: FIXED[name] for name in ('p128', 'q64', 'p224')}       # name -> (modulus, bits): the flavours the device tests run (the builders take any of FIXED)
HOST_SEGMENTS = 8           # GS_HOST_TRACE_MAX_SEGMENTS: traces of at most this many segments run on a host core, whatever the JIT mode


# ---- 1. the model ---------------------------------------------------------------------------------------------------------------
class UndefinedRead(Exception):
    """The program reads a scratch register that this execution has not written: the implementations keep stale values there."""


def _execute(code, consts, q, cur, nxt, static, out):
    vm = {}                                             # cleared before every execution

    def rd(r):
        if r not in vm:
            raise UndefinedRead(f't{r} is read before it is written')
        return vm[r]
    for op, d, a, b in code:
        if op == LOADC: vm[d] = consts[a] % q
        elif op == LOADR: vm[d] = cur(a)
        elif op == LOADN: vm[d] = nxt(a)
        elif op == LOADS: vm[d] = static(a)
        elif op == ADD: vm[d] = (rd(a) + rd(b)) % q
        elif op == SUB: vm[d] = (rd(a) - rd(b)) % q
        elif op == MUL: vm[d] = rd(a) * rd(b) % q
        elif op == POW: vm[d] = pow(rd(a), b, q)
        elif op == POWC: vm[d] = pow(rd(a), consts[b], q)
        elif op == OUT: out[d] = rd(a)                  # in program order: the last write to a destination wins
        else: raise ValueError(f'opcode {op}')


def _no(_):
    raise ValueError('the program loads what this kind of program does not have')


def run_trace(code, init_code, consts, statics, first_rows, segments, seglen, q):
    """gs_air_trace_segments: registers x (segments * seglen) values, row-major."""
    registers, steps = len(first_rows[0]), segments * seglen
    out = [0] * (registers * steps)
    for g in range(segments):
        row = [v % q for v in first_rows[g]]
        if init_code:
            nxt = list(row)
            _execute(init_code, consts, q, lambda a: row[a], _no, _no, nxt)
            row = nxt
        for k in range(seglen):
            i = g * seglen + k
            for r in range(registers):
                out[r * steps + i] = row[r]
            if k + 1 == seglen:
                break
            nxt = list(row)                             # a register without an OUT keeps the current row's value
            _execute(code, consts, q, lambda a: row[a], _no, lambda s: statics[s][i % len(statics[s])] % q, nxt)
            row = nxt
    return out


def run_constraints(code, consts, columns, prow, pstride, nc, shift, tables, q):
    """gs_air_constraints_strided: constraints x nc values, row-major; register r at point j is columns[r * prow + j * pstride]."""
    nout = 1 + max(d for op, d, a, b in code if op == OUT)
    out = [0] * (nout * nc)
    for j in range(nc):
        jn = (j + shift) % nc
        res = {}
        _execute(code, consts, q, lambda a: columns[a * prow + j * pstride] % q, lambda a: columns[a * prow + jn * pstride] % q,
                 lambda s: tables[s][j % len(tables[s])] % q, res)
        for d, v in res.items():
            out[d * nc + j] = v
    return out


# ---- 2. writing programs ---------------------------------------------------------------------------------------------------------
class Asm:
    """Instructions, a constant pool and a free list of scratch registers."""

    def __init__(self, vm_regs=64):
        self.code, self.consts, self.free, self.top = [], [], list(range(vm_regs)), 0

    def const(self, v):
        self.consts.append(v)
        return len(self.consts) - 1

    def rel(self, *ts):
        self.free = sorted(set(self.free) | set(ts))

    def ins(self, op, a=0, b=0, d=None):
        if d is None:
            d = self.free.pop(0)
        self.top = max(self.top, d + 1)
        self.code.append((op, d, a, b))
        return d

    def loadc(self, v, d=None): return self.ins(LOADC, self.const(v), d=d)
    def loadk(self, index, d=None): return self.ins(LOADC, index, d=d)
    def loadr(self, r, d=None): return self.ins(LOADR, r, d=d)
    def loadn(self, r, d=None): return self.ins(LOADN, r, d=d)
    def loads(self, s, d=None): return self.ins(LOADS, s, d=d)
    def add(self, x, y, d=None): return self.ins(ADD, x, y, d)
    def sub(self, x, y, d=None): return self.ins(SUB, x, y, d)
    def mul(self, x, y, d=None): return self.ins(MUL, x, y, d)
    def pow(self, x, e, d=None): return self.ins(POW, x, e, d)
    def powk(self, x, index, d=None): return self.ins(POWC, x, index, d)

    def mulc(self, x, v):
        k = self.loadc(v)
        return self.mul(x, k, d=k)

    def out(self, dst, x, rel=False):
        self.code.append((OUT, dst, x, 0))
        if rel:
            self.rel(x)

    def row(self, terms, pooled=False):
        """sum of x * c over terms (x, c); c None: the leaf rides along by one; pooled: c is an index into the constant pool.
        A left-leaning chain of ADDs whose inner sums have one user each: what ssa_fuse_dots takes for the row of a linear layer."""
        acc, acc_own = None, False
        for x, c in terms:
            if c is None:
                t, own = x, False
            else:
                k = self.loadk(c) if pooled else self.loadc(c)
                t, own = self.mul(x, k, d=k), True
            if acc is None:
                acc, acc_own = t, own
                continue
            d = acc if acc_own else (t if own else None)
            new = self.add(acc, t, d=d)
            if own and d != t:
                self.rel(t)
            acc, acc_own = new, True
        return acc


def corner_values(q):
    """q - 1 and the edges of tests/field_corners.py, with operands of its corner products (the rare carries of the field's reduction)."""
    bits = [b for m, b in FIXED.values() if m == q][0]
    pairs = product_pairs(cases_for(q, bits))
    step = max(1, len(pairs) // 24)
    return edge_list(q, bits) + [v for pair in pairs[::step] for v in pair]


def first_rows(q, registers, segments, seed):
    rng, ev = random.Random(seed), corner_values(q)
    fixed = [[q - 1] * registers, [0] * registers, [1] * registers, [q - 2] * registers]
    return [fixed[s] if s < 4 else [rng.choice(ev) if rng.random() < 0.5 else rng.randrange(q) for _ in range(registers)] for s in range(segments)]


def trace_prog(name, q, a, registers, seglen=5, segment_counts=(9,), statics=(), init=None, expect=(), vm_regs=None, seed=1):
    p = SimpleNamespace(name=name, kind='trace', q=q, code=a.code, consts=a.consts, registers=registers, seglen=seglen,
                        segment_counts=tuple(dict.fromkeys(segment_counts)), statics=[list(s) for s in statics], init=(init.code if init else []),
                        expect=tuple(expect), vm_regs=vm_regs or max(a.top, init.top if init else 0), seed=seed)
    if init:
        assert init.consts is a.consts, 'the init block shares the constant pool'
    p.rows = lambda segments: first_rows(q, registers, segments, seed)
    return p


def long_exponents(q, bits):
    """name -> exponent: every chain shape of emit_pow away from Rescue's one exponent."""
    rng = random.Random(0x65787073 ^ q)

    def run(k, p3):      # a leading "10" run of k pairs, then runs the dictionary serves, and "11" with trailing zeros or a last single "1"
        return int('10' * k + '0' + '10' * k + '00' + '10' * (k - 1) + ('11' + '10' * 3 + '000' if p3 else '00' + '10' * 3 + '0001'), 2)
    return {'inv_cube': (2 * q - 1) // 3, 'fermat': q - 2, 'top_bit': 2**(bits - 1), 'random': rng.randrange(2**(bits - 1), q),
            'run7_p3': run(7, True), 'run7': run(7, False), 'run8_p3': run(8, True), 'run8': run(8, False)}


# ---- 2a. targeted trace programs: one builder per branch ---------------------------------------------------------------------------
def rows_program(q, bits):
    """Fused rows of 2, 6, 7, 12, 13 and 24 terms in one layer, more rows than lanes, maximal operands: the fold every six terms.
    What the fold is there for: a term adds up to 4.25 * 2^52 to a 64-bit column (x = q - 2 times the constant q - 1: the first rows of
    segment 3; 3.25 * 2^52 for x = q - 1, segment 0), and the carry out of a column is exact below 2^57 = 32 * 2^52.  Six terms reach 25.5,
    seven 29.75 (a fold every seven terms computes the same values), eight 34: the rows of 12 and 24 terms by q - 1 alone lose their
    carries when the fold comes every eight terms or not at all."""
    a, regs = Asm(), 8
    x = [a.loadr(r) for r in range(regs)]
    ev = [q - 1] + corner_values(q)
    ys = []
    for j, K in enumerate((2, 6, 7, 12, 13, 24, 7, 13, 24, 2)):
        # three of the rows: every constant q - 1 (with a first row of q - 1 everywhere every term is (q - 1)^2, the columns' maximum)
        terms = [(x[(j + k) % regs], q - 1 if j in (2, 3, 5) else ev[(5 * j + k) % len(ev)]) for k in range(K)]
        if j == 6:
            terms[3] = (x[3], None)                     # a leaf that is no product: rides along by one
        if j == 7:
            terms[5] = (a.loadc(q - 1), None)           # the row's additive constant
        ys.append(a.row(terms))
    for r in range(6):
        a.out(r, ys[r])
    a.out(6, a.mul(ys[6], ys[7]))
    a.out(7, a.sub(ys[8], ys[9]))
    return trace_prog('rows', q, a, regs, segment_counts=(9, 17), expect=('#define GS_LANES 8u', 'gs_dot_flush(acc);', 'fe_one()'))


def lanes_program(q, bits, widest):
    """`widest` independent products at the widest depth -> 1, 2, 4, 8 or 16 lanes; more registers than lanes; segment counts that leave
    the last wave and the last lane group partly filled."""
    lanes = {1: 1, 2: 2, 4: 4, 5: 8, 12: 16}[widest]
    a, regs = Asm(), lanes + 3
    x = [a.loadr(r) for r in range(regs)]
    p1 = [a.mul(x[i], x[i + 1]) for i in range(widest)]
    p2 = [a.mul(p1[i], p1[(i + 1) % widest]) for i in range(max(1, widest - 1))]     # a round with fewer products than lanes
    for i in range(len(p2)):
        a.out(i, a.add(p2[i], x[regs - 1]))
    a.out(regs - 2, a.add(x[regs - 2], p1[-1]))
    per_wave = 64 // lanes
    return trace_prog(f'lanes{lanes}', q, a, regs, seglen=3, segment_counts=(9, per_wave - 1, per_wave + 1, 2 * per_wave + 1),
                      expect=(f'#define GS_LANES {lanes}u',))


def rounds_program(q, bits):
    """Depth 1: sixteen products by constants (one full round), then three squares (a last group smaller than the lanes); depth 2: one
    round of constants and variables mixed."""
    a, regs = Asm(), 20
    ev = corner_values(q)
    x = [a.loadr(r) for r in range(regs)]
    byc = [a.mulc(x[i], ev[(3 * i + 1) % len(ev)]) for i in range(16)]
    sq = [a.mul(x[i], x[i]) for i in (16, 17, 18)]
    mixed = [a.mulc(byc[0], q - 1), a.mul(byc[1], byc[2]), a.mul(sq[0], sq[0]), a.mulc(sq[1], q - 2), a.mul(byc[3], sq[2])]
    for i in range(5):
        a.out(i, mixed[i])
    for i in range(5, 16):
        a.out(i, a.sub(byc[i], x[19]), rel=True)
    a.out(16, sq[0])
    a.out(17, a.sub(sq[1], sq[2]))
    return trace_prog('rounds', q, a, regs, seglen=3, segment_counts=(9, 13),
                      expect=('#define GS_LANES 16u', 'const fe xr = gs_sqr(xa);', 'const fe vk0 = consts[', 'const fe xr = gs_mul(xa, xb);'))


def short_exponents_program(q, bits):
    """POW by 0, 1, 2, 3, 5, 7, 2^31 and 2^32 - 1, POWC with a 32-bit exponent; bases 0, 1 and q - 1 (the first rows of segments 1, 2, 0);
    adjacent POWs with one exponent in twos and threes (the interpreter's interleaved groups)."""
    a = Asm()
    exps = (0, 1, 2, 3, 5, 7, 2**31, 2**32 - 1)
    regs = len(exps) + 1 + 5
    x = [a.loadr(r) for r in range(regs)]
    res = [a.pow(x[i], e) for i, e in enumerate(exps)]
    res.append(a.powk(x[8], a.const(0xdeadbeef)))
    res += [a.pow(x[9], 5), a.pow(x[10], 5)]            # a group of two
    res += [a.pow(x[11], 7), a.pow(x[12], 7), a.pow(x[13], 7)]       # a group of three
    for i, v in enumerate(res):
        a.out(i, a.add(v, x[(i + 1) % regs]))
    return trace_prog('short_exponents', q, a, regs, seglen=3, segment_counts=(9, 33), expect=('lz_sqr(acc, K)', 'fe_one()'))


def long_exponents_program(q, bits):
    """POWC by every long exponent of long_exponents(): canonical and lazy windows, the pattern chain with and without p3."""
    a = Asm()
    es = long_exponents(q, bits)
    x = [a.loadr(r) for r in range(len(es))]
    for i, e in enumerate(es.values()):
        a.out(i, a.add(a.powk(x[i], a.const(e)), x[(i + 1) % len(es)]))
    return trace_prog('long_exponents', q, a, len(es), seglen=3, segment_counts=(9, 12),
                      expect=('const lz g1 = lz_sqr(p1, K);', 'const lz p3 = lz_mul_v(g1, p1, K);', 'const lz p2 = lz_sqr(p1, K);'))


def pow_groups_program(q, bits):
    """Adjacent same-exponent groups of 2, 3, 4 and 5 long exponentiations (the interpreter's 4-lane mode with exponents other than
    Rescue's; the generator's one-member-per-lane rounds); two equal exponents at different depths, and two that depend on each other."""
    a = Asm()
    es = long_exponents(q, bits)
    sizes = {'run8': 2, 'random': 3, 'top_bit': 4, 'inv_cube': 5}
    regs = sum(sizes.values()) + 4
    x = [a.loadr(r) for r in range(regs)]
    res, r = [], 0
    for name, n in sizes.items():
        k = a.const(es[name])
        res += [a.powk(x[r + i], k) for i in range(n)]
        r += n
    k = a.const(es['fermat'])
    first = a.powk(x[r], k)                             # depth 1
    later = a.powk(a.mul(x[r + 1], x[r + 2]), k)        # depth 2, independent of `first`: ssa_align_pows puts them in one round
    chained = a.powk(a.add(first, x[r + 3]), k)         # depends on `first`
    res += [first, later, chained]
    for i, v in enumerate(res):
        a.out(i, a.add(v, x[(i + 1) % regs]))
    return trace_prog('pow_groups', q, a, regs, seglen=3, segment_counts=(9, 18), expect=('#define GS_LANES 16u', 'x = gs_pick(sub == 4u'))


def statics_program(q, bits):
    """Static registers of periods 1, 2, 3, 8 and 64 with segments of 5 steps (they start in mid-period); 0/1 tables times a value, times
    another 0/1 table, and used twice."""
    ev = corner_values(q)
    rng = random.Random(0x73746174)
    statics = [[rng.choice(ev) for _ in range(n)] for n in (1, 2, 3, 8, 64)] + [[1, 0, 0, 1, 1, 0, 1, 0], [0, 1, 1]]
    a, regs = Asm(), 8
    x = [a.loadr(r) for r in range(regs)]
    s = [a.loads(i) for i in range(len(statics))]
    a.out(0, a.mul(x[0], s[5]))                         # a value times a selector
    a.out(1, a.add(a.mul(s[5], s[6]), x[1]))            # a selector times a selector
    a.out(2, a.mul(a.loads(5), x[2]))                   # the selector again, loaded again
    a.out(3, a.add(x[3], s[0]))
    a.out(4, a.mul(x[4], s[1]))                         # not a selector: a product
    a.out(5, a.add(a.mul(x[5], s[2]), s[2]))            # period 3, used twice
    a.out(6, a.add(a.mul(x[6], s[4]), s[3]))
    a.out(7, a.sub(x[7], a.mul(s[6], x[0])))
    return trace_prog('statics', q, a, regs, seglen=5, segment_counts=(9, 33), statics=statics, expect=('= gs_blend(', '% 3ull', '& 63ull'))


def outputs_program(q, bits):
    """A register left unwritten, a swap, an OUT of a constant, an OUT of x^1."""
    a, regs = Asm(), 6
    x = [a.loadr(r) for r in range(regs)]
    a.out(0, x[1])
    a.out(1, x[0])
    a.out(2, a.loadc(q - 1))
    a.out(3, a.pow(a.add(x[3], x[4]), 1))
    a.out(4, a.mul(x[4], x[5]))                         # register 5 keeps its value
    return trace_prog('outputs', q, a, regs, seglen=4, segment_counts=(9,))


def two_outs_program(q, bits):
    """LOADR t0,r0; MUL t1,t0,t0; OUT 0,t1; OUT 0,t0: the second OUT is the shallower one, and it is the one that counts."""
    a = Asm()
    t0 = a.loadr(0)
    t1 = a.mul(t0, t0)
    a.out(0, t1)
    a.out(0, t0)
    a.out(1, a.mul(a.loadr(1), t1))
    return trace_prog('two_outs', q, a, 2, seglen=4, segment_counts=(9,))


def init_program(q, bits, seglen=4):
    """An init block with a product, a short power and a fusable row."""
    a = Asm()
    init = Asm()
    init.consts = a.consts
    regs = 4
    y = [init.loadr(r) for r in range(regs)]
    init.out(0, init.mul(y[0], y[1]))
    init.out(1, init.pow(y[1], 3))
    init.out(2, init.row([(y[0], q - 1), (y[1], 3), (y[2], q - 2), (y[3], None)]))
    x = [a.loadr(r) for r in range(regs)]
    for r in range(regs):
        a.out(r, a.add(a.mul(x[r], x[(r + 1) % regs]), a.loadc(q - 1 - r)))
    return trace_prog(f'init_seglen{seglen}', q, a, regs, seglen=seglen, segment_counts=(9,), init=init, expect=('gs_dot_acc(acc, ', 'gs_dotk ud'))


def shape_program(q, bits, vm_regs, registers, segment_counts=(9,), seglen=3):
    """registers x vm_regs at the limits and on both sides of the interpreter's 160 KiB rule ((vm_regs + 2 registers) * 64 elements of
    LDS, private arrays <16|32|64> beyond); every scratch register is used."""
    a = Asm(vm_regs)
    if vm_regs == 1:
        for r in range(registers):
            a.loadr(r, d=0)
            a.mul(0, 0, d=0)
            a.out(r, 0)
    else:
        c = a.const(q - 1)
        for r in range(registers):
            t, u = (2 * r) % (vm_regs - 1), (2 * r) % (vm_regs - 1) + 1
            a.loadr(r, d=t)
            a.loadr((r + 1) % registers, d=u)
            a.mul(t, u, d=u)
            a.loadk(c, d=t)
            a.add(t, u, d=t)
            a.out(r, t)
        a.top = vm_regs
    return trace_prog(f'shape_vm{vm_regs}_r{registers}', q, a, registers, seglen=seglen, segment_counts=segment_counts, vm_regs=vm_regs)


def targeted_programs(name):
    """Every targeted trace program of one field flavour, in a fixed order."""
    q, bits = FIXED[name]
    progs = [rows_program(q, bits)] + [lanes_program(q, bits, w) for w in (1, 2, 4, 5, 12)]
    progs += [rounds_program(q, bits), short_exponents_program(q, bits), long_exponents_program(q, bits), pow_groups_program(q, bits),
              statics_program(q, bits), outputs_program(q, bits), two_outs_program(q, bits), init_program(q, bits, 4), init_program(q, bits, 1),
              init_program(q, bits, 2), shape_program(q, bits, 1, 1), shape_program(q, bits, 64, 64),
              # vm_regs 33 and 32 with 64 registers: the two sides of the interpreter's 160 KiB rule where an element takes 16 bytes of LDS
              # (p128, and q64: its 64-bit elements sit in 16-byte slots too)
              shape_program(q, bits, 33, 64), shape_program(q, bits, 32, 64),
              shape_program(q, bits, 5, 3, segment_counts=(5,))]                                       # the last: host_run
    if bits > 128:      # 32-byte elements: all three private-array variants are reachable, each next to a shape that still fits the LDS
        progs += [shape_program(q, bits, 16, 33), shape_program(q, bits, 16, 32), shape_program(q, bits, 32, 25), shape_program(q, bits, 32, 24),
                  shape_program(q, bits, 64, 9), shape_program(q, bits, 64, 8)]
    return progs


# ---- 2b. constraint programs ----------------------------------------------------------------------------------------------------
CONSTRAINT_SHAPES = [   # (nc, pstride, shift, vm_regs)
    (1, 1, 0, 16), (1, 2, 4, 17), (2, 2, 1, 17), (2, 1, 5, 32), (127, 16, 126, 32), (127, 1, 130, 33), (128, 1, 131, 33), (128, 2, 0, 64),
    (129, 2, 1, 64), (129, 16, 128, 16), (1000, 16, 1003, 16), (1000, 1, 999, 33)]


def constraint_program(q, bits, fused, nc, pstride, shift, vm_regs):
    """Eight constraints over four registers, LOADN, static tables of 1, 3, 8 and nc points.  fused: with a linear row (the flat SSA
    route of jit_constraints_source); otherwise the register route."""
    a, regs = Asm(vm_regs), 4
    ev = corner_values(q)
    x = [a.loadr(r) for r in range(regs)]
    n = [a.loadn(r) for r in range(regs)]
    s = [a.loads(i) for i in range(4)]
    k = a.const(long_exponents(q, bits)['run8'])
    for j in range(4):
        if fused:
            y = a.row([(x[(j + i) % regs], q - 1 if j == 0 else ev[(j + 3 * i) % len(ev)]) for i in range(7 + j)] + [(s[j], None)])
        else:
            y = a.mul(x[j], x[(j + 1) % regs])
            y = a.mul(y, s[j], d=y)
        t = a.sub(n[j], y, d=y)
        a.out(j, t)
        a.rel(t)
    t = a.mul(x[0], s[0]); a.out(4, t); a.rel(t)
    t = a.pow(x[1], 3); t = a.sub(t, n[1], d=t); a.out(5, t); a.rel(t)
    u, v = a.powk(x[2], k), a.powk(x[3], k)             # two adjacent exponentiations with one exponent: a group
    t = a.add(a.mul(u, v, d=u), a.mul(s[1], s[2], d=v), d=u); a.out(6, t); a.rel(u, v)
    t = a.add(s[3], n[3]); a.out(7, t)
    a.top = vm_regs
    assert len(a.free) >= 0 and max(d for op, d, _, _ in a.code if op != OUT) < vm_regs
    rng = random.Random(nc * 131 + pstride)
    prow = (nc - 1) * pstride + 1                       # just large enough
    columns = [rng.choice(ev) if rng.random() < 0.3 else rng.randrange(q) for _ in range(regs * prow)]
    for r in range(regs):
        columns[r * prow] = q - 1
    tables = [[rng.choice(ev) if rng.random() < 0.3 else rng.randrange(q) for _ in range(m)] for m in (1, 3, 8, nc)]
    return SimpleNamespace(name=f"constraints_{'flat' if fused else 'registers'}_nc{nc}_s{pstride}_vm{vm_regs}", kind='constraints', q=q, code=a.code,
                           consts=a.consts, registers=regs, vm_regs=vm_regs, constraints=8, columns=columns, prow=prow, pstride=pstride, nc=nc,
                           shift=shift, tables=tables, init=[], expect=('gs_dot9_flush(acc);',) if fused else ('= gs_mul(t',))


def constraint_programs(name):
    q, bits = FIXED[name]
    return [constraint_program(q, bits, fused, *shape) for shape in CONSTRAINT_SHAPES for fused in (True, False)]


# ---- 3. generated programs ------------------------------------------------------------------------------------------------------
def generated_program(seed, name):
    """A random program at instruction level: expression DAGs over every opcode, biased toward sums of products by constants (rows fuse)
    and repeated exponents (groups form).  Every third seed is a constraint program (LOADN), the others are trace programs."""
    q, bits = FIXED[name]
    rng = random.Random(seed * 7919 + bits)
    constraints = seed % 3 == 2
    regs = rng.randint(1, 8)
    periods = [rng.choice((1, 2, 3, 4, 8)) for _ in range(rng.randint(0, 3))]
    nconsts = rng.randint(0, 12)
    a = Asm()
    a.consts[:] = [v % q for v in rand_elements(rng, nconsts, edge=0.3)]
    exps = long_exponents(q, bits)
    nexp = min(nconsts, rng.randint(0, 2))              # the first nexp constants double as exponents: one short, one long
    for i in range(nexp):
        a.consts[i] = rng.choice((3, 0xfffffffb, 2**32 + 1)) if i else rng.choice(sorted(exps.values()))

    def block(a, budget, statics, nxt):
        pool, long_pows = [], 0

        def load():
            kinds = ['r'] * 3 + (['c'] * 2 if nconsts else []) + (['s'] if statics else []) + (['n'] if nxt else [])
            k = rng.choice(kinds)
            if k == 'r': return a.loadr(rng.randrange(regs))
            if k == 'c': return a.loadk(rng.randrange(nconsts))
            if k == 'n': return a.loadn(rng.randrange(regs))
            return a.loads(rng.randrange(len(periods)))
        pool.append(a.loadr(0))
        while len(a.code) < budget:
            if len(pool) > 24:                          # keep the scratch file small: forget values (their registers are reused)
                for t in rng.sample(pool, 8):
                    pool.remove(t)
                    a.rel(t)
            roll, room = rng.random(), budget - len(a.code)
            if roll < 0.25 or len(pool) < 2:
                pool.append(load())
            elif roll < 0.55:
                pool.append(a.ins(rng.choice((ADD, SUB, MUL, MUL)), rng.choice(pool), rng.choice(pool)))
            elif roll < 0.70 and nconsts and room >= 6: # a row: products by constants, sometimes a leaf that rides along
                terms = [(rng.choice(pool), None) if rng.random() < 0.15 and i else (rng.choice(pool), rng.randrange(nconsts)) for i in range(rng.randint(2, min(9, room // 3)))]
                pool.append(a.row(terms, pooled=True))
            elif roll < 0.85:                           # adjacent exponentiations with one exponent
                e = rng.choice((0, 1, 2, 3, 5, 7, 2**31, 2**32 - 1, rng.randrange(2**32)))
                pool += [a.pow(x, e) for x in rng.sample(pool, min(len(pool), room, rng.randint(1, 5)))]
            elif nexp and long_pows < 4:
                k = rng.randrange(nexp)
                srcs = rng.sample(pool, min(len(pool), room, rng.randint(1, 5), 4 - long_pows))
                long_pows += len(srcs)
                pool += [a.powk(x, k) for x in srcs]
        return pool
    init = None
    if not constraints and rng.random() < 0.4:
        init = Asm()
        init.consts = a.consts
        pool = block(init, rng.randint(4, 20), False, False)
        for r in rng.sample(range(regs), rng.randint(1, regs)):
            init.out(r, rng.choice(pool))
    nout = rng.randint(1, 8) if constraints else regs
    pool = block(a, rng.randint(10, 120 - nout - 1), bool(periods), constraints)
    dsts = list(range(nout)) if constraints else rng.sample(range(regs), rng.randint(1, regs))
    if rng.random() < 0.2:
        dsts.append(dsts[0])                            # a destination written twice
    for d in dsts:
        a.out(d, rng.choice(pool))
    tables = [[v % q for v in rand_elements(rng, m, edge=0.3)] if rng.random() < 0.7 else [rng.randrange(2) for _ in range(m)] for m in periods]
    if constraints:
        nc, pstride = rng.choice((1, 2, 63, 64, 200)), rng.choice((1, 2, 3))
        prow = (nc - 1) * pstride + 1 + rng.randrange(3)
        return SimpleNamespace(name=f'generated_{seed}', kind='constraints', q=q, code=a.code, consts=a.consts, registers=regs, vm_regs=a.top,
                               constraints=nout, columns=[v % q for v in rand_elements(rng, regs * prow, edge=0.3)], prow=prow, pstride=pstride, nc=nc,
                               shift=rng.randrange(nc + 4), tables=tables, init=[], expect=())
    p = trace_prog(f'generated_{seed}', q, a, regs, seglen=rng.randint(2, 6), segment_counts=(rng.randint(9, 40),), statics=tables, init=init, seed=seed)
    p.rows = lambda segments: [[v % q for v in rand_elements(random.Random(seed * 31 + s), regs, edge=0.3)] for s in range(segments)]
    return p


# ---- 4. running a program -----------------------------------------------------------------------------------------------------
def _words(code):
    return (C.c_uint32 * (4 * len(code)))(*[w for ins in code for w in ins]) if code else None


def _pack(vals, es):
    return b''.join(int(v).to_bytes(es, 'little') for v in vals) or None


def _unpack(raw, es):
    return [int.from_bytes(raw[i:i + es], 'little') for i in range(0, len(raw), es)]


def model(p, segments=None):
    if p.kind == 'trace':
        return run_trace(p.code, p.init, p.consts, p.statics, p.rows(segments), segments, p.seglen, p.q)
    return run_constraints(p.code, p.consts, p.columns, p.prow, p.pstride, p.nc, p.shift, p.tables, p.q)


def trace_on(backend, p, segments):
    """gs_air_trace_segments of a backend (the oracle, or the product library interpreted or compiled) -> registers x steps integers."""
    es, steps = backend.element_size, segments * p.seglen
    periods = (C.c_uint32 * max(len(p.statics), 1))(*[len(s) for s in p.statics])
    out = backend.alloc(p.registers * steps * es)
    try:
        backend.call('gs_air_trace_segments', _words(p.code), len(p.code), _words(p.init), len(p.init), _pack(p.consts, es), len(p.consts), p.vm_regs,
                     p.registers, _pack([v for s in p.statics for v in s], es), periods if p.statics else None, len(p.statics),
                     _pack([v for row in p.rows(segments) for v in row], es), segments, p.seglen, C.c_void_p(out))
        return _unpack(backend.download(out, p.registers * steps * es), es)
    finally:
        backend.free(out)


def constraints_on(backend, p):
    """gs_air_constraints (contiguous columns) or gs_air_constraints_strided of a backend -> constraints x nc integers."""
    es = backend.element_size
    lens = (C.c_uint64 * max(len(p.tables), 1))(*[len(t) for t in p.tables])
    cols, out = backend.alloc(len(p.columns) * es), backend.alloc(p.constraints * p.nc * es)
    tabs = backend.alloc(max(1, sum(len(t) for t in p.tables)) * es)
    try:
        backend.upload(cols, _pack(p.columns, es))
        if p.tables:
            backend.upload(tabs, _pack([v for t in p.tables for v in t], es))
        backend.upload(out, bytes(p.constraints * p.nc * es))
        head = [_words(p.code), len(p.code), _pack(p.consts, es), len(p.consts), p.vm_regs, p.registers, p.constraints, C.c_void_p(cols)]
        tail = [p.nc, p.shift, C.c_void_p(tabs) if p.tables else None, lens if p.tables else None, len(p.tables), C.c_void_p(out)]
        if p.pstride == 1 and p.prow == p.nc:
            backend.call('gs_air_constraints', *head, *tail)
        else:
            backend.call('gs_air_constraints_strided', *head, p.prow, p.pstride, *tail)
        return _unpack(backend.download(out, p.constraints * p.nc * es), es)
    finally:
        for ptr in (cols, out, tabs):
            backend.free(ptr)


def run_on(backend, p, segments=None):
    return trace_on(backend, p, segments) if p.kind == 'trace' else constraints_on(backend, p)


def generated_source(lib, p, tmp_path, monkeypatch, declined_ok=False):
    """The HIP source the generator writes for the program, after it has built for gfx950 (gs_air_jit_check_statics: no device needed;
    GSTARK_AIR_JIT_DUMP keeps the source, in a directory of its own for every call).  declined_ok: None when the generator declines the
    program (the interpreter then runs it) instead of a failure."""
    dump_dir = tmp_path / f'dump{len(list(tmp_path.iterdir()))}'
    dump_dir.mkdir()
    monkeypatch.setenv('GSTARK_AIR_JIT_DUMP', str(dump_dir))
    es = lib.gs_element_size()
    hook = lib.gs_air_jit_check_statics
    hook.restype = C.c_int
    hook.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                     C.c_char_p, C.c_void_p, C.c_uint64]
    tables = p.statics if p.kind == 'trace' else p.tables
    lens = (C.c_uint64 * max(len(tables), 1))(*[len(t) for t in tables])
    log = C.create_string_buffer(8192)
    rc = hook(0 if p.kind == 'trace' else 1, _words(p.code), len(p.code), _words(p.init), len(p.init), _pack(p.consts, es), len(p.consts), p.vm_regs,
              p.registers, lens, len(tables), _pack([v for t in tables for v in t], es) if p.kind == 'trace' else None, log, len(log))
    if declined_ok and rc != 0 and b'does not know' in log.value:
        return None
    assert rc == 0, f'{p.name} does not build:\n{log.value.decode(errors="replace")}'
    new = sorted(dump_dir.iterdir())
    assert len(new) == 1, f'{p.name}: one source file expected, got {new}'
    return new[0].read_text()


# ---- 5. reading an emitted addition chain ---------------------------------------------------------------------------------------
def chain_exponent(block):
    """The exponent a generated chain computes, by following its statements with integers (x = p1 has exponent 1): the lazy form
    (lz_sqr / lz_mul_v, windows over the odd powers p3, p5, ... or the pattern chain's g words) and the canonical one (gs_sqr / gs_mul).
    -> (the exponent of acc, the number of products, every variable's exponent)."""
    val = {'p1': 1}
    lines = block.split('\n')
    products = block.count('lz_mul_v(') + block.count('gs_mul(')          # every product in the text, matched below or not
    for ln in lines:
        ln = ln.strip()
        m = re.match(r'for \(int q = 0; q < (\d+); q\+\+\) (\w+) = (?:lz_sqr|gs_sqr)\((\w+)(?:, K)?\);', ln)
        if m:
            assert m.group(2) == m.group(3)
            val[m.group(2)] <<= int(m.group(1))
            continue
        m = re.match(r'(?:const )?(?:lz |fe )?(\w+) = (?:lz_sqr|gs_sqr)\((\w+)(?:, K)?\);', ln)
        if m:
            val[m.group(1)] = 2 * val[m.group(2)]
            continue
        m = re.match(r'(?:const )?(?:lz |fe )?(\w+) = (?:lz_mul_v|gs_mul)\((\w+), (\w+)(?:, K)?\);', ln)
        if m:
            val[m.group(1)] = val[m.group(2)] + val[m.group(3)]
            continue
        m = re.match(r'(?:const )?(?:lz |fe )?(\w+) = (\w+);$', ln)
        if m and m.group(2) in val:
            val[m.group(1)] = val[m.group(2)]
    return val['acc'], products, val


def chain_blocks(source):
    """The addition chains of a generated source, in program order: from `p1 = <base>` to the statement that takes acc."""
    return re.findall(r'const (?:lz|fe) p1 = .*?(?:lz_pack\(acc\);|= acc;)', source, flags=re.S)


def chain_test_exponents(q, bits):
    """At least sixty exponents (none 0 or 1, which emit no chain): the structured ones, powers of two, all-ones, random ones of several widths."""
    rng = random.Random(0x636861696e ^ bits)
    es = [2, 3, 5, 7] + list(long_exponents(q, bits).values()) + [2**31, 2**32 - 1, 0xdeadbeef]
    es += [2**k for k in (1, 2, 5, 16, 32, 33, 63, 64, 100, bits - 2) if k < bits - 1]
    es += [2**k - 1 for k in (2, 3, 8, 16, 33, 63, 64, 100, bits - 1) if k < bits]
    for width in (8, 33, 64, 100, bits):
        if width <= bits:
            es += [rng.randrange(2**(width - 1), min(2**width, q)) for _ in range(6)]
    es += [rng.randrange(2, q) for _ in range(12)]
    return list(dict.fromkeys(es))


def chains_program(q, exponents):
    """One POWC per exponent on the register route of the constraint generator: each chain is emitted once, in program order."""
    a = Asm()
    x = a.loadr(0)
    for i, e in enumerate(exponents):
        t = a.powk(x, a.const(e))
        a.out(i, t)
        a.rel(t)
    return SimpleNamespace(name='chains', kind='constraints', q=q, code=a.code, consts=a.consts, registers=1, vm_regs=a.top, constraints=len(exponents),
                           tables=[], init=[], expect=())
