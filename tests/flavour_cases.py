"""Kernel-level checks for the library builds of the other fields (csrc/build.sh: q64, q32, q17, p256, p224 and the runtime-modulus
build).  A large part of what those builds run is code the 128-bit build never compiles (the canonical k_ntt_pass<LB>, the plain
fe_inv at the end of k_batch_inv, the canonical branch and the `fe k, kp` descriptors of k_composition_tail, the byte-wise Horner
prng_point, the canonical mimc_dot) or code whose shape follows the element size (leaf hashing over 32-byte elements, the column
buffer of k_fri_layers).  Every check here takes a backend, reads q = backend.modulus and es = backend.element_size, and compares
with plain Python integers, hashlib and oracle/pyref.py at the smallest shapes that take each path of that code.  Each returns a
digest of every output byte, so the same call on two backends (the HIP build and the oracle flavour) can be compared byte for byte.

The shape lists below are derived from the plan arithmetic of csrc/ntt.hip (plan_get / ntt_run) — see ntt_plan()."""
import ctypes as C
import hashlib

import abi_cases as cases
from genstark_amd._abi import HASH_ALGS, FriLayer
from genstark_amd.field import PrimeField
from oracle import pyref

FULL_NTT_LOGN = 13          # up to here every output value is compared with pyref's recursive radix-2 transform
RANDOM_NTT_LOGN = 17        # above: the input is a power series made on the device (no Python loop over 2^20 values)
MAX_PASS_TWIDDLES = 1 << 20  # kMaxPassTwiddleEntries (csrc/ntt.hip): a later pass with more inter-pass twiddles keeps a running product


# ---- field elements -----------------------------------------------------------------------------------------------------------
def two_adicity(q):
    return ((q - 1) & -(q - 1)).bit_length() - 1


def field_edges(q):
    """0, 1, 2, q-1, q-2, (q+1)/2, 2^k and 2^k - 1 at the 32-bit limb seams below q, and C = 2^B - q (B = the bits of q: what a
    reduction folds back in)."""
    bits = q.bit_length()
    out = {0, 1, 2, q - 1, q - 2, (q + 1) // 2, (1 << bits) - q}
    for k in range(32, bits, 32):
        if (1 << k) < q:
            out |= {1 << k, (1 << k) - 1}
    return sorted(out)


def rand_elements(rng, n, q, edge=0.1):
    edges = field_edges(q)
    return [rng.choice(edges) if rng.random() < edge else rng.randrange(q) for _ in range(n)]


def _digest(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p)
    return h.hexdigest()


def _values(raw, es):
    return [int.from_bytes(raw[i:i + es], 'little') for i in range(0, len(raw), es)]


# ---- (a) NTT ------------------------------------------------------------------------------------------------------------------
def ntt_plan(logn):
    """The radix bits of each pass, as plan_get derives them: np = (logn + 7) / 8 passes of base (+1) bits.  Pass i runs
    k_ntt_pass<L[i] - 4>; the first pass transposes its output through LDS, a later one reads its inter-pass twiddles from a table
    when the table has at most 2^20 entries and from a running product otherwise.  Below 2^8 points (or at most 8 coefficients)
    the Horner kernel serves the call."""
    if logn < 8:
        return []
    np_ = (logn + 7) // 8
    base, extra = divmod(logn, np_)
    return [base + (1 if i < extra else 0) for i in range(np_)]


def ntt_roles(logn):
    """[(LB, role)] of the passes of a 2^logn-point transform; role: 'first', 'table' or 'running'."""
    out, acc = [], 0
    for i, bits in enumerate(ntt_plan(logn)):
        role = 'first' if i == 0 else ('table' if (1 << (acc + bits)) <= MAX_PASS_TWIDDLES else 'running')
        out.append((bits - 4, role))
        acc += bits
    return out


def _plens(logn):
    n = 1 << logn
    return [n // 16, n // 16 + 1, n // 2 + 3, n]


# (logn, plen, rows) served by k_eval_horner: every size below 2^8 at a short, a ragged and the full length; 2^10 points of 8 coefficients
NTT_HORNER = sorted({(logn, plen, 2 if logn == 5 else 1) for logn in range(8) for plen in (1, (1 << logn) // 2 + 1, 1 << logn)
                     if plen <= 1 << logn}) + [(10, 8, 2)]
# one radix-256 pass in a 16-thread workgroup; 16 coefficients take the skipped-butterfly branch (in_len <= n / 16), 17 do not
NTT_ONE_PASS = [(8, plen, 1) for plen in (9, 16, 17, 256)]
# [5,4] [5,5] [6,5] [6,6] [7,6] [7,7] [8,7] [8,8]: LB 1..4 as the first pass, LB 0..4 as the table pass; three distinct rows in one
# launch at 2^9, 2^12, 2^13 and 2^16
NTT_TWO_PASS = {logn: [(logn, plen, 3 if logn in (9, 12, 13, 16) else 1) for plen in _plens(logn)] for logn in range(9, 17)}
# [6,6,5] and [7,7,6]: tables in every later pass, the third table of 2^20 exactly at the limit; [7,7,7]: the third pass is over it
NTT_THREE_PASS = {logn: [(logn, plen, 1) for plen in ((1 << logn) // 16, 1 << logn)] for logn in (17, 20, 21)}


def check_ntt(backend, rng, logn, plen, rows=1, reference=True):
    """gs_eval_polys_at_roots over `rows` distinct random polynomials of `plen` coefficients in ONE call, then gs_interpolate_roots
    of the result: the round trip returns the zero-padded input bytes; the evaluations equal pyref's recursive transform (every value,
    up to 2^13 points) or direct evaluation on Python integers at eight sampled indices (above)."""
    be = backend
    f = PrimeField(backend=be)
    q, es, n = f.modulus, f.elementSize, 1 << logn
    w = f.getRootOfUnity(n)
    polys = [rand_elements(rng, plen, q) for _ in range(rows)]
    m, ev, back = f.newMatrixFrom(polys), f.newMatrix(rows, n), f.newMatrix(rows, n)
    be.call('gs_eval_polys_at_roots', C.c_void_p(m.ptr), rows, plen, f.le(w), n, C.c_void_p(ev.ptr))
    be.call('gs_interpolate_roots', C.c_void_p(ev.ptr), rows, f.le(w), n, C.c_void_p(back.ptr))
    ev_raw, back_raw = ev.toBuffer(), back.toBuffer()
    assert back_raw == b''.join(b''.join(f.le(c) for c in p) + bytes(es * (n - plen)) for p in polys), ('round trip', logn, plen, rows)
    if reference:
        ref = pyref.Field(q)
        for r in range(rows):
            got = _values(ev_raw[r * n * es:(r + 1) * n * es], es)
            if logn <= FULL_NTT_LOGN:
                want = ref.ntt(polys[r], w, n)
                if got != want:
                    bad = [i for i in range(n) if got[i] != want[i]]
                    raise AssertionError(f'eval: logn {logn} plen {plen} row {r}: {len(bad)} of {n} values differ, first at {bad[:8]}')
            else:
                for i in sorted({0, 1, n - 1, n // 2} | {rng.randrange(n) for _ in range(4)}):
                    assert got[i] == ref.eval_poly_at(polys[r], pow(w, i, q)), ('eval', logn, plen, r, i)
    return _digest(ev_raw, back_raw)


def check_ntt_series(backend, rng, logn, plens, reference=True):
    """The same at sizes where a Python loop over the input is too slow: the coefficients are a power series c^i made on the device.
    Round trip on every byte, linearity eval(a) + eval(b) == eval(a + b) at the full length, and the closed form of a (zero-extended)
    geometric series p(x) = ((c x)^plen - 1) / (c x - 1) at eight sampled indices."""
    be = backend
    f = PrimeField(backend=be)
    q, es, n = f.modulus, f.elementSize, 1 << logn
    w = f.getRootOfUnity(n)
    c, c2 = rng.randrange(2, q), rng.randrange(2, q)
    a = f.getPowerSeries(c, n)
    a_raw = a.toBuffer()
    parts, full = [], None
    for plen in plens:
        ev, back = f.newVector(n), f.newVector(n)
        be.call('gs_eval_polys_at_roots', C.c_void_p(a.ptr), 1, plen, f.le(w), n, C.c_void_p(ev.ptr))
        be.call('gs_interpolate_roots', C.c_void_p(ev.ptr), 1, f.le(w), n, C.c_void_p(back.ptr))
        back_raw = back.toBuffer()
        assert back_raw[:plen * es] == a_raw[:plen * es] and back_raw[plen * es:] == bytes((n - plen) * es), ('round trip', logn, plen)
        if reference:
            for i in sorted({0, 1, n - 1, n // 2} | {rng.randrange(n) for _ in range(4)}):
                cx = c * pow(w, i, q) % q
                want = (pow(cx, plen, q) - 1) * pow(cx - 1, -1, q) % q if cx != 1 else plen % q
                assert ev.getValue(i) == want, ('eval', logn, plen, i)
        parts.append(ev.toBuffer())
        if plen == n:
            full = ev
    if reference and full is not None:
        b, eb, es_ = f.getPowerSeries(c2, n), f.newVector(n), f.newVector(n)
        be.call('gs_eval_polys_at_roots', C.c_void_p(b.ptr), 1, n, f.le(w), n, C.c_void_p(eb.ptr))
        s = f.addVectorElements(a, b)
        be.call('gs_eval_polys_at_roots', C.c_void_p(s.ptr), 1, n, f.le(w), n, C.c_void_p(es_.ptr))
        assert f.addVectorElements(full, eb).toBuffer() == es_.toBuffer(), ('linearity', logn)
    return _digest(*parts)


def check_ntt_shape(backend, rng, logn, plen, rows, reference=True):
    if logn <= RANDOM_NTT_LOGN:
        return check_ntt(backend, rng, logn, plen, rows, reference)
    return check_ntt_series(backend, rng, logn, [plen], reference)


# ---- (b) batch inversion and division -----------------------------------------------------------------------------------------------
# k_batch_inv: one element per thread up to 16 383, 16 384 threads from there on (several elements per thread), 32 elements per
# thread with a ragged tail at 2^19 + 13
INVERSE_SIZES = [5, 257, 16383, 16384, 40000, (1 << 19) + 13]
FULL_INVERSE_N = 40000


def check_batch_inverse(backend, rng, n, reference=True):
    """gs_vec_inv / gs_vec_div with every third element zero (0^-1 = 0), and an all-zero vector, against pow(x, -1, q): every
    element up to 40 000, 2 000 sampled indices above."""
    f = PrimeField(backend=backend)
    q, es = f.modulus, f.elementSize
    if n <= FULL_INVERSE_N:
        xs, ys = rand_elements(rng, n, q), rand_elements(rng, n, q)
    else:
        xs, ys = [rng.randrange(1, q) for _ in range(n)], [rng.randrange(q) for _ in range(n)]
    for i in range(0, n, 3):
        xs[i] = 0
    vx, vy = f.newVectorFrom(xs), f.newVectorFrom(ys)
    inv_raw, div_raw = f.invVectorElements(vx).toBuffer(), f.divVectorElements(vy, vx).toBuffer()
    zeros = f.newVector(n)
    backend.upload(zeros.ptr, bytes(n * es))
    assert f.invVectorElements(zeros).toBuffer() == bytes(n * es), ('all-zero vector', n)
    assert f.divVectorElements(vy, zeros).toBuffer() == bytes(n * es), ('division by an all-zero vector', n)
    if reference:
        idx = range(n) if n <= FULL_INVERSE_N else sorted({0, 1, n - 1, n - 2} | set(rng.sample(range(n), 2000)))
        for i in idx:
            want = pow(xs[i], -1, q) if xs[i] else 0
            assert int.from_bytes(inv_raw[i * es:(i + 1) * es], 'little') == want, ('inv', n, i)
            assert int.from_bytes(div_raw[i * es:(i + 1) * es], 'little') == ys[i] * want % q, ('div', n, i)
    return _digest(inv_raw, div_raw)


# ---- (c) leaf hashing and Merkle trees at this element size -----------------------------------------------------------------------------
MERGE_ROWS_COUNTS = (1, 2, 3, 5, 8)
MERGE_ROWS_SIZES = (1, 255, 4097)
# one subtree workgroup; subtrees + the last-arrival top; the widest one-launch tree; the streaming launches
MERKLE_LOGN = (1, 8, 9, 15, 16)
MERKLE_COUNTS = (1, 3)


def check_hash_merge_rows(backend, rng, alg, n):
    """gs_hash_merge_rows over 1, 2, 3, 5 and 8 columns of field elements (edge values among them): every digest against hashlib over
    the row's little-endian elements, each of element_size bytes."""
    be = backend
    f = PrimeField(backend=be)
    q, H, out = f.modulus, cases._h(alg), []
    for count in MERGE_ROWS_COUNTS:
        cols = [rand_elements(rng, n, q, edge=0.2) for _ in range(count)]
        vecs = [f.newVectorFrom(c) for c in cols]
        leaves = be.alloc(32 * n)
        be.call('gs_hash_merge_rows', HASH_ALGS[alg], (C.c_void_p * count)(*[v.ptr for v in vecs]), count, n, C.c_void_p(leaves))
        raw = be.download(leaves, 32 * n)
        be.free(leaves)
        for i in range(n):
            assert raw[32 * i:32 * i + 32] == H(b''.join(f.le(c[i]) for c in cols)), (alg, count, n, i)
        out.append(raw)
    return _digest(*out)


def check_merkle(backend, rng, alg, logn):
    """The fused commit entry, and gs_hash_merge_rows + gs_merkle_build, over 1 and 3 columns: every leaf digest against hashlib,
    every node against pyref's tree (abi_cases.check_merkle_commit, which takes the element size from the backend)."""
    for count in MERKLE_COUNTS:
        cases.check_merkle_commit(backend, rng, alg, logn, count)


# ---- (d) the fused entries against their definitions ----------------------------------------------------------------------------------------
FRI_FOLD_SHAPES = [(8, 0), (12, 1)]
FRI_LAYERS_SHAPES = [(9, 0, 1, 'blake2s256'), (13, 1, 3, 'sha256'), (17, 1, 5, 'blake2s256')]       # the last: multi-workgroup + last-arrival top
TAIL_SHAPES = [(8, 4, [1], 0, False), (12, 8, [2, 1], 3, True), (13, 9, [1, 1], 70, False)]          # 70 vectors: twelve groups of six
MIMC_SHAPES = [(5, 2, 1), (8, 4, 2), (12, 8, 4)]


def check_fri_layers_definition(backend, rng, logm, depth, nlayers, alg):
    """gs_fri_layers against its definition, layer by layer, on Python integers and hashlib: the folded column (the cubic through each
    row's four points, evaluated at the layer's point: every row up to 2 048, sampled rows above), every leaf digest (a row of the
    transposed next column), every node (pyref's tree), the posted root, and every derived point = sha256(root) as a big-endian integer
    mod q — the point each following layer is folded at, asked for at every layer."""
    be = backend
    f = PrimeField(backend=be)
    q, es, H = f.modulus, f.elementSize, cases._h(alg)
    m, step = 1 << logm, 4 ** depth
    n = m * step
    w = f.getRootOfUnity(n)
    vals = rand_elements(rng, m, q)
    column, x = f.newVectorFrom(vals), rng.randrange(q)
    xv = f.newVectorFrom([x])
    layers, keep = (FriLayer * nlayers)(), []
    for i in range(nlayers):
        rows = m >> (2 * i + 2)
        nxt, leaves, nodes, point = f.newVector(rows), be.alloc(32 * (rows // 4)), be.alloc(32 * (rows // 4)), f.newVector(1)
        keep.append((nxt, leaves, nodes, point))
        layers[i].next, layers[i].leaves, layers[i].nodes, layers[i].point_out = nxt.ptr, leaves, nodes, point.ptr
    be.call('gs_fri_layers', HASH_ALGS[alg], f.le(w), n, step, C.c_void_p(column.ptr), m, C.c_void_p(xv.ptr), nlayers, C.cast(layers, C.c_void_p))
    cur_m, cur_step = m, step
    for i, (nxt, leaves, nodes, point) in enumerate(keep):
        rows = cur_m // 4
        nxt_raw = nxt.toBuffer()
        got = _values(nxt_raw, es)
        picks = range(rows) if rows <= 2048 else sorted({0, 1, rows - 1, rows // 2} | set(rng.sample(range(rows), 60)))
        for r in picks:
            pts = [(pow(w, (r + c * rows) * cur_step, q), vals[r + c * rows]) for c in range(4)]
            acc = 0
            for j, (xj, yj) in enumerate(pts):
                num = den = 1
                for k, (xk, _) in enumerate(pts):
                    if k != j:
                        num, den = num * (x - xk) % q, den * (xj - xk) % q
                acc = (acc + yj * num * pow(den, -1, q)) % q
            assert got[r] == acc, ('fold', i, r)
        qn = rows // 4
        want_leaves = [H(b''.join(nxt_raw[(j + k * qn) * es:(j + k * qn + 1) * es] for k in range(4))) for j in range(qn)]
        got_leaves, got_nodes = be.download(leaves, 32 * qn), be.download(nodes, 32 * qn)
        assert [got_leaves[32 * j:32 * j + 32] for j in range(qn)] == want_leaves, ('leaves', i)
        tree = pyref.MerkleTree(want_leaves, H)
        assert [got_nodes[32 * j:32 * j + 32] for j in range(1, qn)] == tree.nodes[1:], ('nodes', i)
        root = C.create_string_buffer(32)
        be.call('gs_readback_wait', layers[i].ticket, root)
        assert root.raw == tree.root, ('posted root', i)
        x = int.from_bytes(hashlib.sha256(tree.root).digest(), 'big') % q
        assert point.toValues() == [x], ('point', i)
        vals, cur_m, cur_step = got, rows, cur_step * 4
        be.free(leaves); be.free(nodes)


# ---- every group on one backend (the runtime-modulus worker: one modulus per process) -------------------------------------------------------
def run_groups(backend, seed, ntt_max_logn=16, inverse_max_n=40000, merkle_max_logn=9, fri_layers_max_logm=17, reference=True):
    """Groups (a) to (d) within the given limits (and the field's two-adicity); {case: digest of its output bytes}."""
    import random
    adic = two_adicity(backend.modulus)
    out = {}
    rng = lambda *key: random.Random(repr((seed,) + key))
    for logn, plen, rows in NTT_HORNER + NTT_ONE_PASS + [s for v in NTT_TWO_PASS.values() for s in v] + [s for v in NTT_THREE_PASS.values() for s in v]:
        if logn <= min(ntt_max_logn, adic):
            out[f'ntt-{logn}-{plen}-{rows}'] = check_ntt_shape(backend, rng('ntt', logn, plen), logn, plen, rows, reference)
    for n in INVERSE_SIZES:
        if n <= inverse_max_n:
            out[f'inverse-{n}'] = check_batch_inverse(backend, rng('inv', n), n, reference)
    for alg in ('sha256', 'blake2s256'):
        for n in MERGE_ROWS_SIZES:
            out[f'merge-rows-{alg}-{n}'] = check_hash_merge_rows(backend, rng('rows', alg, n), alg, n)
        for logn in MERKLE_LOGN:
            if logn <= merkle_max_logn:
                check_merkle(backend, rng('merkle', alg, logn), alg, logn)
    for logn, depth in FRI_FOLD_SHAPES:
        if logn <= adic:
            out[f'fri-fold-{logn}-{depth}'] = _digest(cases.check_fri_fold(backend, rng('fold', logn), logn, depth))
    for logm, depth, nlayers, alg in FRI_LAYERS_SHAPES:
        if logm + 2 * depth <= adic and logm <= fri_layers_max_logm:
            out[f'fri-layers-{logm}'] = cases.check_fri_layers(backend, rng('layers', logm), logm, depth, nlayers, alg)
            if reference:
                check_fri_layers_definition(backend, rng('layers-def', logm), logm, depth, nlayers, alg)
    for logn, logsteps, per_row, lcount, adjusted in TAIL_SHAPES:
        if logn <= adic:
            for with_c in (True, False):
                got = cases.check_composition_tail(backend, rng('tail', logn, with_c), logn, logsteps, per_row, lcount, adjusted, with_c=with_c)
                out[f'tail-{logn}-{int(with_c)}'] = _digest(repr(got).encode())
    for logn, logsteps, nroots in MIMC_SHAPES:
        if logn <= adic:
            out[f'mimc-{logn}'] = _digest(cases.check_mimc_composition(backend, rng('mimc', logn), logn, logsteps, nroots))
    return out
