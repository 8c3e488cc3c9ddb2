// verifier.h — Stark.verify() (lib/Stark.ts:167-248) and LowDegreeProver.verify (lib/components/LowDegreeProver.ts:70-172) as
// native host code (included once, by prover.cc: it shares the driver's statement plan, prng and index generator).
//
// CPU-side by design, like the reference's verifier: a proof is a few hundred field elements and a few thousand digests, there is
// nothing for a GPU to do.  Input: the statement as a gs_prover_job (the fields a verifier needs: sizes, query counts, hash,
// root of unity, assertions, and of the AIR its kind, register counts, constraint degrees and — kind 0 — the round constants or —
// kind 1 — the constraint evaluator program with its constants and the PUBLIC static registers' values) + the serialized proof.
// Every check of the reference is made, in its order, with its messages; what the reference computes on BigInt / wasm runs here on
// the build flavour's host arithmetic (host_field.h) through the shared polynomial helpers (host_poly.h: transform, batch inversion,
// product of linear factors, Horner).  Hashing: host_hash.h (SHA-256, with SHA-NI when present, and a portable BLAKE2s).
#pragma once

namespace {

// ---- the wire format, read side (lib/Serializer.ts:83-144, lib/utils/serialization.ts:44-127): bounds-checked
struct Reader {
    const uint8_t *p;
    uint64_t len, at = 0;
    void need(uint64_t n) const { if (at + n > len || at + n < at) fail(GS_ERR_ARG, "malformed proof: truncated"); }
    uint8_t byte() { need(1); return p[at++]; }
    const uint8_t *take(uint64_t n) { need(n); const uint8_t *q = p + at; at += n; return q; }
};
struct ParsedMerkleProof {
    std::vector<Bytes> values;                 // the leaves' contents (rows)
    std::vector<std::vector<Bytes>> nodes;     // authentication columns
    uint32_t depth = 0;
};
ParsedMerkleProof read_merkle_proof(Reader &r, uint64_t leaf_size) {
    ParsedMerkleProof mp;
    uint32_t n = r.byte();
    if (!n) n = (uint32_t)MAX_ARRAY;
    for (uint32_t i = 0; i < n; i++) { const uint8_t *v = r.take(leaf_size); mp.values.emplace_back(v, v + leaf_size); }
    uint32_t cols = r.byte();
    if (!cols) cols = (uint32_t)MAX_ARRAY;
    std::vector<uint8_t> heads(cols);
    for (uint32_t i = 0; i < cols; i++) heads[i] = r.byte();
    for (uint8_t head : heads) {
        std::vector<Bytes> col;
        for (uint32_t j = 0; j < (uint32_t)(head >> 1); j++) {
            const uint64_t size = (j == 0 && (head & 1)) ? leaf_size : DIGEST;          // serialization.ts:93-101: a "leaf" column starts with a leaf-sized item
            const uint8_t *v = r.take(size);
            col.emplace_back(v, v + size);
        }
        mp.nodes.push_back(std::move(col));
    }
    mp.depth = r.byte();
    return mp;
}

// MerkleTree.verifyBatch (merkle package; restated with proveBatch's layout, genstark_amd/merkle.py:151-199): the leaves' DIGESTS at
// `indexes` (request order) + the columns of `proof` must hash up to `root`.  The nodes of a level are visited in ascending order, and so
// are their parents: two parallel arrays per level, no look-up structure.
struct Dg { uint8_t b[32]; };
bool merkle_verify_batch(int alg, const uint8_t *root, const std::vector<uint64_t> &indexes, const std::vector<Dg> &leaf_digests,
                         const std::vector<std::vector<Bytes>> &columns, uint32_t depth) {
    if (depth == 0 || depth > 62 || leaf_digests.size() != indexes.size()) return false;
    const uint64_t offset = 1ull << depth;
    std::vector<std::pair<uint64_t, size_t>> srt;         // (index, position in the request)
    for (size_t i = 0; i < indexes.size(); i++) {
        if (indexes[i] >= offset) return false;
        srt.push_back({indexes[i], i});
    }
    std::sort(srt.begin(), srt.end());
    for (size_t i = 1; i < srt.size(); i++) if (srt[i].first == srt[i - 1].first) return false;      // repeating indexes
    auto merge = [&](const uint8_t *a, const uint8_t *b) {
        uint8_t buf[64];
        memcpy(buf, a, 32); memcpy(buf + 32, b, 32);
        Dg d;
        host_digest(alg, buf, 64, d.b);
        return d;
    };
    auto column_item = [&](size_t col, size_t k) -> const uint8_t * {
        if (col >= columns.size() || k >= columns[col].size()) return nullptr;
        if (columns[col][k].size() != DIGEST) fail(GS_ERR_ARG, "malformed proof: a Merkle node is not a digest");
        return columns[col][k].data();
    };
    std::vector<uint64_t> ix;
    std::vector<Dg> dg;
    std::vector<size_t> ptr;
    size_t col = 0;
    for (size_t i = 0; i < srt.size(); col++) {           // the leaf pairs: one column each
        const uint64_t e = srt[i].first & ~1ull;
        const uint8_t *v1 = nullptr, *v2 = nullptr;
        size_t used = 0;
        if (srt[i].first == e) { v1 = leaf_digests[srt[i].second].b; i++; }
        if (i < srt.size() && srt[i].first == e + 1) { v2 = leaf_digests[srt[i].second].b; i++; }
        if (!v1) { v1 = column_item(col, 0); used = 1; }
        else if (!v2) { v2 = column_item(col, 0); used = 1; }
        if (!v1 || !v2) return false;
        ix.push_back((offset + e) >> 1);
        dg.push_back(merge(v1, v2));
        ptr.push_back(used);
    }
    if (col != columns.size()) return false;
    for (uint32_t lvl = depth - 1; lvl > 0; lvl--) {
        std::vector<uint64_t> nix;
        std::vector<Dg> ndg;
        for (size_t i = 0; i < ix.size(); i++) {
            const uint64_t node = ix[i];
            const uint8_t *self = dg[i].b, *sib;
            if (i + 1 < ix.size() && ix[i + 1] == (node ^ 1)) { sib = dg[i + 1].b; i++; ndg.push_back(merge(self, sib)); }
            else {
                // (the path entries of the i-th node of the CURRENT level sit in column i: proveBatch's layout)
                const size_t c = i;
                sib = column_item(c, ptr[c]);
                if (!sib) return false;
                ptr[c]++;
                ndg.push_back((node & 1) ? merge(sib, self) : merge(self, sib));
            }
            nix.push_back(node >> 1);
        }
        ix.swap(nix);
        dg.swap(ndg);
    }
    return ix.size() == 1 && ix[0] == 1 && !memcmp(dg[0].b, root, DIGEST);
}
// rehashMerkleProofValues (lib/utils/index.ts:34-45) + verifyBatch
bool merkle_check(int alg, const Bytes &root, const std::vector<uint64_t> &indexes, const ParsedMerkleProof &mp) {
    std::vector<Dg> digests(mp.values.size());
    for (size_t i = 0; i < mp.values.size(); i++) host_digest(alg, mp.values[i].data(), mp.values[i].size(), digests[i].b);
    return merkle_verify_batch(alg, root.data(), indexes, digests, mp.nodes, mp.depth);
}

// the constraint evaluator of an AIR given as a register-machine program (kind 1), on host scalars (what the device runs in
// k_air_constraints).  verify_impl validates it ONCE per job (air_program.h): every index used here lies inside cur / nxt (registers),
// statics (nstatic), the constants, the scratch file and the outputs (nconstraints).
std::vector<F> run_program(const AirProgram &p, const std::vector<F> &cur, const std::vector<F> &nxt, const std::vector<F> &statics) {
    std::vector<F> vm(p.vm_regs, (F)0), out(p.nout, (F)0);
    for (uint32_t k = 0; k < p.ninstr; k++) {
        const AirIns i = p.at(k);
        switch (i.op) {
            case OP_LOADC: vm[i.dst] = load_elem(p.consts + ELEM * i.a); break;
            case OP_LOADR: vm[i.dst] = cur[i.a]; break;
            case OP_LOADN: vm[i.dst] = nxt[i.a]; break;
            case OP_LOADS: vm[i.dst] = statics[i.a]; break;
            case OP_ADDV: vm[i.dst] = hf_add(vm[i.a], vm[i.b]); break;
            case OP_SUBV: vm[i.dst] = hf_sub(vm[i.a], vm[i.b]); break;
            case OP_MULV: vm[i.dst] = hf_mul(vm[i.a], vm[i.b]); break;
            case OP_POW: vm[i.dst] = hf_pow(vm[i.a], (hfe)(uint64_t)i.b); break;
            case OP_POWC: vm[i.dst] = hf_pow(vm[i.a], load_elem(p.consts + ELEM * i.b)); break;
            default: out[i.dst] = vm[i.a]; break;      // OP_OUT (the validator admits no other opcode)
        }
    }
    return out;
}

// coefficients of the polynomial through `values` on the m-th roots of unity {g^i} (m a power of two): an inverse DFT of size m on host
// scalars — the O(m^2) sum for the short periods of cyclic registers, the radix-2 transform with g^-1 and a scale by 1/m for the
// columns of input registers (a public input register of an air-assembly component can be as long as the trace)
std::vector<F> cyclic_poly(const std::vector<F> &values, F g) {
    const size_t m = values.size();
    const F ginv = hf_inv(g), minv = hf_inv((F)(uint64_t)m);
    if (m <= 32) {
        std::vector<F> out(m), pw(m);
        F cur = 1;
        for (size_t i = 0; i < m; i++) { pw[i] = cur; cur = hf_mul(cur, ginv); }
        for (size_t j = 0; j < m; j++) {
            F s = 0;
            for (size_t i = 0; i < m; i++) s = hf_add(s, hf_mul(values[i], pw[(i * j) % m]));
            out[j] = hf_mul(s, minv);
        }
        return out;
    }
    std::vector<F> out(values);
    host_transform(out, ginv);
    for (size_t j = 0; j < m; j++) out[j] = hp_mul(out[j], minv);
    return out;
}
// the shortest power-of-two period of a column (a cyclic register of that length denotes the same polynomial): airassembly.py _shrink
void shrink_column(std::vector<F> &col) {
    while (col.size() > 1 && col.size() % 2 == 0) {
        const size_t half = col.size() / 2;
        bool same = true;
        for (size_t i = 0; i < half && same; i++) same = col[i] == col[half + i];
        if (!same) break;
        col.resize(half);
    }
}
// a column rotated right by `shift` steps: airassembly.py _rotate (new[i] = old[(i - shift) mod len])
void rotate_column(std::vector<F> &col, int32_t shift) {
    if (col.empty()) return;
    const int64_t len = (int64_t)col.size();
    const int64_t k = (((-(int64_t)shift) % len) + len) % len;
    std::rotate(col.begin(), col.begin() + k, col.end());
}

// ---- boundary constraints at the queried points (BoundaryConstraints.ts:55-69): I_r(x) and Z_r(x) of one asserted register
// The reference's form — interpolate the m assertions, multiply the m factors out, evaluate both (lagrange + Plan::zero_poly + Horner) —
// costs ~3 m^2 products and gs_small_interpolate stops at 4096 points.  For a register with many assertions the same VALUES come from
//   Z_r          a product tree over the factors (schoolbook below, the host transform above BOUNDARY_SCHOOLBOOK_MAX coefficients),
//   c_i          = y_i / Z_r'(x_i): Z_r' over the whole execution domain is ONE T-point transform (the x_i are points of it),
//   I_r(x)       = Z_r(x) sum_i c_i / (x - x_i)  at each queried x (none of them lies in the execution domain): O(m) per point.
// m comes from the statement's assertions.  T is the statement's too, except for an AIR with input registers verified with job.steps = 0:
// there the proof's shapes lay the trace out (capped at 2^26 steps above), and this form then allocates two T-long vectors like the
// input-register columns do.
// Products with an operand of at most this many coefficients are schoolbook products.  Chosen by count, not measured on its own: 64 x 64
// is 4 096 products, the three 128-point transforms it would replace ~1 350 butterflies plus their set-up, and below it the
// transforms' bit reversal and twiddle tables outweigh the difference.
const size_t BOUNDARY_SCHOOLBOOK_MAX = 64;
// Registers with at most this many assertions keep the reference's form.  Measured with tools/boundary_host_bench.py (one core, 128-bit
// flavour, T = 2^13, 128 queried points; direct / tree in ms): m = 64: 1.1 / 4.4, 128: 3.1 / 5.6, 256: 8.8 / 8.7, 1 024: 112 / 30,
// 4 096: 1 387 / 102.  The tree form's floor is its T-point transform; the two cross at m = 256.
const size_t BOUNDARY_DIRECT_MAX = 256;
std::vector<F> poly_product(const std::vector<F> &a, const std::vector<F> &b, F omega, uint64_t N) {
    const size_t len = a.size() + b.size() - 1;
    if (std::min(a.size(), b.size()) <= BOUNDARY_SCHOOLBOOK_MAX) {
        std::vector<F> out(len, (F)0);
        for (size_t i = 0; i < a.size(); i++)
            for (size_t j = 0; j < b.size(); j++) out[i + j] = hf_add_weak(out[i + j], hf_mul_weak(a[i], b[j]));
        for (F &v : out) v = hf_canon(v);
        return out;
    }
    uint64_t n = 1;
    while (n < len) n <<= 1;
    if (n > N) fail(GS_ERR_ARG, "boundary constraints: a product of %zu coefficients needs a root of unity of order %llu", len, (unsigned long long)n);
    const F w = hf_pow(omega, (hfe)(N / n));
    std::vector<F> fa(a), fb(b);
    fa.resize(n, (F)0); fb.resize(n, (F)0);
    host_transform(fa, w);
    host_transform(fb, w);
    for (uint64_t i = 0; i < n; i++) fa[i] = hp_mul(fa[i], fb[i]);
    host_transform(fa, hf_pow(w, (hfe)(n - 1)));
    const F ninv = hf_inv((F)n);
    fa.resize(len);
    for (F &v : fa) v = hp_mul(v, ninv);
    return fa;
}
std::vector<F> zero_poly_tree(const F *xs, size_t m, F omega, uint64_t N) {
    if (m <= BOUNDARY_SCHOOLBOOK_MAX) {
        std::vector<F> zp(m + 1);
        host_linear_product(xs, m, zp.data());
        return zp;
    }
    const size_t h = m / 2;
    return poly_product(zero_poly_tree(xs, h, omega, N), zero_poly_tree(xs + h, m - h, omega, N), omega, N);
}
struct BoundaryValues { std::vector<F> i_at, z_at; };
BoundaryValues boundary_values_direct(const Plan &plan, const Plan::Reg &r, const std::vector<F> &points) {
    const std::vector<F> ipoly = lagrange(r.xs, r.ys), zpoly = plan.zero_poly(r);
    BoundaryValues out;
    for (F x : points) { out.i_at.push_back(horner(ipoly, x)); out.z_at.push_back(horner(zpoly, x)); }
    return out;
}
// what the tree form refuses of a register's assertions, with its messages
void check_many_assertions(const Plan &plan, const Plan::Reg &r) {
    const size_t m = r.steps.size();
    const uint64_t T = plan.T;
    if (m > T) fail(GS_ERR_ARG, "Invalid assertion: register %u has %zu assertions, the execution trace %llu steps", r.reg, m, (unsigned long long)T);
    std::vector<bool> seen(T, false);
    for (uint64_t s : r.steps) {
        if (s >= T) fail(GS_ERR_ARG, "Invalid assertion: step %llu is outside of execution trace", (unsigned long long)s);
        if (seen[s]) fail(GS_ERR_ARG, "Invalid assertion: step %llu of register %u is asserted more than once", (unsigned long long)s, r.reg);
        seen[s] = true;
    }
}
BoundaryValues boundary_values_tree(const Plan &plan, const Plan::Reg &r, const std::vector<F> &points) {
    const size_t m = r.steps.size();
    const uint64_t T = plan.T;
    check_many_assertions(plan, r);
    const std::vector<F> z = zero_poly_tree(r.xs.data(), m, plan.omega, plan.N);
    std::vector<F> d(T, (F)0);                                       // Z_r' ...
    for (size_t k = 0; k < m; k++) d[k] = hp_mul((F)(uint64_t)(k + 1), z[k + 1]);
    host_transform(d, hf_pow(plan.omega, (hfe)plan.E));             // ... at every point of the execution domain
    std::vector<F> c(m);
    for (size_t i = 0; i < m; i++) c[i] = d[r.steps[i]];
    host_batch_invert(c);
    for (size_t i = 0; i < m; i++) c[i] = hp_mul(c[i], r.ys[i]);
    BoundaryValues out;
    out.z_at = horner_many(z, points);
    std::vector<F> diff(m);
    for (size_t q = 0; q < points.size(); q++) {
        for (size_t i = 0; i < m; i++) diff[i] = hf_sub(points[q], r.xs[i]);
        host_batch_invert(diff);
        F sum = 0;
        for (size_t i = 0; i < m; i++) sum = hf_add_weak(sum, hf_mul_weak(c[i], diff[i]));
        out.i_at.push_back(hp_mul(out.z_at[q], hf_canon(sum)));
    }
    return out;
}


// ---- the device's share of a device-assisted verification (gs_prover_verify_device).  Two providers of "values at the queried points"
// are all that differs from verify_impl's host form, and only for LONG polynomials:
//   I_r, Z_r of a register with more than `min_assertions` assertions: their coefficients from gs_boundary_polys (what prove() builds
//            them with), evaluated by gs_eval_polys_at_points — instead of boundary_values_tree (a host product tree, a T-point host
//            transform and m barycentric terms per point);
//   the column of a public input register whose shortest period exceeds `min_column`: uploaded, gs_interpolate_roots,
//            gs_eval_polys_at_points — instead of cyclic_poly + horner_many.
// Both are the same field elements (unique polynomials, exact arithmetic), read back with ONE gs_download.  Whatever the host form
// refuses of a statement is refused here first, with its message, before anything is enqueued.
struct DeviceVerify {
    gs_ctx *c;
    size_t min_assertions;
    uint64_t min_column;
};
struct DeviceColumn { size_t at; std::vector<F> values; };      // static register `at`: one period of its column
// may the device build this register's boundary polynomials?  (Throws what the host form would throw of it.)
bool device_boundary_fits(const Plan &plan, const Plan::Reg &r) {
    if (plan.E < 2 || plan.T > (1ull << 28)) return false;          // gs_boundary_polys: a domain of at least 2 T points, T <= 2^28
    if (r.steps.size() > BOUNDARY_DIRECT_MAX) { check_many_assertions(plan, r); return true; }
    // (below BOUNDARY_DIRECT_MAX — reached with the thresholds lowered — the host's direct form is the judge of a repeated step)
    std::vector<uint64_t> sorted(r.steps);
    std::sort(sorted.begin(), sorted.end());
    return std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end() && sorted.back() < plan.T;
}
void device_values(const DeviceVerify &dev, const Plan &plan, const std::vector<F> &points, const std::vector<size_t> &regs, std::vector<BoundaryValues> &bvals,
                   const std::vector<DeviceColumn> &columns, std::vector<std::vector<F>> &column_values) {
    Ctx x{dev.c};
    const uint32_t Q = (uint32_t)points.size(), nb = (uint32_t)regs.size();
    column_values.assign(columns.size(), std::vector<F>());
    if (!Q) return;
    auto evaluate = [&](const void *polys, uint32_t rows, uint64_t stride, const std::vector<uint64_t> &lens, const Bytes &at, void *out) {
        x.check(A.gs_eval_polys_at_points(x.c, polys, rows, stride, lens.data(), at.data(), Q, out), "gs_eval_polys_at_points");
    };
    Buf out(x, (2ull * nb + columns.size()) * Q * ELEM);
    Buf iPolys, zPolys;
    if (nb) {
        uint32_t width = 0;
        for (size_t k : regs) width = std::max(width, (uint32_t)plan.regs[k].steps.size());
        std::vector<uint64_t> at((size_t)nb * width, 0), ilen(nb), zlen(nb);
        std::vector<uint32_t> per_row(nb);
        Bytes ys((size_t)nb * width * ELEM, 0);
        for (uint32_t r = 0; r < nb; r++) {
            const Plan::Reg &d = plan.regs[regs[r]];
            per_row[r] = (uint32_t)d.steps.size(); ilen[r] = d.steps.size(); zlen[r] = d.steps.size() + 1;
            for (size_t k = 0; k < d.steps.size(); k++) {
                at[(size_t)r * width + k] = d.steps[k];
                store_elem(d.ys[k], ys.data() + ((size_t)r * width + k) * ELEM);
            }
        }
        iPolys = Buf(x, (uint64_t)nb * width * ELEM);
        zPolys = Buf(x, (uint64_t)nb * (width + 1ull) * ELEM);
        x.check(A.gs_boundary_polys(x.c, enc(plan.omega), plan.N, plan.T, at.data(), ys.data(), per_row.data(), nb, width, iPolys.p, zPolys.p), "gs_boundary_polys");
        const Bytes pts = pack(points, 0, Q);
        evaluate(iPolys.p, nb, width, ilen, pts, out.p);
        evaluate(zPolys.p, nb, width + 1ull, zlen, pts, out.at((uint64_t)nb * Q * ELEM));
    }
    // columns of one period share an upload, a transform, their points x^(T / period) and an evaluation
    std::map<uint64_t, std::vector<size_t>> by_period;
    for (size_t k = 0; k < columns.size(); k++) by_period[columns[k].values.size()].push_back(k);
    std::vector<uint64_t> row_of(columns.size());
    uint64_t row = 2ull * nb;
    std::vector<Buf> held;
    for (auto &g : by_period) {
        const uint64_t m = g.first;
        const uint32_t cnt = (uint32_t)g.second.size();
        Bytes host(cnt * m * ELEM);
        for (uint32_t j = 0; j < cnt; j++) {
            const std::vector<F> &v = columns[g.second[j]].values;
            for (uint64_t i = 0; i < m; i++) store_elem(v[i], host.data() + (j * m + i) * ELEM);
            row_of[g.second[j]] = row + j;
        }
        held.emplace_back(x, host.size());
        held.emplace_back(x, host.size());
        Buf &ys = held[held.size() - 2], &poly = held.back();
        x.check(A.gs_upload(x.c, ys.p, host.data(), host.size()), "gs_upload(input register columns)");
        x.check(A.gs_interpolate_roots(x.c, ys.p, cnt, enc(hf_pow(plan.omega, (hfe)(plan.E * (plan.T / m)))), m, poly.p), "gs_interpolate_roots(input register columns)");
        std::vector<F> at(Q);
        for (uint32_t q = 0; q < Q; q++) at[q] = hf_pow(points[q], (hfe)(plan.T / m));
        evaluate(poly.p, cnt, m, std::vector<uint64_t>(cnt, m), pack(at, 0, Q), out.at(row * Q * ELEM));
        row += cnt;
    }
    Bytes back((size_t)row * Q * ELEM);
    x.check(A.gs_download(x.c, back.data(), out.p, back.size()), "gs_download(values at the queried points)");
    auto take = [&](uint64_t r) {
        std::vector<F> v(Q);
        for (uint32_t q = 0; q < Q; q++) v[q] = load_elem(back.data() + (r * Q + q) * ELEM);
        return v;
    };
    for (uint32_t r = 0; r < nb; r++) { bvals[regs[r]].i_at = take(r); bvals[regs[r]].z_at = take((uint64_t)nb + r); }
    for (size_t k = 0; k < columns.size(); k++) column_values[k] = take(row_of[k]);
}

// dev = null: everything on this host core (gs_prover_verify)
void verify_impl(const gs_prover_job &job, const uint8_t *proof, uint64_t proof_len, const DeviceVerify *dev) {
    const gs_prover_air &air = job.air;
    const AirProgram evaluator{air.e_code, air.e_ninstr, air.consts, air.nconsts, air.vm_regs, air.registers, air.nstatic, air.nconstraints};
    char emsg[96] = "air program: its constants are missing";
    if (air.kind == 1 && ((air.nconsts && !air.consts) || !air_validate(evaluator, true, true, emsg, sizeof emsg))) fail(GS_ERR_ARG, "%s", emsg);
    const uint64_t E = job.extension_factor;
    const uint32_t R = air.registers, S = air.nsecret;
    const int alg = job.hash_alg;
    if (!E || (E & (E - 1)) || !R || !air.nconstraints) fail(GS_ERR_ARG, "invalid job");
    if (job.nassertions < 1) fail(GS_ERR_ARG, "At least one assertion must be provided");
    if (alg != GS_HASH_SHA256 && alg != GS_HASH_BLAKE2S256) fail(GS_ERR_ARG, "unknown hash algorithm");
    if (air.ninputs && (air.kind != 1 || !air.inputs)) fail(GS_ERR_ARG, "invalid job: input registers belong to a program AIR and need their declarations");

    // ----- parse (lib/Serializer.ts:83-144)
    Reader r{proof, proof_len};
    const uint8_t *evr = r.take(DIGEST);
    Bytes evRoot(evr, evr + DIGEST);
    ParsedMerkleProof evProof = read_merkle_proof(r, (uint64_t)(R + S) * ELEM);
    const uint8_t *lcr = r.take(DIGEST);
    Bytes lcRoot(lcr, lcr + DIGEST);
    ParsedMerkleProof lcProof = read_merkle_proof(r, 4 * ELEM);
    const uint32_t ncomp = r.byte();
    struct Comp { Bytes columnRoot; ParsedMerkleProof columnProof, polyProof; };
    std::vector<Comp> comps(ncomp);
    for (auto &c : comps) {
        const uint8_t *cr = r.take(DIGEST);
        c.columnRoot.assign(cr, cr + DIGEST);
        c.columnProof = read_merkle_proof(r, 4 * ELEM);
        c.polyProof = read_merkle_proof(r, 4 * ELEM);
    }
    uint32_t rlen = r.byte();
    if (!rlen) rlen = (uint32_t)MAX_ARRAY;
    std::vector<F> remainder(rlen);
    for (uint32_t i = 0; i < rlen; i++) remainder[i] = load_elem(r.take(ELEM));
    // input shapes (lib/Serializer.ts:127-141) — and with them the trace length: the reference sizes the trace from the proof's shapes
    // (initVerificationContext(proof.iShapes, publicInputs), lib/Stark.ts:176).  An AIR without input registers has a fixed trace
    // (job.steps) and a proof of it carries no shapes.
    Shapes shapes;
    {
        const uint32_t nshapes = r.byte();
        shapes.resize(nshapes);
        for (auto &sh : shapes) {
            const uint32_t rank = r.byte();
            const uint8_t *q = r.take(4ull * rank);
            sh.resize(rank);
            for (uint32_t k = 0; k < rank; k++) sh[k] = (uint32_t)q[4 * k] | ((uint32_t)q[4 * k + 1] << 8) | ((uint32_t)q[4 * k + 2] << 16) | ((uint32_t)q[4 * k + 3] << 24);
        }
    }
    // (bytes after the shapes are ignored, as lib/Serializer.ts:83-144 ignores them)
    uint64_t T = job.steps;
    InputLayout layout;
    if (air.ninputs) {
        layout = input_layout(air, shapes);
        if (job.steps && job.steps != layout.length)
            fail(GS_ERR_ARG, "the proof's input shapes lay out a trace of %llu steps, the statement is about %llu", (unsigned long long)layout.length, (unsigned long long)job.steps);
        T = layout.length;
    } else if (!shapes.empty()) {
        fail(GS_ERR_ARG, "malformed proof: %zu input shapes for an AIR without input registers", shapes.size());
    }
    if (!T || (T & (T - 1))) fail(GS_ERR_ARG, "invalid job");
    if (T > (1ull << 32) / E) fail(GS_ERR_ARG, "a trace of %llu steps at extension factor %llu is beyond this verifier", (unsigned long long)T, (unsigned long long)E);
    const uint64_t N = T * E;
    const F omega = domain_root(job, N);
    // (the assertions' points are what the HOST forms of the boundary values work on: with a device they wait for the first register that needs them)
    Plan plan = make_plan(job, T, E, omega, dev == nullptr);
    bool have_xs = dev == nullptr;
    const uint64_t combination_degree = plan.combination_degree, b_inc = plan.b_inc;
    // the number of FRI layers is a function of the domain size alone (LowDegreeProver.ts:179: fold while more than 256 values are
    // left); a proof with any other count is malformed — in particular one with extra layers, which would floor the degree bound of
    // the remainder to zero and leave the low-degree test with nothing to check
    {
        uint32_t want = 0;
        for (uint64_t len = N; len > MAX_ARRAY; len /= 4) want++;
        if (ncomp != want) fail(GS_ERR_ARG, "malformed proof: %u FRI components, %u expected for a domain of %llu", ncomp, want, (unsigned long long)N);
        const uint64_t rem_want = N >> (2 * want);
        if (rlen != rem_want) fail(GS_ERR_ARG, "malformed proof: remainder of %u values, %llu expected", rlen, (unsigned long long)rem_want);
    }

    // ----- composition polynomial set-up (CompositionPolynomial.ts:29-69): the same coefficient stream as the prover's
    for (uint32_t i = 0; i < job.nassertions; i++) {
        const gs_assertion &a = job.assertions[i];
        if (a.reg >= R) fail(GS_ERR_ARG, "Invalid assertion: register %u is outside of register bank", a.reg);
        if (a.step >= T) fail(GS_ERR_ARG, "Invalid assertion: step %llu is outside of execution trace", (unsigned long long)a.step);
    }
    const std::vector<Plan::Reg> &rdata = plan.regs;
    const uint32_t bcount = (uint32_t)rdata.size(), dcount = plan.dcount, bcoef = plan.bcoef, V = R + S;
    const std::vector<F> coeffs = plan.coefficients(evRoot, V);
    const F x_last = hf_pow(omega, (hfe)((T - 1) * E));

    // static registers of the AIR at a point (kind 1: K_s(x^(T/period)); kind 0: the round-constant register)
    std::vector<std::vector<F>> static_polys;
    std::vector<uint64_t> static_periods;
    std::vector<DeviceColumn> device_columns;                                 // (their entries of static_polys stay empty)
    if (air.kind == 0) {
        if (!air.nrc || !air.round_constants) fail(GS_ERR_ARG, "the MiMC AIR needs its round constants");
        if ((air.nrc & (air.nrc - 1)) || T % air.nrc) fail(GS_ERR_ARG, "invalid job: the number of round constants must be a power of two dividing the trace length");
        std::vector<F> rc(air.nrc);
        for (uint32_t i = 0; i < air.nrc; i++) rc[i] = load_elem(air.round_constants + ELEM * i);
        static_polys.push_back(cyclic_poly(rc, hf_pow(omega, (hfe)(E * (T / air.nrc)))));
        static_periods.push_back(air.nrc);
    } else {
        if (air.nstatic < S) fail(GS_ERR_ARG, "static register list shorter than the secret register count");
        if (air.ninputs && !air.static_sources) fail(GS_ERR_ARG, "invalid job: an AIR with input registers says where each static register takes its values from");
        // which public input register's values are the k-th list of public_inputs (declaration order, lib/Stark.ts:167)
        std::vector<int64_t> public_at(air.ninputs, -1);
        std::vector<uint64_t> public_off;
        if (air.ninputs) {
            uint32_t k = 0;
            uint64_t off = 0;
            for (uint32_t j = 0; j < air.ninputs; j++) {
                if (air.inputs[j].secret) continue;
                if (k >= air.npublic_inputs || !air.public_input_counts || (!air.public_inputs && air.public_input_counts[k]))
                    fail(GS_ERR_ARG, "the values of %u public input registers are needed", (unsigned)std::count_if(air.inputs, air.inputs + air.ninputs, [](const gs_input_register &d) { return !d.secret; }));
                if (air.public_input_counts[k] != layout.count[j]) fail(GS_ERR_ARG, "public input register %u: %llu values expected (the shape in the proof), %llu given", j, (unsigned long long)layout.count[j], (unsigned long long)air.public_input_counts[k]);
                public_at[j] = k++;
                public_off.push_back(off);
                off += layout.count[j];
            }
        }
        uint64_t off = 0;
        uint32_t cyc = 0;
        for (uint32_t s = 0; s + S < air.nstatic; s++) {                     // the public ones (the secret ones follow them and arrive in the leaves)
            const gs_static_source src = air.static_sources ? air.static_sources[s] : gs_static_source{GS_STATIC_CYCLE, 0};
            std::vector<F> vals;
            if (src.kind == GS_STATIC_CYCLE) {
                const uint32_t m = air.static_periods[cyc++];
                if (!m || (m & (m - 1)) || T % m) fail(GS_ERR_ARG, "a static register's period must be a power of two dividing the trace length");
                vals.resize(m);
                for (uint32_t i = 0; i < m; i++) vals[i] = load_elem(air.static_values + ELEM * (off + i));
                off += m;
            } else if (src.kind == GS_STATIC_INPUT || src.kind == GS_STATIC_MASK) {
                // the column the loader lays out (airassembly.py: _Layout.column / .mask): every value held for `span` steps — or a 1
                // on the first of them —, the whole rotated by the register's shift, then cut to its shortest period
                const uint32_t j = src.index;
                if (j >= air.ninputs) fail(GS_ERR_ARG, "invalid job: static register %u names input register %u of %u", s, j, air.ninputs);
                if (T > (1ull << 26)) fail(GS_ERR_ARG, "a trace of %llu steps is beyond this verifier's input-register columns", (unsigned long long)T);
                const uint64_t span = layout.span[j];
                if (src.kind == GS_STATIC_MASK) {
                    // one period of the mask is all there is to it (span divides the power of two T, so it is a power of two itself): a
                    // proof cannot make the verifier build a trace-length column out of its shapes alone
                    vals.assign(span, (F)0);
                    vals[0] = (F)1;
                } else {
                    vals.resize(T);
                    if (air.inputs[j].secret || public_at[j] < 0) fail(GS_ERR_ARG, "invalid job: static register %u is a public one, input register %u is secret", s, j);
                    const uint8_t *src_vals = air.public_inputs + ELEM * public_off[public_at[j]];
                    for (uint64_t v = 0; v < layout.count[j]; v++) {
                        const F val = load_elem(src_vals + ELEM * v);
                        for (uint64_t i = 0; i < span; i++) vals[v * span + i] = val;
                    }
                }
                rotate_column(vals, air.inputs[j].shift);
                shrink_column(vals);
            } else {
                fail(GS_ERR_ARG, "invalid job: static register %u has unknown source %u", s, src.kind);
            }
            const uint64_t m = vals.size();
            if (dev && src.kind == GS_STATIC_INPUT && m > dev->min_column) {
                device_columns.push_back(DeviceColumn{static_polys.size(), std::move(vals)});
                static_polys.emplace_back();
            } else {
                static_polys.push_back(cyclic_poly(vals, hf_pow(omega, (hfe)(E * (T / m)))));
            }
            static_periods.push_back(m);
        }
    }
    // statics_at[k][pi]: static register k at the pi-th queried point (filled below, once the positions are known)
    std::vector<std::vector<F>> statics_at;
    auto constraints_at = [&](size_t pi, const std::vector<F> &p, const std::vector<F> &n, const std::vector<F> &s) {
        std::vector<F> statics;
        for (size_t k = 0; k < static_polys.size(); k++) statics.push_back(statics_at[k][pi]);
        if (air.kind == 0) {                                                 // examples/mimc/mimc128Assembly.ts:46-51
            const F x3 = hf_mul(hf_mul(p[0], p[0]), p[0]);
            return std::vector<F>{hf_sub(n[0], hf_add(x3, statics[0]))};
        }
        for (F v : s) statics.push_back(v);
        return run_program(evaluator, p, n, statics);
    };

    // ----- spot-check positions and the evaluation tree (lib/Stark.ts:183-216)
    const std::vector<uint64_t> positions = plan.exe_positions(lcRoot), aug = plan.evaluation_positions(positions);
    if (evProof.values.size() != aug.size()) fail(GS_ERR_ARG, "malformed proof: the evaluation proof does not hold one leaf per queried position");
    std::map<uint64_t, size_t> at_leaf;
    for (size_t i = 0; i < aug.size(); i++) at_leaf[aug[i]] = i;
    auto leaf_values = [&](uint64_t pos, std::vector<F> &p, std::vector<F> &s) {
        const Bytes &b = evProof.values[at_leaf.at(pos)];
        p.resize(R); s.resize(S);
        for (uint32_t k = 0; k < R; k++) p[k] = load_elem(b.data() + ELEM * k);
        for (uint32_t k = 0; k < S; k++) s[k] = load_elem(b.data() + ELEM * (R + k));
    };
    if (!merkle_check(alg, evRoot, aug, evProof)) fail(GS_ERR_ARG, "Verification of evaluation Merkle proof failed");

    // ----- transition and boundary constraints at every position (:218-234; CompositionPolynomial.ts:150-191; LinearCombination.ts:66-88)
    // (the divisions of all positions share one inversion: first the denominators — x^T - 1 of Z(x), Z_r(x) of every asserted register —
    //  then the values)
    std::vector<F> lcValues, xsq, dens;
    for (uint64_t step : positions) xsq.push_back(hf_pow(omega, (hfe)step));
    std::vector<BoundaryValues> bvals;                                    // per asserted register: I_r and Z_r at every queried point (BoundaryConstraints.ts:42, :24-30)
    std::vector<size_t> device_regs;                                      // ... of these the device provides them (filled in below)
    for (size_t k = 0; k < rdata.size(); k++) {
        const Plan::Reg &d = rdata[k];
        if (dev && d.steps.size() > dev->min_assertions && device_boundary_fits(plan, d)) { device_regs.push_back(k); bvals.emplace_back(); continue; }
        if (!have_xs) { plan.fill_xs(); have_xs = true; }
        bvals.push_back(d.steps.size() <= BOUNDARY_DIRECT_MAX ? boundary_values_direct(plan, d, xsq) : boundary_values_tree(plan, d, xsq));
    }
    std::vector<std::vector<F>> device_column_values;
    if (dev && (!device_regs.empty() || !device_columns.empty())) device_values(*dev, plan, xsq, device_regs, bvals, device_columns, device_column_values);
    for (size_t pi = 0; pi < positions.size(); pi++) {
        dens.push_back(hf_sub(hf_pow(xsq[pi], (hfe)T), 1));                                            // ZeroPolynomial.ts:28-34: Z = (x^T - 1) / (x - x_last)
        for (auto &bv : bvals) dens.push_back(bv.z_at[pi]);                                         // BoundaryConstraints.ts:55-69
    }
    host_batch_invert(dens);
    for (size_t k = 0, dc = 0; k < static_polys.size(); k++) {                // K_s(x^(T/period)) at every queried x
        if (dc < device_columns.size() && device_columns[dc].at == k) { statics_at.push_back(std::move(device_column_values[dc++])); continue; }
        std::vector<F> at(xsq.size());
        for (size_t pi = 0; pi < xsq.size(); pi++) at[pi] = hf_pow(xsq[pi], (hfe)(T / static_periods[k]));
        statics_at.push_back(horner_many(static_polys[k], at));
    }
    size_t di = 0;
    for (size_t pi = 0; pi < positions.size(); pi++) {
        const uint64_t step = positions[pi];
        const F x = xsq[pi];
        std::vector<F> p, n, s, unused;
        leaf_values(step, p, s);
        leaf_values((step + E) % N, n, unused);
        std::vector<F> q = constraints_at(pi, p, n, s);
        if (q.size() != air.nconstraints) fail(GS_ERR_ARG, "constraint evaluator returned the wrong number of values");
        for (auto &g : plan.groups) {
            if (g.first == combination_degree) continue;
            const F power = hf_pow(x, (hfe)(combination_degree - g.first));
            for (uint32_t i : g.second) q.push_back(hf_mul(q[i], power));
        }
        F qc = 0;
        for (size_t k = 0; k < q.size(); k++) qc = hf_add(qc, hf_mul(q[k], coeffs[k]));
        const F dValue = hf_mul(hf_mul(qc, hf_sub(x, x_last)), dens[di++]);                             // Q / Z = Q (x - x_last) / (x^T - 1)
        std::vector<F> b;
        for (uint32_t r = 0; r < bcount; r++) b.push_back(hf_mul(hf_sub(p[rdata[r].reg], bvals[r].i_at[pi]), dens[di++]));
        const F xb = hf_pow(x, (hfe)b_inc);
        if (b_inc > 0) for (uint32_t i = 0; i < bcount; i++) b.push_back(hf_mul(b[i], xb));
        F bValue = 0;
        for (size_t k = 0; k < b.size(); k++) bValue = hf_add(bValue, hf_mul(b[k], coeffs[dcount + k]));
        const F cValue = hf_add(dValue, bValue);
        std::vector<F> ps(p);
        ps.insert(ps.end(), s.begin(), s.end());
        if (b_inc > 0) for (uint32_t i = 0; i < V; i++) ps.push_back(hf_mul(ps[i], xb));
        F comb = 0;
        for (size_t k = 0; k < ps.size(); k++) comb = hf_add(comb, hf_mul(ps[k], coeffs[dcount + bcoef + k]));
        lcValues.push_back(hf_add(cValue, comb));
    }

    // ----- low-degree proof (LowDegreeProver.ts:70-172)
    uint64_t column_length = N;
    auto column_values = [&](const ParsedMerkleProof &mp, const std::vector<uint64_t> &pos, const std::vector<uint64_t> &rows, uint64_t clen) {   // :264-282
        const uint64_t row_len = clen / 4;
        std::vector<F> out;
        for (uint64_t p : pos) {
            size_t idx = rows.size();
            for (size_t k = 0; k < rows.size(); k++) if (rows[k] == p % row_len) { idx = k; break; }
            if (idx >= mp.values.size()) fail(GS_ERR_ARG, "malformed proof: a queried row is missing");
            out.push_back(load_elem(mp.values[idx].data() + ELEM * (p / row_len)));
        }
        return out;
    };
    {
        const std::vector<uint64_t> lc_rows = augmented_rows(positions, column_length);
        if (lcProof.values.size() != lc_rows.size()) fail(GS_ERR_ARG, "malformed proof: the linear-combination proof does not hold one row per queried position");
        const std::vector<F> checks = column_values(lcProof, positions, lc_rows, column_length);
        if (!merkle_check(alg, lcRoot, lc_rows, lcProof)) fail(GS_ERR_ARG, "Verification of linear combination Merkle proof failed");
        for (size_t i = 0; i < lcValues.size(); i++)
            if (lcValues[i] != checks[i]) fail(GS_ERR_ARG, "Verification of linear combination correctness failed");
    }
    Bytes pRoot = lcRoot;
    F rou = omega;
    uint64_t max_degree_plus1 = plan.composition_degree;
    column_length /= 4;
    const F zeta[4] = {(F)1, hf_pow(omega, (hfe)(N / 4)), hf_pow(omega, (hfe)(N / 2)), hf_pow(omega, (hfe)(N / 4 * 3))};      // :75-77
    const F inv4 = hf_inv((F)4);
    uint64_t domain_size = N;                  // order of `rou`
    for (uint32_t depth = 0; depth < ncomp; depth++) {
        Comp &c = comps[depth];
        if (column_length < 4) fail(GS_ERR_ARG, "malformed proof: too many FRI components");
        const Plan::Queries q = plan.layer_queries(c.columnRoot, column_length);
        const std::vector<uint64_t> &pos = q.positions, &rows = q.rows;
        if (c.columnProof.values.size() != rows.size() || c.polyProof.values.size() != pos.size()) fail(GS_ERR_ARG, "malformed proof: wrong number of rows at depth %u", depth);
        const std::vector<F> col = column_values(c.columnProof, pos, rows, column_length);
        if (!merkle_check(alg, c.columnRoot, rows, c.columnProof)) fail(GS_ERR_ARG, "Verification of column Merkle proof failed at depth %u", depth);
        if (!merkle_check(alg, pRoot, pos, c.polyProof)) fail(GS_ERR_ARG, "Verification of polynomial Merkle proof failed at depth %u", depth);
        const F special = prng_one(pRoot);                                                            // :132
        // the cubic through (x zeta^k, y_k), k < 4 (:123-137: interpolateQuarticBatch + evalQuarticBatch), evaluated at `special`:
        // (u0 + u1 t + u2 t^2 + u3 t^3) / 4 with u the inverse 4-point DFT of y and t = special / x — the same polynomial, no
        // inversion per position (x^-1 = rou^(order - position))
        for (size_t i = 0; i < pos.size(); i++) {
            const F xinv = hf_pow(rou, (hfe)((domain_size - pos[i]) % domain_size));
            F y[4];
            for (int k = 0; k < 4; k++) y[k] = load_elem(c.polyProof.values[i].data() + ELEM * k);
            const F s0 = hf_add(y[0], y[2]), s1 = hf_sub(y[0], y[2]), s2 = hf_add(y[1], y[3]), s3 = hf_mul(hf_sub(y[1], y[3]), zeta[3]);     // zeta^-1 = zeta^3
            const F u0 = hf_add(s0, s2), u2 = hf_sub(s0, s2), u1 = hf_add(s1, s3), u3 = hf_sub(s1, s3);
            const F t = hf_mul(special, xinv);
            F v = hf_add(hf_mul(u3, t), u2);
            v = hf_add(hf_mul(v, t), u1);
            v = hf_add(hf_mul(v, t), u0);
            if (hf_mul(v, inv4) != col[i]) fail(GS_ERR_ARG, "Degree 4 polynomial didn't evaluate to column value at depth %u", depth);
        }
        domain_size /= 4;
        pRoot = c.columnRoot;
        rou = hf_pow(rou, (hfe)4);
        max_degree_plus1 /= 4;
        column_length /= 4;
    }
    // ----- remainder (:155-171)
    if (max_degree_plus1 > remainder.size()) fail(GS_ERR_ARG, "Remainder degree is greater than number of remainder values");
    // the bound is floor(floor(d / 4) / 4 ...): with a tiny trace under a large extension factor it floors to 0 although a fold never
    // takes a polynomial below a constant.  Untrusted input never gets the prover's `m == 0: nothing to check` shortcut: the remainder
    // must then be a constant (the ceiling of the same divisions)
    if (!max_degree_plus1) max_degree_plus1 = 1;
    if (remainder.size() < 4 || (remainder.size() & 3)) fail(GS_ERR_ARG, "malformed proof: remainder length");
    {
        // the tree over the rows of transposeVector(remainder, 4) must be the last column's tree
        const uint64_t rows = remainder.size() / 4;
        std::vector<Bytes> level(rows, Bytes(32));
        for (uint64_t i = 0; i < rows; i++) {
            uint8_t msg[4 * GS_PROVER_ELT_MAX];
            for (int k = 0; k < 4; k++) store_elem(remainder[i + k * rows], msg + ELEM * k);
            host_digest(alg, msg, 4 * ELEM, level[i].data());
        }
        if (rows & (rows - 1)) fail(GS_ERR_ARG, "malformed proof: remainder length");
        while (level.size() > 1) {
            std::vector<Bytes> up(level.size() / 2, Bytes(32));
            for (size_t i = 0; i < up.size(); i++) {
                uint8_t buf[64];
                memcpy(buf, level[2 * i].data(), 32); memcpy(buf + 32, level[2 * i + 1].data(), 32);
                host_digest(alg, buf, 64, up[i].data());
            }
            level.swap(up);
        }
        if (level[0] != pRoot) fail(GS_ERR_ARG, "Remainder values do not match Merkle root of the last column");
    }
    if (!remainder_is_low_degree(remainder, E, max_degree_plus1, rou, 1))                              // :223-252
        fail(GS_ERR_ARG, "Remainder is not a valid degree %llu polynomial", (unsigned long long)(max_degree_plus1 - 1));
}

}  // namespace

extern "C" {

static int verify_entry(const struct gs_prover_job *job, const uint8_t *proof, uint64_t len, char *err, uint64_t errcap) {
    if (!job || !proof) return GS_ERR_ARG;
    return guarded(err, errcap, GS_ERR_ARG, [&]() -> int {
        verify_impl(*job, proof, len, nullptr);
        return GS_OK;
    });
}
// Thresholds of the device providers.  Measured (tools/verify_device_bench.py, profiles/verify_device.md): NOT YET — the values below are
// where the host's own forms change (BOUNDARY_DIRECT_MAX) and an estimate for the columns.
const uint32_t VERIFY_DEVICE_MIN_ASSERTIONS = 256;
const uint64_t VERIFY_DEVICE_MIN_COLUMN = 1024;
static thread_local uint32_t g_verify_min_assertions = 0;      // gs_prover_verify_device_min: 0 = the default
static thread_local uint64_t g_verify_min_column = 0;
static int verify_device_entry(gs_ctx *ctx, const struct gs_prover_job *job, const uint8_t *proof, uint64_t len, char *err, uint64_t errcap) {
    if (!ctx || !job || !proof) return GS_ERR_ARG;
    return guarded(err, errcap, GS_ERR_ARG, [&]() -> int {
        const DeviceVerify dev{ctx, g_verify_min_assertions ? g_verify_min_assertions : VERIFY_DEVICE_MIN_ASSERTIONS,
                               g_verify_min_column ? g_verify_min_column : VERIFY_DEVICE_MIN_COLUMN};
        // a library without the two optional entries (a test double): the host providers answer
        verify_impl(*job, proof, len, A.gs_boundary_polys && A.gs_eval_polys_at_points ? &dev : nullptr);
        return GS_OK;
    });
}
// I_r(x) and Z_r(x) of one asserted register at `npoints` points outside the execution domain, for tests (include/gstark_boundary.h)
static int boundary_at_entry(const uint8_t *omega, uint64_t n, uint64_t steps, const uint64_t *at, const uint8_t *values, uint32_t m, const uint8_t *points,
                             uint32_t npoints, int method, uint8_t *i_out, uint8_t *z_out, char *err, uint64_t errcap) {
    if (!omega || !at || !values || !m || (npoints && (!points || !i_out || !z_out)) || (method != 0 && method != 1)) return GS_ERR_ARG;
    if (!steps || (steps & (steps - 1)) || !n || (n & (n - 1)) || n < steps) return GS_ERR_ARG;
    return guarded(err, errcap, GS_ERR_OOM, [&]() -> int {
        Plan plan;
        plan.T = steps; plan.N = n; plan.E = n / steps; plan.omega = load_elem(omega);
        plan.regs.push_back(Plan::Reg{0, {}, {}, {}});
        Plan::Reg &r = plan.regs[0];
        for (uint32_t i = 0; i < m; i++) { r.steps.push_back(at[i]); r.ys.push_back(load_elem(values + ELEM * i)); }
        plan.fill_xs();
        std::vector<F> pts(npoints);
        for (uint32_t q = 0; q < npoints; q++) pts[q] = load_elem(points + ELEM * q);
        const BoundaryValues bv = method ? boundary_values_tree(plan, r, pts) : boundary_values_direct(plan, r, pts);
        for (uint32_t q = 0; q < npoints; q++) { store_elem(bv.i_at[q], i_out + ELEM * q); store_elem(bv.z_at[q], z_out + ELEM * q); }
        return GS_OK;
    });
}
int gs_prover_boundary_at_on(const gs_prover_binding *b, const uint8_t *omega, uint64_t n, uint64_t steps, const uint64_t *at, const uint8_t *values, uint32_t m,
                             const uint8_t *points, uint32_t npoints, int method, uint8_t *i_out, uint8_t *z_out, char *err, uint64_t errcap) {
    if (!b) return GS_ERR_ARG;
    UseApi use(reinterpret_cast<const Api *>(b));
    return boundary_at_entry(omega, n, steps, at, values, m, points, npoints, method, i_out, z_out, err, errcap);
}
int gs_prover_verify(const struct gs_prover_job *job, const uint8_t *proof, uint64_t len, char *err, uint64_t errcap) {
    if (!g_bound) return GS_ERR_UNSUPPORTED;
    UseApi use(&g_default_api);
    return verify_entry(job, proof, len, err, errcap);
}
int gs_prover_verify_on(const gs_prover_binding *b, const struct gs_prover_job *job, const uint8_t *proof, uint64_t len, char *err, uint64_t errcap) {
    if (!b) return GS_ERR_ARG;
    UseApi use(reinterpret_cast<const Api *>(b));
    return verify_entry(job, proof, len, err, errcap);
}
int gs_prover_verify_device(gs_ctx *ctx, const struct gs_prover_job *job, const uint8_t *proof, uint64_t len, char *err, uint64_t errcap) {
    if (!g_bound) return GS_ERR_UNSUPPORTED;
    UseApi use(&g_default_api);
    return verify_device_entry(ctx, job, proof, len, err, errcap);
}
int gs_prover_verify_device_on(const gs_prover_binding *b, gs_ctx *ctx, const struct gs_prover_job *job, const uint8_t *proof, uint64_t len, char *err,
                               uint64_t errcap) {
    if (!b) return GS_ERR_ARG;
    UseApi use(reinterpret_cast<const Api *>(b));
    return verify_device_entry(ctx, job, proof, len, err, errcap);
}
void gs_prover_verify_device_min(uint32_t assertions, uint64_t column) { g_verify_min_assertions = assertions; g_verify_min_column = column; }

}  // extern "C"
