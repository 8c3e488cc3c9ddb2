// diagnose.h — gs_prover_diagnose (include/gstark_diagnose.h): why a statement does not prove.  Included by prover.cc, whose helpers
// (Ctx, Buf, the job checks, launch_trace, the counted transforms) it uses; like the prover it is written against the C ABI only.
//
// prove() runs the whole proof and then fails its remainder check with one sentence, whichever of three things is wrong.  The diagnosis
// takes the same job, commits to nothing, and looks at each of them where it shows:
//   (a) the assertions: EVERY asserted cell of the trace that holds another value (prove names the first);
//   (b) the constraints on the trace itself: the evaluator — the same programs, interpreted or compiled, that prove() runs — over the
//       T trace rows (gs_air_constraints with nc = T, shift = 1: "next row" is the next step), then gs_nonzero_spans over the steps
//       [0, T - 1): the last step is exempt (ZeroPolynomial.ts:36-44).  A static register at step j is values[j mod period], the
//       trace's own rule, so the concatenated static_values serve as the evaluator's tables with lens = static_periods;
//   (c) the constraints as polynomials: the evaluator over the trace polynomials on 2 * Nc points (Nc = composition_factor * T), the
//       rows interpolated, and the last non-zero coefficient of each = its degree, against what its DECLARED degree lets through
//       (CompositionPolynomial.ts:37-43,88-99,196-204).
// A library without gs_nonzero_spans (the tests' double) has the matrices downloaded and scanned here.

namespace {

struct Spans { std::vector<uint64_t> count, first, last; };
// per row of m (rows x row_stride elements on the device) over the columns [0, n)
Spans nonzero_spans(Ctx &x, const void *m, uint64_t rows, uint64_t row_stride, uint64_t n) {
    Spans s;
    s.count.resize(rows); s.first.resize(rows); s.last.resize(rows);
    if (A.gs_nonzero_spans) {
        x.check(A.gs_nonzero_spans(x.c, m, rows, row_stride, n, s.count.data(), s.first.data(), s.last.data()), "gs_nonzero_spans");
        return s;
    }
    Bytes host(rows * row_stride * ELEM);
    x.check(A.gs_download(x.c, host.data(), m, host.size()), "gs_download(matrix to scan)");
    for (uint64_t r = 0; r < rows; r++) {
        s.count[r] = 0; s.first[r] = s.last[r] = n;
        for (uint64_t j = 0; j < n; j++) {
            const uint8_t *e = host.data() + (r * row_stride + j) * ELEM;
            bool nz = false;
            for (uint64_t b = 0; b < ELEM; b++) nz |= e[b] != 0;
            if (!nz) continue;
            if (!s.count[r]++) s.first[r] = j;
            s.last[r] = j;
        }
    }
    return s;
}

void diagnose_impl(Ctx &x, const gs_prover_job &job, gs_diagnose_constraint *constraints, uint32_t *nconstraints, gs_diagnose_assertion *assertions,
                   uint32_t assertions_cap, uint32_t *nassertions) {
    const gs_prover_air &air = job.air;
    const uint64_t T = job.steps, E = job.extension_factor, N = T * E;
    const uint32_t R = air.registers, K = air.nconstraints;
    *nconstraints = 0;
    *nassertions = 0;
    // what prove() refuses, in its order and its words
    check_job(job);
    checked_job_shapes(job);
    check_extension_factor(job);
    const F omega = domain_root(job, N);
    Buf trace(x, (uint64_t)R * T * ELEM);
    launch_trace(x, job, air.first_rows, air.segments, trace.p);
    check_assertion_ranges(job);

    // (a) every assertion the trace does not meet
    {
        std::vector<uint64_t> at;
        for (uint32_t i = 0; i < job.nassertions; i++) at.push_back((uint64_t)job.assertions[i].reg * T + job.assertions[i].step);
        Bytes got(at.size() * ELEM);
        x.check(A.gs_gather(x.c, trace.p, ELEM, at.data(), at.size(), got.data()), "gs_gather(asserted cells)");
        uint32_t bad = 0;
        for (uint32_t i = 0; i < job.nassertions; i++) {
            if (!memcmp(got.data() + i * ELEM, job.assertions[i].value, ELEM)) continue;
            if (bad < assertions_cap && assertions) {
                gs_diagnose_assertion &a = assertions[bad];
                memset(&a, 0, sizeof a);
                a.index = i;
                memcpy(a.found, got.data() + i * ELEM, ELEM);
            }
            bad++;
        }
        *nassertions = bad;
    }
    if (air.kind != 1) return;           // MiMC: transition and constraint are both the library's and cannot disagree
    if (!constraints) fail(GS_ERR_ARG, "invalid job: no room for the constraints' records");
    if (air.nstatic && (!air.static_values || !air.static_periods)) fail(GS_ERR_ARG, "invalid job: static registers without their values");
    for (uint32_t i = 0; i < K; i++) {
        memset(&constraints[i], 0, sizeof constraints[i]);
        constraints[i].declared = air.degrees[i];
    }

    // (b) the constraints on the trace
    uint64_t static_total = 0;
    std::vector<uint64_t> periods(air.nstatic ? air.nstatic : 1, 0);
    for (uint32_t s = 0; s < air.nstatic; s++) {
        const uint64_t m = air.static_periods[s];
        if (!m || (m & (m - 1)) || m > T) fail(GS_ERR_ARG, "invalid job: static register %u has %llu values for a trace of %llu steps", s, (unsigned long long)m, (unsigned long long)T);
        periods[s] = m;
        static_total += m;
    }
    Buf statics(x, static_total * ELEM);
    if (static_total) x.check(A.gs_upload(x.c, statics.p, air.static_values, static_total * ELEM), "gs_upload(static values)");
    {
        Buf q(x, (uint64_t)K * T * ELEM);
        x.check(A.gs_air_constraints(x.c, air.e_code, air.e_ninstr, air.consts, air.nconsts, air.vm_regs, R, K, trace.p, T, 1, statics.p, periods.data(), air.nstatic,
                                     q.p), "gs_air_constraints(trace)");
        if (T > 1) {
            const Spans s = nonzero_spans(x, q.p, K, T, T - 1);
            std::vector<uint64_t> at;
            std::vector<uint32_t> who;
            for (uint32_t i = 0; i < K; i++) {
                constraints[i].violations = s.count[i];
                constraints[i].first_step = s.first[i];
                constraints[i].last_step = s.last[i];
                if (s.count[i]) { at.push_back((uint64_t)i * T + s.first[i]); who.push_back(i); }
            }
            if (!at.empty()) {
                Bytes got(at.size() * ELEM);
                x.check(A.gs_gather(x.c, q.p, ELEM, at.data(), at.size(), got.data()), "gs_gather(violations)");
                for (size_t k = 0; k < who.size(); k++) memcpy(constraints[who[k]].first_value, got.data() + k * ELEM, ELEM);
            }
        }
    }

    // (c) the constraints as polynomials, over the 2 Nc points w2^j, w2 = omega^(N / 2 Nc)
    const uint64_t cf = composition_factor(air), Nc = cf * T, N2 = 2 * Nc;           // (check_extension_factor: N2 <= N)
    const uint64_t C = cf * T, composition_degree = std::max(C - T, T);
    const F w2 = hf_pow(omega, (hfe)(N / N2)), exec_rou = hf_pow(omega, (hfe)E);
    Buf pExt(x, (uint64_t)R * N2 * ELEM);
    {
        Buf pPolys(x, (uint64_t)R * T * ELEM);
        x.check(A.gs_interpolate_roots(x.c, trace.p, R, enc(exec_rou), T, pPolys.p), "gs_interpolate_roots(trace)");
        x.check(A.gs_eval_polys_at_roots(x.c, pPolys.p, R, T, enc(w2), N2, pExt.p), "gs_eval_polys_at_roots(P)");
    }
    trace.release();
    // each static register over those points, as the caller builds the composition-domain tables: the polynomial through its period's
    // values (at the period-th roots of unity), at 2 cf times as many roots
    std::vector<uint64_t> lens(periods);
    uint64_t table_total = 0;
    for (uint32_t s = 0; s < air.nstatic; s++) { lens[s] = periods[s] * 2 * cf; table_total += lens[s]; }
    Buf tables(x, table_total * ELEM);
    for (uint64_t s = 0, in = 0, out = 0; s < air.nstatic; in += periods[s], out += lens[s], s++) {
        const uint64_t m = periods[s];
        Buf poly(x, m * ELEM);
        if (m == 1) x.check(A.gs_copy(x.c, poly.p, statics.at(in * ELEM), ELEM), "gs_copy(static value)");      // a constant
        else x.check(A.gs_interpolate_roots(x.c, statics.at(in * ELEM), 1, enc(hf_pow(omega, (hfe)(N / m))), m, poly.p), "gs_interpolate_roots(static)");
        x.check(A.gs_eval_polys_at_roots(x.c, poly.p, 1, m, enc(hf_pow(omega, (hfe)(N / lens[s]))), lens[s], tables.at(out * ELEM)), "gs_eval_polys_at_roots(static)");
    }
    statics.release();
    Buf q(x, (uint64_t)K * N2 * ELEM), coef(x, (uint64_t)K * N2 * ELEM);
    x.check(A.gs_air_constraints(x.c, air.e_code, air.e_ninstr, air.consts, air.nconsts, air.vm_regs, R, K, pExt.p, N2, 2 * cf, tables.p, lens.data(), air.nstatic, q.p),
            "gs_air_constraints(extension)");
    x.check(A.gs_interpolate_roots(x.c, q.p, K, enc(w2), N2, coef.p), "gs_interpolate_roots(constraints)");
    const Spans s = nonzero_spans(x, coef.p, K, N2, N2);
    for (uint32_t i = 0; i < K; i++) {
        gs_diagnose_constraint &c = constraints[i];
        const uint64_t d = (uint64_t)c.declared * T;
        c.all_zero = s.count[i] ? 0 : 1;
        c.degree = s.count[i] ? s.last[i] : 0;
        c.limit = d < C ? (d >= 2 ? d - 2 : 0) : composition_degree + T - 2;
        c.needed = (uint32_t)((c.degree + 2 + T - 1) / T);
        c.at_least = !c.all_zero && c.degree >= N2 - T ? 1 : 0;
    }
    *nconstraints = K;
}

int diagnose_entry(gs_ctx *ctx, const gs_prover_job *job, gs_diagnose_constraint *constraints, uint32_t *nconstraints, gs_diagnose_assertion *assertions,
                   uint32_t assertions_cap, uint32_t *nassertions, char *err, uint64_t errcap) {
    if (!ctx || !job || !nconstraints || !nassertions) return GS_ERR_ARG;
    return guarded(err, errcap, GS_ERR_OOM, [&]() -> int {
        Ctx x{ctx};
        diagnose_impl(x, *job, constraints, nconstraints, assertions, assertions_cap, nassertions);
        return GS_OK;
    });
}

}  // namespace

extern "C" {

int gs_prover_diagnose_on(const gs_prover_binding *b, gs_ctx *ctx, const struct gs_prover_job *job, struct gs_diagnose_constraint *constraints,
                          uint32_t *nconstraints, struct gs_diagnose_assertion *assertions, uint32_t assertions_cap, uint32_t *nassertions, char *err,
                          uint64_t errcap) {
    if (!b) return GS_ERR_ARG;
    UseApi use(reinterpret_cast<const Api *>(b));
    return diagnose_entry(ctx, job, constraints, nconstraints, assertions, assertions_cap, nassertions, err, errcap);
}
int gs_prover_diagnose(gs_ctx *ctx, const struct gs_prover_job *job, struct gs_diagnose_constraint *constraints, uint32_t *nconstraints,
                       struct gs_diagnose_assertion *assertions, uint32_t assertions_cap, uint32_t *nassertions, char *err, uint64_t errcap) {
    if (!g_bound) return GS_ERR_UNSUPPORTED;
    UseApi use(&g_default_api);
    return diagnose_entry(ctx, job, constraints, nconstraints, assertions, assertions_cap, nassertions, err, errcap);
}

}  // extern "C"
