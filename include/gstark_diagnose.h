/* gstark_diagnose.h — why a statement does not prove: which assertion, which constraint at which step, which declared degree.
 *
 * prove() ends a statement that cannot be proved with one sentence ("Low degree proof failed: Remainder is not a valid degree 47
 * polynomial", csrc/prover.cc: check_remainder) whatever the cause: a witness that breaks one constraint, an evaluator that drifted from
 * its transition, or a declared degree the reference's degree rule (lib/components/CompositionPolynomial.ts:37-43,88-99,196-204) does not
 * let through.  gs_prover_diagnose takes the same job, writes no proof and says which it is.
 *
 * gs_nonzero_spans is the one device routine it adds: per row of a matrix, how many elements are non-zero and where the first and the
 * last of them lie.  It is OPTIONAL on an implementation of the ABI (include/gstark.h lists the mandatory ones), like the entries of
 * gstark_boundary.h: the HIP library exports it (csrc/diagnose.hip); a driver bound to a library without it downloads the matrix and
 * scans it on the host. */
#ifndef GSTARK_DIAGNOSE_H
#define GSTARK_DIAGNOSE_H

#include "gstark_prover.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per row r < rows of m (device: rows x row_stride elements, canonical, so an element is zero exactly when all its bytes are), over the
 * columns [0, n): count_host[r] = how many elements are non-zero, first_host[r] / last_host[r] = the column of the first / the last of
 * them; first = last = n when the row is all zero.  Columns [n, row_stride) are not read.  rows == 0, n == 0, n > row_stride and null
 * pointers are refused with a message.  The call returns with the three host arrays (rows entries each) filled. */
int gs_nonzero_spans(gs_ctx *ctx, const void *m, uint64_t rows, uint64_t row_stride, uint64_t n, uint64_t *count_host, uint64_t *first_host,
                     uint64_t *last_host);

/* ---- the driver's entry (csrc/diagnose.h, part of libgstark_prover*.so) ---- */

/* One record per constraint of a kind-1 AIR (register-machine programs).  Values are elements of gs_element_size() bytes, little-endian,
 * in fields of GS_PROVER_ELT_MAX bytes, like the job's scalars. */
struct gs_diagnose_constraint {
    /* on the trace: the constraint at the steps [0, steps - 1) — the last step is exempt (lib/components/ZeroPolynomial.ts:36-44) */
    uint64_t violations;                         /* steps at which it does not evaluate to zero */
    uint64_t first_step, last_step;              /* of those; both = steps - 1 when there is none */
    uint8_t first_value[GS_PROVER_ELT_MAX];      /* what it evaluates to at first_step (zero when there is none) */
    /* as a polynomial: the constraint over the trace polynomials, interpolated over 2 * composition_factor * steps points */
    uint64_t degree;                             /* measured; 0 with all_zero = 1 */
    uint64_t limit;                              /* the highest degree its declared degree lets through */
    uint32_t declared;                           /* the job's degrees[i] */
    uint32_t needed;                             /* ceil((degree + 2) / steps): the smallest declaration the measured degree fits */
    uint32_t at_least;                           /* 1: a constraint of true degree above 2 * composition_factor folds onto the domain it
                                                    was measured on, so degree and needed are lower bounds */
    uint32_t all_zero;                           /* 1: the polynomial is identically zero */
};
/* An assertion whose cell of the trace holds another value. */
struct gs_diagnose_assertion {
    uint32_t index;                              /* in job.assertions */
    uint32_t reserved;
    uint8_t found[GS_PROVER_ELT_MAX];            /* what the trace holds there */
};

/* The job is prove()'s; hash_alg and the query counts are not read, nothing is committed and no proof is written.  Validation and its
 * messages are prove()'s.  constraints: job.air.nconstraints records (kind 1; kind 0, MiMC, fills none and sets *nconstraints = 0: its
 * transition and its constraint are both the library's).  assertions: room for assertions_cap records; *nassertions receives how many
 * assertions conflict with the trace, EVERY one of them (the first assertions_cap are written).  GS_OK = the diagnosis was made, whatever
 * it says.  A failure leaves the context usable. */
int gs_prover_diagnose(gs_ctx *ctx, const struct gs_prover_job *job, struct gs_diagnose_constraint *constraints, uint32_t *nconstraints,
                       struct gs_diagnose_assertion *assertions, uint32_t assertions_cap, uint32_t *nassertions, char *err, uint64_t errcap);
int gs_prover_diagnose_on(const gs_prover_binding *b, gs_ctx *ctx, const struct gs_prover_job *job, struct gs_diagnose_constraint *constraints,
                          uint32_t *nconstraints, struct gs_diagnose_assertion *assertions, uint32_t assertions_cap, uint32_t *nassertions, char *err,
                          uint64_t errcap);

#ifdef __cplusplus
}
#endif
#endif
