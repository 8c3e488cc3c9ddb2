/* gstark_mimc.h — gs_mimc_composition (include/gstark.h) with its per-point factors taken from tables (csrc/air_mimc.hip).
 *
 * Of the ten field products gs_mimc_composition spends on a point, three depend on neither the trace nor the coefficients drawn from
 * the evaluation root: the domain point x = omega^i, the interpolant I(x), and one of the divisions by (x - x_a).  A prover knows them
 * before it has a trace, and its device is idle while a host core runs the MiMC recurrence.  So, over the n points of the domain:
 *     X[i]  = omega^i - x_last                              x_last = omega^((steps - 1) * n/steps)
 *     U[i]  = prod_{a < nroots} u[(i - root_index[a]) mod n]      u[j] = 1 / (omega^j - 1), u[0] = 0: U = 0 at the asserted points
 *     IU[i] = I(omega^i) * U[i]
 * and the pass becomes (qz, bt, lt: the n/steps-entry tables of gs_mimc_composition; bt carries prod_a omega^-root_index[a])
 *     out[i] = qz * (Q * X[i]) + bt * (p[i] * U[i] - IU[i]) [+ lt * p[i]]
 * seven products, the same field element: every output byte is gs_mimc_composition's.
 *
 * The tables belong to the context: 3 * n elements of device memory, one statement shape at a time.  X is kept from call to call for
 * the same (omega, n, steps), U for the same root indices on top; IU depends on the asserted values and is rebuilt by every prepare.
 *
 * These entry points are OPTIONAL on an implementation of the ABI (include/gstark.h lists the mandatory ones): the HIP library
 * exports them, a binding that does not find them calls gs_mimc_composition. */
#ifndef GSTARK_MIMC_H
#define GSTARK_MIMC_H

#include "gstark.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Builds (or finds) the tables of one statement; arguments as in gs_mimc_composition.  Everything is enqueued on the context's stream,
 * nothing is read back: call it before the trace is generated.  GS_OK also when no tables were made — n above the limit below, or no
 * device memory for them: gs_mimc_composition_tables then runs gs_mimc_composition. */
int gs_mimc_composition_prepare(gs_ctx *ctx, uint64_t n, uint64_t steps, const gs_elt *omega, const uint64_t *root_index_host, uint32_t nroots,
                                const uint8_t *ipoly_host);

/* gs_mimc_composition, same arguments, same output: from the context's tables when the last gs_mimc_composition_prepare made them for
 * exactly this (n, steps, omega, root indices, interpolant), by gs_mimc_composition itself otherwise. */
int gs_mimc_composition_tables(gs_ctx *ctx, const void *p_eval, uint64_t n, uint64_t steps, const gs_elt *omega, const void *k_table,
                               uint64_t klen, const uint8_t *coeffs_host, uint64_t q_inc, uint64_t b_inc, const uint8_t *ipoly_host,
                               const uint64_t *root_index_host, uint32_t nroots, const uint8_t *lc_coeffs_host, void *out);

/* Process-wide: domains of more than max_n points get no tables (0: the default, 2^26 — 3 GiB of tables per context there; larger
 * values are clamped to it).  Returns the previous value.  Tests force the table-free pass at small sizes with it. */
uint64_t gs_mimc_composition_tables_max_n(uint64_t max_n);

#ifdef __cplusplus
}
#endif

#endif
