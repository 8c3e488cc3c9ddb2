/* gstark_hades.h — Hades permutations (Poseidon hashes) and Poseidon Merkle trees on the device (csrc/hades.hip;
 * gs_hades_merkle_paths, which hashes nothing, is in csrc/field_tree.hip).
 *
 * The permutation is the one of the reference's examples/poseidon/utils.ts:19-49 (createHash): the state is the inputs followed by zeros
 * up to `width`; round i < full_rounds + partial_rounds adds round constant row i, raises to `alpha` (every element in a full round:
 * i < full_rounds / 2 or i >= full_rounds / 2 + partial_rounds; only element width - 1 otherwise) and replaces the state by mds * state
 * (new[i] = sum_j mds[i][j] * state[j]).  The digest is the first `digest` elements of the last state.  Every result is an exact field
 * element: what host integers give.
 *
 * The tree is the reference's MerkleTree / MerkleTree2 (utils.ts:126-210) in its heap layout: 2n x digest elements, the leaves at nodes
 * n .. 2n - 1, node i = the digest of the permutation of node 2i followed by node 2i + 1, the root at 1, node 0 zero.
 *
 * These entry points are OPTIONAL on an implementation of the ABI (include/gstark.h lists the mandatory ones), like those of
 * gstark_boundary.h: the HIP library exports them; a binding that does not find them computes on host integers (genstark_amd/hades.py)
 * or says so (js/hades.js).  Everything is enqueued on the context's stream; nothing is read back. */
#ifndef GSTARK_HADES_H
#define GSTARK_HADES_H

#include "gstark.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gs_hades gs_hades;

/* One parameter set, its constants uploaded once: 2 <= width <= 8, full_rounds even and >= 2, alpha >= 2;
 * round_constants_host: (full_rounds + partial_rounds) x width elements, round-major; mds_host: width x width elements, row-major
 * (gs_element_size() bytes each, canonical).  The handle belongs to the context that made it. */
int gs_hades_create(gs_ctx *ctx, uint32_t width, uint32_t full_rounds, uint32_t partial_rounds, uint64_t alpha, const uint8_t *round_constants_host,
                    const uint8_t *mds_host, gs_hades **out);
int gs_hades_destroy(gs_ctx *ctx, gs_hades *h);

/* `count` permutations, one thread each: in (device) holds count x arity elements, row k the inputs of permutation k
 * (1 <= arity < width); out (device) receives count x digest elements (digest 1 or 2). */
int gs_hades_hash(gs_ctx *ctx, const gs_hades *h, const void *in, uint64_t count, uint32_t arity, uint32_t digest, void *out);

/* The tree over n leaves of `digest` elements (n a power of two >= 2, 2 * digest < width): nodes_out (device) receives 2n x digest
 * elements in the heap layout above.  leaves may be nodes_out + n * digest elements (the leaves already in place).  A level of more than
 * gs_hades_merkle_top() nodes is one launch; all levels of at most that many nodes are ONE launch of one workgroup. */
int gs_hades_merkle(gs_ctx *ctx, const gs_hades *h, const void *leaves, uint64_t n, uint32_t digest, void *nodes_out);
uint32_t gs_hades_merkle_top(void);

/* The authentication paths of `count` leaves (indexes_host[k] < n; repeats allowed) out of a tree in the heap layout above: out (device)
 * receives count x (log2 n + 1) x digest elements, per path the leaf and its log2 n siblings bottom-up — the order of
 * MerkleTree.prove(index) — so that one read-back serves any number of paths.  The gather is family-neutral: it reads nothing but the
 * node array and hashes nothing, so it serves the trees of gs_hades_merkle and of gs_rescue_merkle (gstark_rescue.h, digest = 1) alike;
 * the name is the one it was first exported with. */
int gs_hades_merkle_paths(gs_ctx *ctx, const void *nodes, uint64_t n, uint32_t digest, const uint64_t *indexes_host, uint64_t count, void *out);

#ifdef __cplusplus
}
#endif
#endif
