// field_tree.h — what the algebraic hash units (hades.hip, rescue.hip) ask of field_tree.hip, the unit of everything that reads and
// writes tree nodes and knows no permutation: the path gather, batches of leaf updates on a heap-layout tree with every update's
// witness (include/gstark_tree_update.h) and sparse trees of fixed depth (include/gstark_sparse_tree.h).  A unit brings "hash these
// rows" as a tree_node_hash: its own launch, so a node computed there is bit for bit the node its tree build computes.
//   plans     tree_update_plan.h and sparse_tree_plan.h, on the host: per (level, update) whose version of the sibling node the update
//             sees, and for a sparse tree the slot of every stored node.
//   versions  ver[l][j] = the value of node (n + indexes[j]) >> l just after update j.  ver[0] is the new leaves (the caller's array),
//             ver[depth] the roots (the caller's array), the levels between lie level-major in one scratch block: a level's hash
//             launch writes one contiguous run.
//   a level   the gather writes, per update, its version and its sibling's value side by side in left/right order (a row of
//             2 * digest elements) and the sibling into the witness; the unit's launch hashes the rows into ver[l + 1].  No update
//             waits for another: a level is `count` independent permutations.
//   commit    NO level writes the nodes: an update further on may still have to read what a node held at the call (its predecessor
//             is -1).  After the last level every node's latest toucher stores its version; one writer per node.
//   sparse    the nodes are slots of a store on the device (slots x digest elements, append-only: a node keeps its slot for life; it
//             grows by doubling with ONE device copy, never past GS_SPARSE_MAX_SLOTS = 2^31) or, where the plan found no slot,
//             empties[level]: (depth + 1) x digest elements, empties[0] the empty leaf, empties[l + 1] = node(empties[l], empties[l]).
//             The index changes only after every launch of a batch has been enqueued without error; before the upload every slot is
//             checked against the slots the store holds (O(count x depth)): a bad slot is an error code, never an access.
// Everything is enqueued on the context's stream; the scratch is stream-ordered (gs_tmp_alloc); nothing is read back.
#pragma once
#include "sparse_tree_plan.h"
#include "sponge_common.h"
#include "tree_update_plan.h"

// run(c, handle, digest, rows, count, out): `count` rows of 2 * digest elements at `rows` into `count` nodes of `digest` elements at
// `out`, enqueued on the context's stream, with the launch's traffic line.  handle: the unit's parameter set.
struct tree_node_hash {
    int (*run)(gs_ctx *c, const void *handle, uint32_t digest, const fe *rows, uint64_t count, fe *out);
    const void *handle;
};

struct gs_sparse {
    gs_ctx *ctx;
    uint32_t depth, digest;
    tree_node_hash hash;                     // the unit's launch and its hash handle, which outlives the tree: only `run` dereferences it
    uint64_t hash_serial;                    // the serial that handle was created under (sponge_common.h)
    fe *store;
    uint64_t capacity;                       // slots the store holds
    fe *empties;
    sparse_tree_index index;
};

// the arguments every unit's update entry shares (the unit has checked its handle and that `digest` fits its state)
int tree_update_check(gs_ctx *c, const char *who, uint64_t n, uint64_t count, const uint64_t *indexes_host, const void *nodes, const void *leaves, const void *before,
                      const void *roots);
// the batch on the 2n nodes at `nodes`.  count >= 1 and the arguments have passed tree_update_check.
int tree_update_run(gs_ctx *c, fe *nodes, uint64_t n, uint32_t digest, const uint64_t *indexes_host, const fe *leaves, uint64_t count, fe *before, fe *roots,
                    const tree_node_hash &hash);
// empty_host: `digest` canonical elements, or null for zeros.  The unit has checked hash.handle (a live one) and that two nodes of
// `digest` elements fit its state.
int sparse_tree_create(gs_ctx *c, const char *who, const tree_node_hash &hash, uint32_t depth, uint32_t digest, const void *empty_host, uint64_t slots_hint, gs_sparse **out);
