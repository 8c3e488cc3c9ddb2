/* gstark_debug.h — a test hook on the context's device block cache (csrc/ctx.hip).  Never needed in production.
 *
 * gs_alloc keeps freed blocks, keyed by their rounded size, and hands one straight back to the next request of that size with whatever
 * its last user left in it; every entry's temporaries and every binding's output vectors come from there.  A long-lived process
 * therefore runs every call on recycled memory, while a test that calls a shape once runs on blocks fresh from the driver.  This
 * entry lets a test put the cache into the worst recycled state on purpose: every cached block holds one byte value throughout.
 *
 * The entry point is OPTIONAL on an implementation of the ABI (include/gstark.h lists the mandatory ones): the HIP library exports
 * it; a binding that does not find it says so. */
#ifndef GSTARK_DEBUG_H
#define GSTARK_DEBUG_H

#include "gstark.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fills every block the cache holds (freed, not yet handed out again) with `byte`, on the context's stream, in order behind everything
 * enqueued so far; does not synchronise.  Blocks that are allocated and the context's own persistent buffers are not touched.
 * *blocks / *bytes (either may be NULL) = how many blocks and how many bytes were filled.  GS_ERR_ARG for a NULL context. */
int gs_cache_fill(gs_ctx *ctx, uint8_t byte, uint64_t *blocks, uint64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif
