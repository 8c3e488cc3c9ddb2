// gstark_jitc — the compiler of AIR programs as a process of its own (air_jit.hip: background builds of the default "auto" mode).
//
// A background build inside the proving process means a thread inside hiprtc / comgr (LLVM) for seconds.  If the host reaches exit()
// meanwhile, the C++ runtime destroys that compiler's statics under the thread: seen on the GPU box as "LLVM ERROR ..." + abort at
// exit, and once as a process that never ended.  No ordering of atexit handlers closes that race (the compiler registers finalisers
// whenever one of its lazily built objects first appears).  So the proving process never runs a background compilation itself: it
// hands the generated source to this helper over a socket and waits for the code object; when the host exits first the helper's
// reply has nowhere to go and the helper ends — after having written the code object to the cache, so the work is not lost.
//
// stdin = stdout = one end of a socketpair.
//   request  "GSJ1" u32 nitems { u32 name_len, name, u64 len, bytes }*  u32 path_len, cache path ("" = none)
//            item 0: name = kernel entry point, bytes = generated source; items 1..: the field headers the source includes
//   reply    "GSOK" u64 len, code object   |   "GSER" u64 len, compiler log
// The compilation itself and the cache file's rules are jit_build.h's, shared with the in-process builds of air_jit.hip.
// Needs no GPU (hiprtc cross-compiles for gfx950).
#include <stdint.h>
#include <string.h>
#include <sys/socket.h>

#include "jit_build.h"

static bool read_all(void *dst, size_t n) {
    char *p = (char *)dst;
    while (n) {
        const ssize_t r = read(0, p, n);
        if (r <= 0) return false;
        p += r;
        n -= (size_t)r;
    }
    return true;
}
static bool write_all(const void *src, size_t n) {
    const char *p = (const char *)src;
    while (n) {
        ssize_t r = send(1, p, n, MSG_NOSIGNAL);
        if (r < 0) r = write(1, p, n);          // stdout is not a socket (run by hand): plain write
        if (r <= 0) return false;
        p += r;
        n -= (size_t)r;
    }
    return true;
}
static void reply(const char *tag, const void *data, uint64_t len) {
    write_all(tag, 4);
    write_all(&len, 8);
    write_all(data, len);
}

int main() {
    char magic[4];
    uint32_t nitems = 0;
    if (!read_all(magic, 4) || memcmp(magic, "GSJ1", 4) != 0 || !read_all(&nitems, 4) || nitems < 1 || nitems > 8) return 2;
    std::vector<std::string> names(nitems), bodies(nitems);
    for (uint32_t i = 0; i < nitems; i++) {
        uint32_t nl = 0;
        uint64_t dl = 0;
        if (!read_all(&nl, 4) || nl > 256) return 2;
        names[i].resize(nl);
        if (!read_all(&names[i][0], nl) || !read_all(&dl, 8) || dl > (64ull << 20)) return 2;
        bodies[i].resize(dl);
        if (!read_all(&bodies[i][0], dl)) return 2;
    }
    uint32_t pl = 0;
    if (!read_all(&pl, 4) || pl > 4096) return 2;
    std::string path(pl, 0);
    if (pl && !read_all(&path[0], pl)) return 2;

    JitHeaders headers;
    for (uint32_t i = 1; i < nitems; i++) headers.push_back({names[i], bodies[i].c_str()});
    std::vector<char> code;
    std::string log;
    if (!jit_build(bodies[0], headers, code, log)) {
        reply("GSER", log.data(), log.size());
        return 1;
    }
    jit_cache_write(path, code);                // first: the host may be gone by now, the next process still finds the program
    reply("GSOK", code.data(), code.size());
    return 0;
}
