// air_jit.hip — AIR programs compiled instead of interpreted: the runtime.  Default (auto): a program runs compiled whenever its code
// object already exists (this process or the on-disk cache) and is built in the background otherwise; gs_air_jit(ctx, 1) /
// GSTARK_AIR_JIT=1 compile on first use, gs_air_jit(ctx, 0) / GSTARK_AIR_JIT=0 always interpret.
//
// The reference's air-assembly GENERATES code for an AIR's transition function and constraint evaluator when a module is
// instantiated ("generated JS over BigInt").  The register machine of air_vm.hip is the portable form of the same
// programs; air_codegen.h turns them into HIP source (plain C++, flavour by value); here that source is compiled once per program with
// hiprtc for gfx950 (jit_build.h: the sequence the helper process gstark_jitc shares), cached for the process and on disk, and launched.
// Same arithmetic (the field header the library itself is built from is embedded in the source), same values; any failure to
// compile falls back to the interpreter.  gs_air_jit_check generates + compiles without a device (CPU test tier).
#include <dlfcn.h>
#include <fcntl.h>
#include <spawn.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <thread>

#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>

#include "common.h"
#include "host_hash.h"
#include "air_codegen.h"
#include "jit_build.h"

static const char *kFieldHeader =
#if defined(GS_SMALL_Q)
#include "jit_gf_small.inc"
#elif defined(GS_WIDE_BITS)
#include "jit_gf_wide.inc"
#else
#include "jit_gf128.inc"
#endif
    ;
#ifdef GS_FIELD_128      // long exponentiations run in the five-limb lazy form (gf128_lazy.h: lz_sqr, lz_mul_v)
static const char *kLazyHeader =
#include "jit_gf128_lazy.inc"
    ;
#endif

#define GS_STR2(x) #x
#define GS_STR(x) GS_STR2(x)
// the headers a generated source is compiled against — what the compiler is given, the helper is sent and the cache key covers
static const JitHeaders &kHeaders = *new JitHeaders{
#ifdef GS_FIELD_128
    {"gf128.h", kFieldHeader}, {"gf128_lazy.h", kLazyHeader},
#else
    {"gs_field.h", kFieldHeader},
#endif
};
// the flavour this library is built for, as the generator wants it (air_codegen.h)
static const JitFlavour &kFlavour = *new JitFlavour{(uint32_t)sizeof(fe),
#ifdef GS_FIELD_128
    true,
#else
    false,
#endif
#if defined(GS_SMALL_Q)
    false, "#define GS_SMALL_Q " GS_STR(GS_SMALL_Q) "\n"
#elif defined(GS_WIDE_BITS)
    true, "#define GS_WIDE_BITS " GS_STR(GS_WIDE_BITS) "\n"
#else
    false, ""
#endif
};

struct JitKernel {
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
    bool failed = false;
    bool compiling = false;          // a background thread is building the code object (auto mode)
    std::vector<char> code;          // built (or read from the disk cache) but not loaded yet: the next launch loads it
};
// Process-wide state of the compiled programs.  Heap-allocated and never destroyed: a builder thread may still be running when the
// process reaches exit(), and function-/namespace-scope statics would be destroyed under it.  Background builds run in a helper
// process (jit_compile_helper); at exit / dlclose the threads waiting for one are released (their sockets shut down — the helper
// still finishes and fills the disk cache) and joined; a build running inside this process (no helper installed) is waited for.
static std::mutex &g_jit_mutex = *new std::mutex;
static std::map<std::string, JitKernel> &g_jit_cache = *new std::map<std::string, JitKernel>;   // per process: the lanes of a pool share the compiled programs
static std::vector<std::thread> &g_jit_builders = *new std::vector<std::thread>;                // guarded by g_jit_mutex
static std::vector<int> &g_jit_helper_fds = *new std::vector<int>;                              // sockets of the helpers being waited for; guarded by g_jit_mutex
static std::atomic<bool> g_jit_shutdown{false};
static std::atomic<int> g_jit_running{0};                   // builds inside this process that have not finished yet
static void jit_join_builders() {
    g_jit_shutdown.store(true);
    std::vector<std::thread> mine;
    {
        std::lock_guard<std::mutex> g(g_jit_mutex);
        mine.swap(g_jit_builders);
        for (int fd : g_jit_helper_fds) shutdown(fd, SHUT_RDWR);
    }
    // an in-process build takes a second to a minute and a half (the largest programs of the examples); its result still reaches the
    // disk cache.  Bounded: should a builder ever be stuck (a compiler that died under it), the process still ends — the thread is let go
    for (int waited = 0; g_jit_running.load() > 0 && waited < 200 * 100; waited++) usleep(10000);
    for (auto &t : mine) {
        if (!t.joinable()) continue;
        if (g_jit_running.load() > 0) t.detach(); else t.join();
    }
}
__attribute__((destructor)) static void jit_library_unload() { jit_join_builders(); }          // dlclose, or exit before the dependencies' finalisers

// hiprtc: source -> gfx950 code object (no device needed); false + log on failure
static bool jit_compile(const std::string &source, const char *entry, std::vector<char> &code, std::string &log) {
    const char *verbose = getenv("GSTARK_AIR_JIT_VERBOSE");
    if (verbose) fprintf(stderr, "[gstark] compiling an AIR program (%zu bytes of source, entry %s)\n", source.size(), entry);
    if (const char *dump = getenv("GSTARK_AIR_JIT_DUMP")) {          // keep the generated source (<dir>/<entry>_<n>.hip) for inspection
        static std::atomic<int> dumped{0};
        const std::string path = std::string(dump) + "/" + entry + "_" + std::to_string(dumped++) + ".hip";
        if (FILE *f = fopen(path.c_str(), "w")) { fputs(source.c_str(), f); fclose(f); }
    }
    const bool ok = jit_build(source, kHeaders, code, log);
    if (!ok && verbose) fprintf(stderr, "[gstark] hiprtc failed, interpreting instead:\n%s\n%.3000s\n", log.c_str(), verbose[0] == '2' ? source.c_str() : "");
    return ok;
}

// ---- background builds run in a helper process (jitc.cc explains why): <directory of this library>/gstark_jitc, or $GSTARK_JITC.
// 1 = built (code filled; the helper has written the cache file too), 0 = the compiler refused the source (log filled),
// -1 = no helper / could not be started (the caller compiles in-process, as gs_air_jit(ctx, 1) does)
extern char **environ;
static std::string jit_helper_path() {
    if (const char *e = getenv("GSTARK_JITC")) return e;
    Dl_info info;
    if (!dladdr((const void *)&jit_helper_path, &info) || !info.dli_fname) return "";
    std::string lib = info.dli_fname;
    const size_t slash = lib.rfind('/');
    return (slash == std::string::npos ? std::string(".") : lib.substr(0, slash)) + "/gstark_jitc";
}
static bool sock_send(int fd, const void *src, size_t n) {
    const char *p = (const char *)src;
    while (n) {
        const ssize_t r = send(fd, p, n, MSG_NOSIGNAL);
        if (r <= 0) return false;
        p += r;
        n -= (size_t)r;
    }
    return true;
}
static bool sock_recv(int fd, void *dst, size_t n) {
    char *p = (char *)dst;
    while (n) {
        const ssize_t r = recv(fd, p, n, 0);
        if (r <= 0) return false;
        p += r;
        n -= (size_t)r;
    }
    return true;
}
static int jit_compile_helper(const std::string &source, const char *entry, const std::string &cache_path, std::vector<char> &code, std::string &log) {
    const std::string helper = jit_helper_path();
    if (helper.empty() || access(helper.c_str(), X_OK) != 0) return -1;
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0, sv) != 0) return -1;
    {
        std::lock_guard<std::mutex> g(g_jit_mutex);
        if (g_jit_shutdown.load()) { close(sv[0]); close(sv[1]); return 0; }
        g_jit_helper_fds.push_back(sv[0]);
    }
    auto forget = [&] { std::lock_guard<std::mutex> g(g_jit_mutex); g_jit_helper_fds.erase(std::find(g_jit_helper_fds.begin(), g_jit_helper_fds.end(), sv[0])); close(sv[0]); };
    posix_spawn_file_actions_t fa;
    posix_spawn_file_actions_init(&fa);
    posix_spawn_file_actions_adddup2(&fa, sv[1], 0);                 // dup2 clears close-on-exec on the copies
    posix_spawn_file_actions_adddup2(&fa, sv[1], 1);
    if (!getenv("GSTARK_AIR_JIT_VERBOSE")) posix_spawn_file_actions_addopen(&fa, 2, "/dev/null", O_WRONLY, 0);
#if defined(__GLIBC__) && (__GLIBC__ > 2 || (__GLIBC__ == 2 && __GLIBC_MINOR__ >= 34))
    posix_spawn_file_actions_addclosefrom_np(&fa, 3);                // nothing else of the host (device nodes, sockets) reaches the helper
#endif
    char *const argv[] = {const_cast<char *>(helper.c_str()), nullptr};
    pid_t pid = 0;
    const int rc = posix_spawn(&pid, helper.c_str(), &fa, nullptr, argv, environ);
    posix_spawn_file_actions_destroy(&fa);
    close(sv[1]);
    if (rc != 0) { forget(); return -1; }
    if (getenv("GSTARK_AIR_JIT_VERBOSE")) fprintf(stderr, "[gstark] %s: built by %s (pid %d), %zu bytes of source\n", entry, helper.c_str(), (int)pid, source.size());
    const int fd = sv[0];
    JitHeaders items = {{entry, source.c_str()}};
    items.insert(items.end(), kHeaders.begin(), kHeaders.end());
    const uint32_t nitems = (uint32_t)items.size();
    bool ok = sock_send(fd, "GSJ1", 4) && sock_send(fd, &nitems, 4);
    for (size_t i = 0; ok && i < items.size(); i++) {
        const uint32_t nl = (uint32_t)items[i].first.size();
        const uint64_t dl = strlen(items[i].second);
        ok = sock_send(fd, &nl, 4) && sock_send(fd, items[i].first.data(), nl) && sock_send(fd, &dl, 8) && sock_send(fd, items[i].second, dl);
    }
    const uint32_t pl = (uint32_t)cache_path.size();
    ok = ok && sock_send(fd, &pl, 4) && sock_send(fd, cache_path.data(), pl);
    char tag[4];
    uint64_t len = 0;
    int result = -1;
    if (ok && sock_recv(fd, tag, 4) && sock_recv(fd, &len, 8) && len <= (256ull << 20)) {
        std::vector<char> body(len);
        if (sock_recv(fd, body.data(), len)) {
            if (memcmp(tag, "GSOK", 4) == 0 && len > 0) { code.swap(body); result = 1; }
            else if (memcmp(tag, "GSER", 4) == 0) { log.assign(body.begin(), body.end()); result = 0; }
        }
    }
    forget();
    int status = 0;
    (void)waitpid(pid, &status, g_jit_shutdown.load() ? WNOHANG : 0);          // reap; the verdict is what came over the socket
    if (result < 0 && g_jit_shutdown.load()) result = 0;            // released at exit: nothing to fall back to
    return result;
}

// ---- code objects on disk: <dir>/<sha256 of the generated source>.hsaco.  A compiled program outlives the process that built it, so
// "compile when an AIR is instantiated" costs its seconds once per machine, and the default mode (auto) can use compiled programs
// whenever they already exist without ever making a proof wait for the compiler.
// The directory is PRIVATE to the user: created 0700, and used only if it is a real directory (no symlink) owned by the effective
// user with no group / other write permission — a code object found there is loaded into the proving path, so nobody else may be
// able to plant one.  Without GSTARK_JIT_CACHE_DIR and without HOME (daemons, bare containers) there is no safe default: no cache.
// The files' own rules (no symlinks, same owner, a new file renamed into place) are jit_build.h's: jit_cache_read, jit_cache_write.
static bool jit_dir_is_private(const std::string &dir) {
    struct stat st;
    if (lstat(dir.c_str(), &st) != 0) return false;
    return S_ISDIR(st.st_mode) && st.st_uid == geteuid() && !(st.st_mode & (S_IWGRP | S_IWOTH));
}
static std::string jit_cache_path(const std::string &source, const char *entry) {
    const char *dir = getenv("GSTARK_JIT_CACHE_DIR");
    std::string base;
    if (dir && dir[0]) base = dir;
    else {
        const char *home = getenv("HOME");
        if (!home || !home[0]) return "";
        base = std::string(home) + "/.cache/gstark_jit";
    }
    if (base == "0" || base == "off") return "";
    while (base.size() > 1 && base.back() == '/') base.pop_back();
    std::string acc;
    for (size_t i = 1; i <= base.size(); i++)          // mkdir -p: parents with the usual mode, the cache directory itself private
        if (i == base.size() || base[i] == '/') { acc = base.substr(0, i); (void)mkdir(acc.c_str(), i == base.size() ? 0700 : 0755); }
    if (!jit_dir_is_private(base)) {
        static std::atomic<bool> warned{false};
        if (!warned.exchange(true) && getenv("GSTARK_AIR_JIT_VERBOSE"))
            fprintf(stderr, "[gstark] code-object cache %s is not a private directory of this user (owner, mode, symlink): not used\n", base.c_str());
        return "";
    }
    // the key covers everything the code object depends on: the generated source AND the field headers it is compiled against
    std::string keyed = std::string(entry) + "|gfx950|v2|";
    for (const auto &h : kHeaders) keyed += h.second;
    keyed += "|" + source;
    uint8_t d[32];
    host_sha256((const uint8_t *)keyed.data(), keyed.size(), d);
    char hex[65];
    for (int i = 0; i < 32; i++) snprintf(hex + 2 * i, 3, "%02x", d[i]);
    return base + "/" + hex + ".hsaco";
}
static bool jit_load(JitKernel &k, const char *entry) {
    if (hipModuleLoadData(&k.module, k.code.data()) != hipSuccess) return false;
    if (hipModuleGetFunction(&k.fn, k.module, entry) != hipSuccess) return false;
    std::vector<char>().swap(k.code);
    return true;
}

// mode 1 (gs_air_jit(ctx, 1)): the kernel, compiling it now if nobody has yet.  mode 2 (auto, the default): the kernel if this process
// or the disk cache already holds it; otherwise null — the caller interprets this time — and ONE background thread builds it for the
// launches (and processes) to come.
static JitKernel *jit_get(gs_ctx *c, const std::string &source, const char *entry) {
    std::unique_lock<std::mutex> lock(g_jit_mutex);
    auto it = g_jit_cache.find(source);
    if (it != g_jit_cache.end()) {
        JitKernel &k = it->second;
        if (k.fn) return &k;
        if (k.failed) return nullptr;
        if (!k.code.empty()) { if (jit_load(k, entry)) return &k; k.failed = true; return nullptr; }
        if (k.compiling && c->air_jit != 1) return nullptr;           // still being built in the background: interpret
        if (k.compiling) {                                            // mode on: wait for the builder instead of compiling twice
            while (k.compiling) { lock.unlock(); usleep(2000); lock.lock(); }
            if (k.failed || k.code.empty()) return nullptr;
            if (jit_load(k, entry)) return &k;
            k.failed = true;
            return nullptr;
        }
    }
    JitKernel &k = g_jit_cache[source];
    const std::string path = jit_cache_path(source, entry);
    if (jit_cache_read(path, k.code)) {
        if (jit_load(k, entry)) return &k;
        k.failed = false;                                             // a stale / truncated file: fall through and rebuild
        std::vector<char>().swap(k.code);
    }
    if (c->air_jit == 1) {
        k.failed = true;
        std::string log;
        if (!jit_compile(source, entry, k.code, log)) { gs_fail(c, GS_ERR_DEVICE, "air jit: %.400s", log.c_str()); return nullptr; }
        jit_cache_write(path, k.code);
        if (!jit_load(k, entry)) return nullptr;
        k.failed = false;
        return &k;
    }
    if (g_jit_shutdown.load()) return nullptr;                        // the process is on its way out: interpret, start nothing
    k.compiling = true;
    // Background builds run in the helper process: a host that exits meanwhile leaves nothing of the compiler inside THIS process to be
    // torn down under a running thread.  Only without the helper (not installed next to the library) does the builder compile here, and
    // then exit waits for it (jit_join_builders, bounded).
    static std::once_flag at_exit_once;
    std::call_once(at_exit_once, [] { atexit(jit_join_builders); });
    g_jit_builders.emplace_back([source, path, entry]() {
        std::vector<char> code;
        std::string log;
        int built = g_jit_shutdown.load() ? 0 : jit_compile_helper(source, entry, path, code, log);
        if (built < 0) {
            static std::atomic<bool> told{false};
            if (!told.exchange(true)) fprintf(stderr, "[gstark] gstark_jitc not found next to the library (%s): AIR programs are compiled inside this process\n", jit_helper_path().c_str());
            g_jit_running.fetch_add(1);
            struct Done { ~Done() { g_jit_running.fetch_sub(1); } } done;
            static std::mutex &one_at_a_time = *new std::mutex;   // hiprtc builds one program at a time (two concurrent builds: the second came back empty)
            std::lock_guard<std::mutex> b(one_at_a_time);
            built = !g_jit_shutdown.load() && jit_compile(source, entry, code, log) ? 1 : 0;          // queued behind another build at exit: skip
            if (built == 1) jit_cache_write(path, code);
        }
        if (built != 1 && getenv("GSTARK_AIR_JIT_VERBOSE")) fprintf(stderr, "[gstark] background build of %s failed: %.600s\n", entry, log.c_str());
        std::lock_guard<std::mutex> g(g_jit_mutex);
        JitKernel &kk = g_jit_cache[source];
        if (built == 1) kk.code.swap(code); else kk.failed = true;
        kk.compiling = false;
    });
    return nullptr;
}

// ---- generated sources, remembered.  Turning a program into source (SSA, scheduling, ~10 KB of text) costs ~0.1 ms of host time — per
// proof, if done per call, and a Poseidon proof is 1.5 ms.  The inputs of the generator — program(s), constants, static layout and,
// for trace programs, which static registers are 0/1 selectors — are concatenated into a key (a ~10 KB memcpy + one map lookup);
// the source (itself the key of the code-object cache) and the lane count are generated once per key and process.
struct JitSource { std::string source; uint32_t lanes = 1; bool ok = false; };
static std::mutex &g_src_mutex = *new std::mutex;
static std::map<std::string, std::shared_ptr<JitSource>> &g_src_memo = *new std::map<std::string, std::shared_ptr<JitSource>>;
template <class Make>
static std::shared_ptr<const JitSource> jit_source_memo(const std::string &key, Make make) {
    std::lock_guard<std::mutex> g(g_src_mutex);
    auto it = g_src_memo.find(key);
    if (it == g_src_memo.end()) {
        if (g_src_memo.size() > 256) g_src_memo.clear();          // a host cycling through hundreds of AIRs: start over rather than grow (callers hold their entry)
        it = g_src_memo.emplace(key, std::make_shared<JitSource>()).first;
        make(*it->second);
    }
    return it->second;
}

// ---- trace segments --------------------------------------------------------------------------------------------------------------
// returns GS_OK when the compiled kernel was launched, GS_ERR_UNSUPPORTED when the caller should interpret instead
int gs_jit_trace_segments(gs_ctx *c, const AirProgram &p, const AirProgram &init, const uint8_t *statics_host, const fe *dconst, const fe *dstat,
                          const fe *drows, uint64_t segments, uint64_t seglen, fe *out) {
    JitGen gen{kFlavour, 1, statics_host};
    std::string key = jit_key(kFlavour, "T", p, &init);
    for (uint32_t r = 0; r < p.nstatic; r++) key.push_back(gen.static_is_binary(p, r) ? '1' : '0');
    const std::shared_ptr<const JitSource> src = jit_source_memo(key, [&](JitSource &js) {
        js.ok = jit_trace_source(js.source, gen, p, init);
        js.lanes = gen.lanes;
    });
    if (!src->ok) return GS_ERR_UNSUPPORTED;
    gen.lanes = src->lanes;
    const std::string &s = src->source;
    JitKernel *k = jit_get(c, s, "gs_jit_trace");
    if (!k) return GS_ERR_UNSUPPORTED;
    unsigned long long a_segments = segments, a_seglen = seglen;
    void *args[] = {(void *)&dconst, (void *)&dstat, (void *)&drows, (void *)&a_segments, (void *)&a_seglen, (void *)&out};
    constexpr unsigned block = 64;
    static_assert(block == 64, "gs_jit_trace: gs_swap[64], __launch_bounds__(64) and the lane groups assume one wave64 per block");
    const unsigned grid = (unsigned)((segments * gen.lanes + block - 1) / block);
    gs_traffic(c, (uint64_t)p.registers * segments * (seglen + 1) * GS_ELT, (uint64_t)p.registers * segments * seglen, "gs_jit_trace");      // first rows in, the trace out
    if (hipModuleLaunchKernel(k->fn, grid, 1, 1, block, 1, 1, 0, c->stream, args, nullptr) != hipSuccess) return GS_ERR_UNSUPPORTED;
    c->jit_launches++;
    return GS_OK;
}

// ---- constraints -----------------------------------------------------------------------------------------------------------------
int gs_jit_constraints(gs_ctx *c, const AirProgram &p, const fe *dconst, const fe *columns, uint64_t nc, uint64_t shift, const fe *statics, fe *out,
                       uint64_t prow, uint64_t pstride) {
    const std::shared_ptr<const JitSource> src = jit_source_memo(jit_key(kFlavour, "C", p, nullptr), [&](JitSource &js) { js.ok = jit_constraints_source(js.source, kFlavour, p); });
    if (!src->ok) return GS_ERR_UNSUPPORTED;
    const std::string &s = src->source;
    JitKernel *k = jit_get(c, s, "gs_jit_constraints");
    if (!k) return GS_ERR_UNSUPPORTED;
    unsigned long long a_nc = nc, a_shift = shift, a_prow = prow, a_pstride = pstride;
    void *args[] = {(void *)&dconst, (void *)&columns, (void *)&a_nc, (void *)&a_shift, (void *)&statics, (void *)&out, (void *)&a_prow, (void *)&a_pstride};
    const unsigned block = 128, grid = gs_grid(nc, block, 256 * 16);
    {   // every register read at nc points (the neighbour row is the same vector), one vector per constraint written
        uint64_t outs = 0;
        for (uint32_t pc = 0; pc < p.ninstr; pc++) outs += p.at(pc).op == OP_OUT;
        gs_traffic(c, nc * ((uint64_t)p.registers + outs) * GS_ELT, nc * outs, "gs_jit_constraints");
    }
    if (hipModuleLaunchKernel(k->fn, grid, 1, 1, block, 1, 1, 0, c->stream, args, nullptr) != hipSuccess) return GS_ERR_UNSUPPORTED;
    c->jit_launches++;
    return GS_OK;
}

// Compile-only check (no device, no context): does the generated source for this program build for gfx950?  kind 0: trace segments
// (code + optional init program), kind 1: constraints.  The "does it build" tier of the tests runs it on machines without a GPU.
// Test hook (not part of include/gstark.h): where the code object of `source` would be cached under the current environment — the
// empty string when the cache is disabled or the directory is not private to this user.  Creates the directory like a real build.
// test hook: one program through the helper process, synchronously.  Returns jit_compile_helper's verdict; *size = bytes of code object
// (or of the compiler's log), the first min(cap, *size) of which are copied to out
extern "C" int gs_jit_helper_probe(const char *source, const char *entry, const char *cache_path, char *out, uint64_t cap, uint64_t *size) {
    std::vector<char> code;
    std::string log;
    const int r = jit_compile_helper(source, entry, cache_path ? cache_path : "", code, log);
    const char *src = r == 1 ? code.data() : log.data();
    const uint64_t n = r == 1 ? code.size() : log.size();
    if (size) *size = n;
    if (out && cap) memcpy(out, src, n < cap ? n : cap);
    return r;
}
extern "C" int gs_jit_cache_path_probe(const char *source, char *out, uint64_t cap) {
    if (!source || !out || !cap) return GS_ERR_ARG;
    const std::string path = jit_cache_path(source, "gs_jit_probe");
    snprintf(out, (size_t)cap, "%s", path.c_str());
    return GS_OK;
}

// gs_air_jit_check with the tables of the static registers (trace programs: products by 0/1 selectors become selects, so the source
// a prover compiles depends on them); not part of the ABI — a hook of this library for AirObject.compileCheck and the CPU test tier
extern "C" int gs_air_jit_check_statics(int kind, const uint32_t *code, uint32_t ninstr, const uint32_t *init_code, uint32_t init_ninstr,
                                        const uint8_t *consts_host, uint32_t nconsts, uint32_t vm_regs, uint32_t registers, const uint64_t *static_lens,
                                        uint32_t nstatic, const uint8_t *static_values_host, char *log_out, uint64_t log_cap) {
    if (!code || !ninstr || nstatic > GS_AIR_MAX_REGISTERS || (nstatic && !static_lens) || (nconsts && !consts_host)) return GS_ERR_ARG;
    // (an evaluator's number of constraints is no argument of this hook: its OUT destinations are not bounded here)
    AirProgram p {code, ninstr, consts_host, nconsts, vm_regs, registers, nstatic, kind == 0 ? registers : UINT32_MAX};
    if (!air_static_layout(static_lens, nstatic, p.sd)) return GS_ERR_ARG;
    const AirProgram init = p.with_code(init_code, kind == 0 ? init_ninstr : 0);
    char msg[96];
    if (!air_validate(p, kind != 0, true, msg, sizeof msg) || (init.ninstr && !air_validate(init, false, false, msg, sizeof msg))) {
        if (log_out && log_cap) snprintf(log_out, log_cap, "%s", msg);
        return GS_ERR_UNSUPPORTED;
    }
    JitGen gen{kFlavour, 1, kind == 0 ? static_values_host : nullptr};
    std::string src, log;
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = kind == 0 ? jit_trace_source(src, gen, p, init) : jit_constraints_source(src, kFlavour, p);
    if (getenv("GSTARK_AIR_JIT_VERBOSE"))
        fprintf(stderr, "[gstark] source of the %s program generated in %.1f us (%zu bytes)\n", kind == 0 ? "trace" : "constraint",
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), src.size());
    std::vector<char> obj;
    const bool built = ok && jit_compile(src, kind == 0 ? "gs_jit_trace" : "gs_jit_constraints", obj, log);
    if (log_out && log_cap) snprintf(log_out, log_cap, "%s", !ok ? "the program has an instruction the generator does not know" : log.c_str());
    return built ? GS_OK : GS_ERR_UNSUPPORTED;
}
extern "C" int gs_air_jit_check(int kind, const uint32_t *code, uint32_t ninstr, const uint32_t *init_code, uint32_t init_ninstr,
                                const uint8_t *consts_host, uint32_t nconsts, uint32_t vm_regs, uint32_t registers, const uint64_t *static_lens,
                                uint32_t nstatic, char *log_out, uint64_t log_cap) {
    return gs_air_jit_check_statics(kind, code, ninstr, init_code, init_ninstr, consts_host, nconsts, vm_regs, registers, static_lens, nstatic, nullptr, log_out, log_cap);
}
