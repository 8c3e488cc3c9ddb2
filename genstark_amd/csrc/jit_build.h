// jit_build.h — what the two builders of compiled AIR programs both know: air_jit.hip (builds inside the proving process) and jitc.cc
// (gstark_jitc, the helper process background builds run in).  The one hiprtc sequence with its options, and the rules of a code
// object's file in the on-disk cache.  Plain C++ plus hiprtc.h: g++ and hipcc both compile it; needs no GPU (hiprtc cross-compiles).
#pragma once
#include <hip/hiprtc.h>
#include <fcntl.h>
#include <stdio.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <utility>
#include <vector>

typedef std::vector<std::pair<std::string, const char *>> JitHeaders;       // (name the source includes it by, text)

// source -> gfx950 code object; false + the compiler's log on failure
inline bool jit_build(const std::string &source, const JitHeaders &headers, std::vector<char> &code, std::string &log) {
    std::vector<const char *> names, texts;
    for (const auto &h : headers) { names.push_back(h.first.c_str()); texts.push_back(h.second); }
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, source.c_str(), "gs_air_jit.hip", (int)headers.size(), texts.data(), names.data()) != HIPRTC_SUCCESS) {
        log = "hiprtcCreateProgram failed";
        return false;
    }
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
    const bool ok = hiprtcCompileProgram(prog, 3, opts) == HIPRTC_SUCCESS;
    size_t n = 0;
    if (ok) {
        hiprtcGetCodeSize(prog, &n);
        code.resize(n);
        hiprtcGetCode(prog, code.data());
    } else {
        hiprtcGetProgramLogSize(prog, &n);
        log.assign(n, 0);
        if (n) hiprtcGetProgramLog(prog, &log[0]);
    }
    hiprtcDestroyProgram(&prog);
    return ok;
}

// A code object found in the cache is loaded into the proving path, so nobody else may be able to plant one: files are opened without
// following symlinks and must be regular files of the effective user that group and others cannot write.
inline bool jit_cache_read(const std::string &path, std::vector<char> &code) {
    if (path.empty()) return false;
    const int fd = open(path.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
    if (fd < 0) return false;
    struct stat st;
    bool ok = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_uid == geteuid() && !(st.st_mode & (S_IWGRP | S_IWOTH)) && st.st_size > 0;
    if (ok) {
        code.resize((size_t)st.st_size);
        size_t got = 0;
        while (got < code.size()) {
            const ssize_t r = read(fd, code.data() + got, code.size() - got);
            if (r <= 0) break;
            got += (size_t)r;
        }
        ok = got == code.size();
    }
    close(fd);
    if (!ok) code.clear();
    return ok;
}
// a new 0600 file of this user, renamed into place when it is complete
inline void jit_cache_write(const std::string &path, const std::vector<char> &code) {
    if (path.empty() || code.empty()) return;
    const std::string t = path + "." + std::to_string((int)getpid()) + ".tmp";
    const int fd = open(t.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600);
    if (fd < 0) return;
    size_t put = 0;
    while (put < code.size()) {
        const ssize_t r = write(fd, code.data() + put, code.size() - put);
        if (r <= 0) break;
        put += (size_t)r;
    }
    close(fd);
    if (put == code.size()) rename(t.c_str(), path.c_str()); else remove(t.c_str());
}
