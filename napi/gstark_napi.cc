// napi/gstark_napi.cc — thin N-API shim over the C ABI of include/gstark.h.
//
// This is the binding a genSTARK maintainer adds in place of the wasm loaders of @guildofweavers/galois and
// @guildofweavers/merkle: it dlopen()s libgstark_hip.so and forwards calls 1:1.  No arithmetic happens here.  open(path) returns one
// object per loaded library (field flavour), so one process can work in several fields; the module-level members act on the library
// of the last load().
// JS-side conventions (used by js/galois.js and js/merkle.js, which rebuild the FiniteField / Hash / MerkleTree
// objects lib/Stark.ts consumes):
//   * a context is an External; a device pointer is a BigInt; sizes/counts are Numbers (or BigInts);
//   * host byte arguments are Buffers (inputs are read, outputs are written in place);
//   * arrays of device pointers / of 64-bit indexes are JS arrays of BigInt / Number.
// Every gs_* function returns gs_status; a non-zero status is thrown as an Error carrying gs_last_error().
//
// build (no node-gyp needed):  g++ -O2 -shared -fPIC -I/usr/include/node napi/gstark_napi.cc -o napi/gstark_napi.node -ldl
#include <dlfcn.h>
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <numeric>
#include <string>
#include <unordered_set>
#include <vector>

#include "../include/gstark.h"
#include "../include/gstark_prover.h"
#include "../include/gstark_diagnose.h"

namespace {

// One loaded implementation of include/gstark.h (a field flavour): its dl handle, the contexts it created, and its bindings of the
// native driver (gs_prover_open against THIS handle, keyed by the driver's path).  open(path) returns it as an object whose members are
// the module's; the module-level members act on the library of the last load().  Libraries and bindings live as long as the process:
// proofs that alternate between fields never close or reopen anything.
struct Driver {
    void *dl = nullptr;
    gs_prover_binding *binding = nullptr;
};
struct Lib {
    void *dl = nullptr;
    size_t es = 0;
    std::string backend;
    std::map<std::string, Driver> drivers;
    std::unordered_set<void *> ctxs;       // gs_ctx layouts differ between flavours: a context is only ever handed to the library that made it
};
std::vector<Lib *> g_libs;
Lib *g_cur = nullptr;                      // the module-level surface: the last load()

#define NAPI_OK(env, call)                                                \
    do {                                                                  \
        if ((call) != napi_ok) {                                          \
            napi_throw_error((env), nullptr, "N-API call failed: " #call); \
            return nullptr;                                               \
        }                                                                 \
    } while (0)

// One descriptor per exported function: argument kinds after the optional leading ctx.
//   c ctx | p device pointer | u uint64 | i int/uint32 | b host bytes in | o host bytes out |
//   a array of device pointers | x array of uint64 | w array of uint32
struct FnDesc {
    const char *name;
    const char *sig;
};
const FnDesc kFns[] = {
    {"gs_sync", "c"},
    {"gs_free", "cp"},
    {"gs_cache_trim", "c"},
    {"gs_upload", "cpbu"},
    {"gs_download", "copu"},
    {"gs_copy", "cppu"},
    {"gs_gather", "cpuxuo"},
    {"gs_power_series", "cbup"},
    {"gs_vec_add", "cppup"},
    {"gs_vec_sub", "cppup"},
    {"gs_vec_mul", "cppup"},
    {"gs_vec_add_scalar", "cpbup"},
    {"gs_vec_sub_scalar", "cpbup"},
    {"gs_vec_mul_scalar", "cpbup"},
    {"gs_vec_inv", "cpup"},
    {"gs_vec_div", "cppup"},
    {"gs_vec_exp", "cpbup"},
    {"gs_combine_many", "cabiup"},
    {"gs_combine", "cppuo"},
    {"gs_air_jit", "ci"},
    {"gs_air_jit_launches", "c"},
    {"gs_defer_begin", "c"},
    {"gs_defer_end", "c"},
    {"gs_pluck", "cpuuup"},
    {"gs_zero_poly_inverses", "cbuubp"},
    {"gs_div_by_domain_roots", "cpiubxwip"},
    {"gs_transpose_vector", "cpuiup"},
    {"gs_transpose_matrix", "cpuup"},
    {"gs_sub_matrix_from_vectors", "capiup"},
    {"gs_eval_polys_at_roots", "cpiubup"},
    {"gs_interpolate_roots", "cpibup"},
    {"gs_eval_poly_at", "cpubo"},
    {"gs_interpolate_quartic_batch", "cppup"},
    {"gs_interpolate_quartic_domain", "cbuupup"},
    {"gs_eval_quartic_batch", "cpubp"},
    {"gs_fri_fold", "cbuupubp"},
    {"gs_fri_fold_seeded", "cbuupupp"},
    {"gs_hash_digest", "cibuo"},
    {"gs_hash_merge_rows", "ciaiup"},
    {"gs_hash_digest_values", "cipuup"},
    {"gs_merkle_build", "cipup"},
    {"gs_mimc_trace", "cbbiup"},
    {"gs_mimc_constraints", "cpuupup"},
    {"gs_mimc_composition", "cpuubpubuubxibp"},
    {"gs_air_trace", "cwibiiibwibup"},
    {"gs_air_trace_segments", "cwiwibiiibwibuup"},
    {"gs_air_constraints", "cwibiiiipuupxip"},
    {"gs_air_jit_check", "iwiwibiiixiou"},
    {"gs_set_modulus", "bi"},
    {"gs_small_interpolate", "bbio"},
    // include/gstark_boundary.h: OPTIONAL on a library (symbols are resolved per call: a library without it answers "symbol not found")
    {"gs_boundary_polys", "cbuuxbwiipp"},
    {"gs_eval_polys_at_points", "cpiuxbip"},
    // include/gstark_hades.h: OPTIONAL in the same way.  gs_hades_create writes the handle (a pointer) into an 8-byte Buffer; the handle
    // then travels as a BigInt like a device pointer
    {"gs_hades_create", "ciiiubbo"},
    {"gs_hades_destroy", "cp"},
    {"gs_hades_hash", "cppuiip"},
    {"gs_hades_merkle", "cppuip"},
    {"gs_hades_merkle_paths", "cpuixup"},
    // include/gstark_rescue.h: OPTIONAL in the same way; the handle travels like gs_hades_create's.  Paths: gs_hades_merkle_paths
    {"gs_rescue_create", "ciiubbbo"},
    {"gs_rescue_destroy", "cp"},
    {"gs_rescue_hash", "cppuiiiip"},
    {"gs_rescue_merkle", "cppup"},
    // include/gstark_tree_update.h: OPTIONAL in the same way; the handles are those of gs_hades_create / gs_rescue_create
    {"gs_hades_merkle_update", "cppuixpupp"},
    {"gs_rescue_merkle_update", "cppuxpupp"},
    // include/gstark_tree_verify.h: OPTIONAL in the same way; `leaves` may be 0 (a path then starts from its own leaf)
    {"gs_hades_merkle_path_roots", "cppiixpup"},
    {"gs_rescue_merkle_path_roots", "cppixpup"},
    // include/gstark_sparse_tree.h: OPTIONAL in the same way; the create entries write the tree (a pointer) into an 8-byte Buffer like
    // gs_hades_create, the empty leaf is host bytes; indexes travel as an array of Numbers or BigInts (64 bits each).
    // gs_sparse_stored returns a count, not a status: call() does not deliver it, so it is not listed
    {"gs_hades_sparse_create", "cpiibuo"},
    {"gs_rescue_sparse_create", "cpibuo"},
    {"gs_sparse_update", "cpxpupp"},
    {"gs_sparse_paths", "cpxup"},
    {"gs_sparse_root", "cpp"},
    {"gs_sparse_empties", "cpp"},
    {"gs_sparse_destroy", "cp"},
    // include/gstark_curve.h: OPTIONAL in the same way; `addends` and `addend_inf` may be 0 (every addend / no addend is infinity)
    {"gs_curve_mul", "cbpupippupp"},
    {"gs_curve_contains", "cbbpup"},
    // include/gstark_msm.h: OPTIONAL in the same way; `points` and `scalars` may be 0 for the empty sum
    {"gs_curve_msm", "cbppiiuipp"},
    // include/gstark_poly.h: OPTIONAL in the same way; an operand of no element may be 0
    {"gs_poly_from_roots", "cbipup"},
    {"gs_poly_div", "cbipupupp"},
    {"gs_poly_eval_points", "cbipupup"},
    {"gs_poly_interpolate_points", "cbippupp"},
    // include/gstark_sqrt.h: OPTIONAL in the same way; `roots_out` and `parities` may be 0 (flags only / every y even); the plan's four
    // results are host uint32 (Buffers of 4 bytes)
    {"gs_field_sqrt", "cpupp"},
    {"gs_curve_lift_x", "cbbppupp"},
    {"gs_curve_compress", "cpupp"},
    {"gs_field_sqrt_plan", "coooo"},
    // include/gstark_scan.h: OPTIONAL in the same way; `heads`, `totals_out` and the affine entry's `a` may be 0 (a = 0: the factor is the
    // host element that follows it); the plan's results are host uint32, uint32, uint64, uint32
    {"gs_scan", "ciippuupp"},
    {"gs_scan_affine", "cipbpbpuup"},
    {"gs_reduce", "cipuup"},
    {"gs_scan_plan", "cuoooo"},
    // include/gstark_absorb.h: OPTIONAL in the same way; the handles are those of gs_hades_create / gs_rescue_create
    {"gs_hades_absorb", "cppuiuuiip"},
    {"gs_rescue_absorb", "cppuiuuiiip"},
    // include/gstark_diagnose.h: OPTIONAL in the same way; the three results are host arrays of `rows` uint64 each (Buffers of 8 * rows bytes)
    {"gs_nonzero_spans", "cpuuuooo"},
    {"gs_pseudorandom_indexes", "biiuio"},
    {"gs_small_eval_poly", "bibio"},
};

// napi_get_buffer_info on a value that is not a Buffer ABORTS the process in node 12 (an assertion inside node::Buffer::Data, found by
// tests/addon_validation.js): ask first
bool buffer_info(napi_env env, napi_value v, void **data, size_t *len) {
    bool is = false;
    if (napi_is_buffer(env, v, &is) != napi_ok || !is) return false;
    return napi_get_buffer_info(env, v, data, len) == napi_ok;
}

bool get_u64(napi_env env, napi_value v, uint64_t *out) {
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok) return false;
    if (t == napi_bigint) {
        bool lossless;
        return napi_get_value_bigint_uint64(env, v, out, &lossless) == napi_ok;
    }
    if (t == napi_number) {
        double d;
        if (napi_get_value_double(env, v, &d) != napi_ok || d < 0) return false;
        *out = (uint64_t)d;
        return true;
    }
    return false;
}

// the library a member acts on: a library object's (the function's data), else the module-level one; throws when there is none
Lib *lib_of(napi_env env, void *data) {
    Lib *L = data ? (Lib *)data : g_cur;
    if (!L) napi_throw_error(env, nullptr, "call load(path) first");
    return L;
}
// a context argument: an External this library created (never one of another library's, nor one it destroyed)
enum CtxArg { CTX_OK, CTX_NOT_EXTERNAL, CTX_FOREIGN };
CtxArg get_ctx(napi_env env, const Lib *L, napi_value v, void **out) {
    void *p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) return CTX_NOT_EXTERNAL;
    if (!L->ctxs.count(p)) return CTX_FOREIGN;
    *out = p;
    return CTX_OK;
}
void throw_foreign(napi_env env, const char *what) {
    napi_throw_type_error(env, nullptr, (std::string(what) + ": the context was not created by this library (a context belongs to one field's library)").c_str());
}

typedef int (*fn16)(uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                    uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t);

// has(name): whether this library exports an entry point of the table — the optional ones (include/gstark_boundary.h) are asked for
// before they are used
napi_value Has(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    void *data;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, &data));
    if (argc < 1) { napi_throw_type_error(env, nullptr, "has(name)"); return nullptr; }
    Lib *L = lib_of(env, data);
    if (!L) return nullptr;
    char name[64];
    size_t len;
    if (napi_get_value_string_utf8(env, argv[0], name, sizeof name, &len) != napi_ok) { napi_throw_type_error(env, nullptr, "has(name): the name is a string"); return nullptr; }
    bool known = false;
    for (const FnDesc &f : kFns)
        if (!strcmp(f.name, name)) known = true;
    napi_value out;
    NAPI_OK(env, napi_get_boolean(env, known && dlsym(L->dl, name) != nullptr, &out));
    return out;
}

// call(name, ...args): generic forwarder.  All ABI parameters are integers or pointers, which the x86-64 SysV
// calling convention passes in 8-byte slots; narrower parameters read the low bytes of their slot.
napi_value Call(napi_env env, napi_callback_info info) {
    size_t argc = 20;
    napi_value argv[20];
    void *data;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, &data));
    if (argc < 1) { napi_throw_type_error(env, nullptr, "call(name, ...args)"); return nullptr; }
    Lib *L = lib_of(env, data);
    if (!L) return nullptr;
    char name[64];
    size_t len;
    if (napi_get_value_string_utf8(env, argv[0], name, sizeof name, &len) != napi_ok) { napi_throw_type_error(env, nullptr, "call(name, ...args): the name is a string"); return nullptr; }
    const FnDesc *d = nullptr;
    for (const FnDesc &f : kFns)
        if (!strcmp(f.name, name)) d = &f;
    if (!d) { napi_throw_error(env, nullptr, (std::string("unknown gstark function ") + name).c_str()); return nullptr; }
    const size_t n = strlen(d->sig);
    if (argc - 1 != n) { napi_throw_type_error(env, nullptr, (std::string(name) + ": wrong number of arguments").c_str()); return nullptr; }
    void *sym = dlsym(L->dl, name);
    if (!sym) { napi_throw_error(env, nullptr, (std::string("symbol not found: ") + name).c_str()); return nullptr; }
    uintptr_t a[16] = {0};
    std::vector<std::vector<uint64_t>> arrays;
    std::vector<std::vector<uint32_t>> arrays32;
    arrays.reserve(4);
    arrays32.reserve(4);
    gs_ctx *ctx = nullptr;
    for (size_t i = 0; i < n; i++) {
        napi_value v = argv[i + 1];
        switch (d->sig[i]) {
            case 'c': {
                void *p = nullptr;
                const CtxArg c = get_ctx(env, L, v, &p);
                if (c == CTX_NOT_EXTERNAL) { napi_throw_type_error(env, nullptr, (std::string(name) + ": expected a context").c_str()); return nullptr; }
                if (c == CTX_FOREIGN) { throw_foreign(env, name); return nullptr; }
                ctx = (gs_ctx *)p;
                a[i] = (uintptr_t)p;
                break;
            }
            case 'p': case 'u': case 'i': {
                uint64_t x;
                if (!get_u64(env, v, &x)) { napi_throw_type_error(env, nullptr, (std::string(name) + ": expected a number/BigInt").c_str()); return nullptr; }
                a[i] = (uintptr_t)x;
                break;
            }
            case 'b': case 'o': {
                void *data;
                size_t blen;
                if (!buffer_info(env, v, &data, &blen)) { napi_throw_type_error(env, nullptr, (std::string(name) + ": expected a Buffer").c_str()); return nullptr; }
                a[i] = (uintptr_t)data;
                break;
            }
            case 'a': case 'x': {
                uint32_t alen;
                NAPI_OK(env, napi_get_array_length(env, v, &alen));
                arrays.emplace_back(alen);
                for (uint32_t k = 0; k < alen; k++) {
                    napi_value e;
                    NAPI_OK(env, napi_get_element(env, v, k, &e));
                    if (!get_u64(env, e, &arrays.back()[k])) { napi_throw_type_error(env, nullptr, (std::string(name) + ": bad array element").c_str()); return nullptr; }
                }
                a[i] = (uintptr_t)arrays.back().data();
                break;
            }
            case 'w': {
                uint32_t alen;
                NAPI_OK(env, napi_get_array_length(env, v, &alen));
                arrays32.emplace_back(alen);
                for (uint32_t k = 0; k < alen; k++) {
                    napi_value e;
                    uint64_t x;
                    NAPI_OK(env, napi_get_element(env, v, k, &e));
                    if (!get_u64(env, e, &x)) { napi_throw_type_error(env, nullptr, (std::string(name) + ": bad array element").c_str()); return nullptr; }
                    arrays32.back()[k] = (uint32_t)x;
                }
                a[i] = (uintptr_t)arrays32.back().data();
                break;
            }
            default:
                napi_throw_error(env, nullptr, "bad descriptor");
                return nullptr;
        }
    }
    int rc = ((fn16)sym)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15]);
    if (rc != GS_OK) {
        typedef const char *(*errfn)(const gs_ctx *);
        errfn le = (errfn)dlsym(L->dl, "gs_last_error");
        std::string msg = std::string(name) + " failed (" + std::to_string(rc) + ")";
        if (ctx && le) msg += std::string(": ") + le(ctx);
        napi_throw_error(env, nullptr, msg.c_str());
        return nullptr;
    }
    napi_value undef;
    napi_get_undefined(env, &undef);
    return undef;
}

// dlopen(path) -> the library's record (one per dl handle: the same path opened twice is the same library); throws and returns null on failure
Lib *open_lib(napi_env env, napi_value path_value, const char *usage) {
    char path[1024];
    size_t len;
    if (napi_get_value_string_utf8(env, path_value, path, sizeof path, &len) != napi_ok) { napi_throw_type_error(env, nullptr, usage); return nullptr; }
    void *lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!lib) { napi_throw_error(env, nullptr, (std::string("cannot load ") + path + ": " + dlerror() + " (there is no CPU fallback)").c_str()); return nullptr; }
    typedef const char *(*namefn)(void);
    typedef int (*sizefn)(void);
    namefn nf = (namefn)dlsym(lib, "gs_backend_name");
    sizefn sf = (sizefn)dlsym(lib, "gs_element_size");
    if (!nf || !sf) { napi_throw_error(env, nullptr, "not a gstark library"); return nullptr; }
    for (Lib *L : g_libs)
        if (L->dl == lib) { dlclose(lib); return L; }       // (drops the reference this dlopen added)
    Lib *L = new Lib;
    L->dl = lib;
    L->es = (size_t)sf();
    L->backend = nf();
    g_libs.push_back(L);
    return L;
}

// load(path): dlopen libgstark_hip.so for the module-level members; returns the backend name
napi_value Load(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    if (argc < 1) { napi_throw_type_error(env, nullptr, "load(path)"); return nullptr; }
    Lib *L = open_lib(env, argv[0], "load(path)");
    if (!L) return nullptr;
    g_cur = L;
    napi_value out;
    NAPI_OK(env, napi_create_string_utf8(env, L->backend.c_str(), NAPI_AUTO_LENGTH, &out));
    return out;
}

// fieldInfo(): { elementSize, modulus: Buffer } of the library (gs_element_size / gs_field_modulus; a runtime-modulus library's modulus
// is the one gs_set_modulus gave it)
napi_value FieldInfo(napi_env env, napi_callback_info info) {
    void *data;
    NAPI_OK(env, napi_get_cb_info(env, info, nullptr, nullptr, nullptr, &data));
    Lib *L = data ? (Lib *)data : g_cur;
    if (!L) { napi_throw_error(env, nullptr, "no library loaded"); return nullptr; }
    typedef int (*modfn)(uint8_t *);
    modfn mf = (modfn)dlsym(L->dl, "gs_field_modulus");
    if (!mf) { napi_throw_error(env, nullptr, "not a gstark library"); return nullptr; }
    const int es = (int)L->es;
    uint8_t mod[64] = {0};
    if (es <= 0 || es > 64 || mf(mod) != GS_OK) { napi_throw_error(env, nullptr, "gs_field_modulus failed"); return nullptr; }
    napi_value out, v;
    NAPI_OK(env, napi_create_object(env, &out));
    NAPI_OK(env, napi_create_uint32(env, (uint32_t)es, &v));
    NAPI_OK(env, napi_set_named_property(env, out, "elementSize", v));
    void *copy;
    NAPI_OK(env, napi_create_buffer_copy(env, (size_t)es, mod, &copy, &v));
    NAPI_OK(env, napi_set_named_property(env, out, "modulus", v));
    return out;
}

napi_value CtxCreate(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    void *data;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, &data));
    int32_t device = 0;
    if (argc >= 1) napi_get_value_int32(env, argv[0], &device);
    Lib *L = lib_of(env, data);
    if (!L) return nullptr;
    typedef int (*createfn)(int, void *, gs_ctx **);
    createfn cf = (createfn)dlsym(L->dl, "gs_ctx_create");
    gs_ctx *ctx = nullptr;
    int rc = cf(device, nullptr, &ctx);
    if (rc != GS_OK || !ctx) {
        napi_throw_error(env, nullptr, ("gs_ctx_create failed (" + std::to_string(rc) + "): no gfx950 device; there is no CPU fallback").c_str());
        return nullptr;
    }
    L->ctxs.insert(ctx);
    napi_value out;
    NAPI_OK(env, napi_create_external(env, ctx, nullptr, nullptr, &out));
    return out;
}

napi_value CtxDestroy(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    void *data;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, &data));
    void *p = nullptr;
    Lib *L = lib_of(env, data);
    if (!L) return nullptr;
    const CtxArg c = argc < 1 ? CTX_NOT_EXTERNAL : get_ctx(env, L, argv[0], &p);
    if (c == CTX_NOT_EXTERNAL) { napi_throw_type_error(env, nullptr, "ctxDestroy(ctx)"); return nullptr; }
    if (c == CTX_FOREIGN) { throw_foreign(env, "ctxDestroy"); return nullptr; }
    typedef void (*dfn)(gs_ctx *);
    ((dfn)dlsym(L->dl, "gs_ctx_destroy"))((gs_ctx *)p);
    L->ctxs.erase(p);
    napi_value undef;
    napi_get_undefined(env, &undef);
    return undef;
}

// alloc(ctx, bytes) -> BigInt device pointer
napi_value Alloc(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    void *data;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, &data));
    void *p = nullptr;
    Lib *L = lib_of(env, data);
    if (!L) return nullptr;
    uint64_t bytes;
    const CtxArg c = argc < 2 ? CTX_NOT_EXTERNAL : get_ctx(env, L, argv[0], &p);
    if (c == CTX_NOT_EXTERNAL || !get_u64(env, argv[1], &bytes)) { napi_throw_type_error(env, nullptr, "alloc(ctx, bytes)"); return nullptr; }
    if (c == CTX_FOREIGN) { throw_foreign(env, "alloc"); return nullptr; }
    typedef int (*afn)(gs_ctx *, uint64_t, void **);
    void *d = nullptr;
    int rc = ((afn)dlsym(L->dl, "gs_alloc"))((gs_ctx *)p, bytes, &d);
    if (rc != GS_OK) { napi_throw_error(env, nullptr, "gs_alloc failed"); return nullptr; }
    napi_value out;
    NAPI_OK(env, napi_create_bigint_uint64(env, (uint64_t)(uintptr_t)d, &out));
    return out;
}

// merkleProveBatch(ctx, leavesPtr, nodesPtr, n, indexes[]) -> { values: Buffer, colLens: number[], nodes: Buffer }
napi_value MerkleProveBatch(napi_env env, napi_callback_info info) {
    size_t argc = 5;
    napi_value argv[5];
    void *data;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, &data));
    void *p = nullptr;
    Lib *L = lib_of(env, data);
    if (!L) return nullptr;
    uint64_t leaves, nodes, n;
    const CtxArg c = argc < 5 ? CTX_NOT_EXTERNAL : get_ctx(env, L, argv[0], &p);
    if (c == CTX_NOT_EXTERNAL || !get_u64(env, argv[1], &leaves) || !get_u64(env, argv[2], &nodes) ||
        !get_u64(env, argv[3], &n) || n < 2 || (n & (n - 1)) || n > (1ull << 40)) { napi_throw_type_error(env, nullptr, "merkleProveBatch: bad arguments"); return nullptr; }
    if (c == CTX_FOREIGN) { throw_foreign(env, "merkleProveBatch"); return nullptr; }
    uint32_t count;
    if (napi_get_array_length(env, argv[4], &count) != napi_ok || count > (1u << 20)) { napi_throw_type_error(env, nullptr, "merkleProveBatch: bad index list"); return nullptr; }
    std::vector<uint64_t> idx(count);
    for (uint32_t k = 0; k < count; k++) {
        napi_value e;
        NAPI_OK(env, napi_get_element(env, argv[4], k, &e));
        if (!get_u64(env, e, &idx[k]) || idx[k] >= n) { napi_throw_type_error(env, nullptr, "merkleProveBatch: bad index"); return nullptr; }
    }
    int depth = 0;
    while ((1ull << depth) < n) depth++;
    const uint64_t cap = (uint64_t)count * (depth ? depth : 1);
    std::vector<uint8_t> values((size_t)count * 32), nd((size_t)cap * 32);
    std::vector<uint32_t> lens(count ? count : 1);
    uint32_t ncols = 0;
    typedef int (*pfn)(gs_ctx *, const void *, const void *, uint64_t, const uint64_t *, uint32_t, uint8_t *, uint32_t *, uint32_t *, uint8_t *, uint64_t);
    int rc = ((pfn)dlsym(L->dl, "gs_merkle_prove_batch"))((gs_ctx *)p, (const void *)(uintptr_t)leaves, (const void *)(uintptr_t)nodes, n, idx.data(),
                                                          count, values.data(), &ncols, lens.data(), nd.data(), cap);
    if (rc != GS_OK) {
        typedef const char *(*errfn)(const gs_ctx *);
        napi_throw_error(env, nullptr, ((errfn)dlsym(L->dl, "gs_last_error"))((gs_ctx *)p));
        return nullptr;
    }
    uint64_t total = 0;
    for (uint32_t i = 0; i < ncols; i++) total += lens[i];
    napi_value out, v, nb, arr;
    NAPI_OK(env, napi_create_object(env, &out));
    NAPI_OK(env, napi_create_buffer_copy(env, values.size(), values.data(), nullptr, &v));
    NAPI_OK(env, napi_create_buffer_copy(env, (size_t)total * 32, nd.data(), nullptr, &nb));
    NAPI_OK(env, napi_create_array_with_length(env, ncols, &arr));
    for (uint32_t i = 0; i < ncols; i++) {
        napi_value e;
        NAPI_OK(env, napi_create_uint32(env, lens[i], &e));
        NAPI_OK(env, napi_set_element(env, arr, i, e));
    }
    NAPI_OK(env, napi_set_named_property(env, out, "values", v));
    NAPI_OK(env, napi_set_named_property(env, out, "nodes", nb));
    NAPI_OK(env, napi_set_named_property(env, out, "colLens", arr));
    return out;
}

// proveMimcSerialized(ctx, proverLibPath, job) -> Buffer: ONE call = Stark.prove() + Serializer.serializeProof() of the MiMC AIR through
// the native driver (include/gstark_prover.h; the driver is bound to the ABI library the member belongs to: a library object's, or the
// one load() opened).
//   job = { steps, extensionFactor, exeQueryCount, friQueryCount, hashAlg, rootOfUnity: Buffer(es), seed: Buffer(es),
//           roundConstants: Buffer(es*n), kTable: BigInt (device pointer), kLen, assertions: [{step, register, value: Buffer(es)}] }   (es = gs_element_size() of that library)
// The driver library is the build for that ABI library's field (js/prover.js picks libgstark_prover*.so by modulus); each ABI library
// keeps its own binding of it (gs_prover_open: nothing process-wide is written), opened on first use and kept.  Scalars of a job are
// gs_element_size() bytes each.
typedef int (*prove_on_fn)(const gs_prover_binding *, gs_ctx *, const gs_prover_job *, uint8_t *, uint64_t, uint64_t *, char *, uint64_t);
const Driver *open_driver(napi_env env, Lib *L, napi_value path_value) {
    char path[1024];
    size_t len;
    if (napi_get_value_string_utf8(env, path_value, path, sizeof path, &len) != napi_ok) { napi_throw_type_error(env, nullptr, "driver library path expected"); return nullptr; }
    auto hit = L->drivers.find(path);
    if (hit != L->drivers.end()) return &hit->second;
    void *lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!lib) { napi_throw_error(env, nullptr, (std::string("cannot load ") + path + ": " + dlerror()).c_str()); return nullptr; }
    typedef int (*openfn)(void *, gs_prover_binding **);
    openfn of = (openfn)dlsym(lib, "gs_prover_open");
    Driver d;
    if (!of || of(L->dl, &d.binding) != GS_OK || !dlsym(lib, "gs_prover_prove_on") || !dlsym(lib, "gs_prover_verify_on")) {
        napi_throw_error(env, nullptr, "gs_prover_open failed: the driver library is not the build for the loaded library's field");
        dlclose(lib);
        return nullptr;
    }
    d.dl = lib;
    return &(L->drivers[path] = d);
}
typedef int (*verify_on_fn)(const gs_prover_binding *, const gs_prover_job *, const uint8_t *, uint64_t, char *, uint64_t);
// a 4th argument (a Buffer holding a serialized proof) turns either call below into Stark.verify() of that proof for the statement the job
// describes (include/gstark_prover.h: gs_prover_verify_on — native, CPU only): returns true or throws the reference's message.
// A 5th argument `true` asks for gs_prover_verify_device_on with the member's context (the long polynomials of a statement on the device:
// same answer, same message); a driver build without that entry verifies on the host.
typedef int (*verify_device_on_fn)(const gs_prover_binding *, gs_ctx *, const gs_prover_job *, const uint8_t *, uint64_t, char *, uint64_t);
napi_value verify_instead(napi_env env, const Driver *drv, napi_value proof_value, const gs_prover_job &job, void *ctx, napi_value device_value) {
    void *d;
    size_t len;
    if (!buffer_info(env, proof_value, &d, &len)) { napi_throw_type_error(env, nullptr, "the proof must be a Buffer"); return nullptr; }
    bool device = false;
    if (device_value && napi_get_value_bool(env, device_value, &device) != napi_ok) { napi_throw_type_error(env, nullptr, "device: a boolean expected"); return nullptr; }
    char err[512] = {0};
    verify_device_on_fn on_device = device ? (verify_device_on_fn)dlsym(drv->dl, "gs_prover_verify_device_on") : nullptr;
    const int rc = on_device ? on_device(drv->binding, (gs_ctx *)ctx, &job, (const uint8_t *)d, len, err, sizeof err)
                             : ((verify_on_fn)dlsym(drv->dl, "gs_prover_verify_on"))(drv->binding, &job, (const uint8_t *)d, len, err, sizeof err);
    if (rc != GS_OK) { napi_throw_error(env, nullptr, err[0] ? err : "verification failed"); return nullptr; }
    napi_value t;
    NAPI_OK(env, napi_get_boolean(env, true, &t));
    return t;
}
// the (ctx, proverLibPath, job[, proof]) head of both one-call entries: the library, its context, its binding of the driver
const Driver *one_call_head(napi_env env, napi_callback_info info, size_t *argc, napi_value *argv, Lib **L, void **ctx) {
    void *data;
    if (napi_get_cb_info(env, info, argc, argv, nullptr, &data) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: napi_get_cb_info"); return nullptr; }
    *L = lib_of(env, data);
    if (!*L) return nullptr;
    napi_valuetype job_type;
    const CtxArg c = *argc < 3 ? CTX_NOT_EXTERNAL : get_ctx(env, *L, argv[0], ctx);
    if (c == CTX_NOT_EXTERNAL || napi_typeof(env, argv[2], &job_type) != napi_ok || job_type != napi_object) {
        napi_throw_type_error(env, nullptr, "(ctx, proverLibPath, job[, proof])");
        return nullptr;
    }
    if (c == CTX_FOREIGN) { throw_foreign(env, "prove"); return nullptr; }
    return open_driver(env, *L, argv[1]);
}
napi_value ProveMimcSerialized(napi_env env, napi_callback_info info) {
    size_t argc = 5;
    napi_value argv[5];
    void *ctx = nullptr;
    Lib *L = nullptr;
    const Driver *drv = one_call_head(env, info, &argc, argv, &L, &ctx);
    if (!drv) return nullptr;
    const size_t es = L->es;
    auto prop = [&](const char *name) { napi_value v; napi_get_named_property(env, argv[2], name, &v); return v; };
    auto u64 = [&](const char *name, uint64_t *out) { return get_u64(env, prop(name), out); };
    auto bytes = [&](napi_value v, const uint8_t **data, size_t *len) { void *d; bool ok = buffer_info(env, v, &d, len); *data = (const uint8_t *)d; return ok; };
    gs_prover_job job;
    memset(&job, 0, sizeof job);
    uint64_t t, ef, exe, fri, alg, klen, ktab;
    const uint8_t *rou, *seed, *rc;
    size_t nrou, nseed, nrc;
    if (!u64("steps", &t) || !u64("extensionFactor", &ef) || !u64("exeQueryCount", &exe) || !u64("friQueryCount", &fri) || !u64("hashAlg", &alg) ||
        !u64("kLen", &klen) || !u64("kTable", &ktab) || !bytes(prop("rootOfUnity"), &rou, &nrou) || nrou != es || !bytes(prop("seed"), &seed, &nseed) ||
        nseed != es || !bytes(prop("roundConstants"), &rc, &nrc) || nrc % es) {
        napi_throw_type_error(env, nullptr, "proveMimcSerialized: malformed job");
        return nullptr;
    }
    job.steps = t; job.extension_factor = (uint32_t)ef; job.exe_query_count = (uint32_t)exe; job.fri_query_count = (uint32_t)fri; job.hash_alg = (int32_t)alg;
    memcpy(job.root_of_unity, rou, es);
    const uint32_t degree = 3;
    job.air.kind = 0; job.air.registers = 1; job.air.nconstraints = 1; job.air.degrees = &degree;
    memcpy(job.air.seed, seed, es);
    job.air.round_constants = rc; job.air.nrc = (uint32_t)(nrc / es);
    job.air.k_table = (const void *)(uintptr_t)ktab; job.air.k_len = klen;
    napi_value arr = prop("assertions");
    uint32_t na = 0;
    NAPI_OK(env, napi_get_array_length(env, arr, &na));
    std::vector<gs_assertion> as(na);
    for (uint32_t i = 0; i < na; i++) {
        napi_value e, v;
        NAPI_OK(env, napi_get_element(env, arr, i, &e));
        uint64_t step, reg;
        const uint8_t *val; size_t nval;
        napi_get_named_property(env, e, "step", &v);
        bool ok = get_u64(env, v, &step);
        napi_get_named_property(env, e, "register", &v);
        ok = ok && get_u64(env, v, &reg);
        napi_get_named_property(env, e, "value", &v);
        ok = ok && bytes(v, &val, &nval) && nval == es;
        if (!ok) { napi_throw_type_error(env, nullptr, "proveMimcSerialized: malformed assertion"); return nullptr; }
        as[i].step = step; as[i].reg = (uint32_t)reg; memcpy(as[i].value, val, es);
    }
    job.assertions = as.data(); job.nassertions = na;
    if (argc >= 4) return verify_instead(env, drv, argv[3], job, ctx, argc >= 5 ? argv[4] : nullptr);
    static thread_local std::vector<uint8_t> out;      // (kept between calls: a fresh vector of this size is 4 MB of zeroing per proof)
    if (out.size() < (1u << 22)) out.resize(1u << 22);
    uint64_t n = 0;
    char err[512] = {0};
    int rcode = ((prove_on_fn)dlsym(drv->dl, "gs_prover_prove_on"))(drv->binding, (gs_ctx *)ctx, &job, out.data(), out.size(), &n, err, sizeof err);
    if (rcode != GS_OK) { napi_throw_error(env, nullptr, (std::string("native prove() failed: ") + err).c_str()); return nullptr; }
    napi_value buf;
    NAPI_OK(env, napi_create_buffer_copy(env, (size_t)n, out.data(), nullptr, &buf));
    return buf;
}

typedef int (*diagnose_on_fn)(const gs_prover_binding *, gs_ctx *, const gs_prover_job *, gs_diagnose_constraint *, uint32_t *, gs_diagnose_assertion *, uint32_t,
                              uint32_t *, char *, uint64_t);
static napi_value diagnosis_of(napi_env env, const Driver *drv, const gs_prover_job &job, void *ctx, size_t es) {
    diagnose_on_fn fn = (diagnose_on_fn)dlsym(drv->dl, "gs_prover_diagnose_on");
    if (!fn) { napi_throw_error(env, nullptr, "the native driver has no gs_prover_diagnose_on (include/gstark_diagnose.h)"); return nullptr; }
    std::vector<gs_diagnose_constraint> cons(job.air.nconstraints ? job.air.nconstraints : 1);
    std::vector<gs_diagnose_assertion> bad(job.nassertions ? job.nassertions : 1);
    uint32_t ncons = 0, nbad = 0;
    char err[512] = {0};
    int rcode = fn(drv->binding, (gs_ctx *)ctx, &job, cons.data(), &ncons, bad.data(), job.nassertions, &nbad, err, sizeof err);
    if (rcode != GS_OK) { napi_throw_error(env, nullptr, (std::string("native diagnose() failed: ") + err).c_str()); return nullptr; }
    auto number = [&](napi_value obj, const char *name, uint64_t v) { napi_value x; napi_create_double(env, (double)v, &x); napi_set_named_property(env, obj, name, x); };
    auto flag = [&](napi_value obj, const char *name, bool v) { napi_value x; napi_get_boolean(env, v, &x); napi_set_named_property(env, obj, name, x); };
    auto element = [&](napi_value obj, const char *name, const uint8_t *le) {
        uint64_t words[GS_PROVER_ELT_MAX / 8] = {0};
        memcpy(words, le, es);
        napi_value x;
        napi_create_bigint_words(env, 0, (es + 7) / 8, words, &x);
        napi_set_named_property(env, obj, name, x);
    };
    napi_value out, as, cs;
    NAPI_OK(env, napi_create_object(env, &out));
    NAPI_OK(env, napi_create_array_with_length(env, nbad, &as));
    NAPI_OK(env, napi_create_array_with_length(env, ncons, &cs));
    for (uint32_t i = 0; i < nbad && i < job.nassertions; i++) {
        napi_value o;
        NAPI_OK(env, napi_create_object(env, &o));
        number(o, "index", bad[i].index);
        element(o, "found", bad[i].found);
        napi_set_element(env, as, i, o);
    }
    for (uint32_t i = 0; i < ncons; i++) {
        const gs_diagnose_constraint &c = cons[i];
        napi_value o;
        NAPI_OK(env, napi_create_object(env, &o));
        number(o, "index", i); number(o, "violations", c.violations); number(o, "firstStep", c.first_step); number(o, "lastStep", c.last_step);
        element(o, "firstValue", c.first_value);
        number(o, "degree", c.degree); number(o, "declared", c.declared); number(o, "limit", c.limit); number(o, "needed", c.needed);
        flag(o, "atLeast", c.at_least != 0); flag(o, "allZero", c.all_zero != 0);
        napi_set_element(env, cs, i, o);
    }
    napi_set_named_property(env, out, "assertions", as);
    napi_set_named_property(env, out, "constraints", cs);
    return out;
}

// proveGenericSerialized(ctx, proverLibPath, job) -> Buffer: the same ONE call for an AIR given as register-machine programs (kind 1 of
// gs_prover_air: what js/air_generic.js holds for the reference's Rescue / Poseidon examples).
//   job = { steps, extensionFactor, exeQueryCount, friQueryCount, hashAlg, rootOfUnity: Buffer(16), assertions: [...], registers, degrees: number[],
//           tCode / iCode / eCode: number[] (4 words per instruction), consts: Buffer(16 * nconsts), vmRegs, staticValues: Buffer, staticPeriods: number[],
//           staticTables: BigInt (device pointer), staticLens: number[], firstRows: Buffer, segments, segmentLen }
static napi_value generic_one_call(napi_env env, napi_callback_info info, bool diagnose);
napi_value ProveGenericSerialized(napi_env env, napi_callback_info info) { return generic_one_call(env, info, false); }
// diagnoseGenericSerialized(ctx, proverLibPath, job) -> { assertions: [{index, found}], constraints: [{...}] }: the job of
// proveGenericSerialized through gs_prover_diagnose_on (include/gstark_diagnose.h) — no proof; values as BigInt
napi_value DiagnoseGenericSerialized(napi_env env, napi_callback_info info) { return generic_one_call(env, info, true); }
static napi_value generic_one_call(napi_env env, napi_callback_info info, bool diagnose) {
    size_t argc = 5;
    napi_value argv[5];
    void *ctx = nullptr;
    Lib *L = nullptr;
    const Driver *drv = one_call_head(env, info, &argc, argv, &L, &ctx);
    if (!drv) return nullptr;
    const size_t es = L->es;
    auto prop = [&](const char *name) { napi_value v; napi_get_named_property(env, argv[2], name, &v); return v; };
    auto u64 = [&](const char *name, uint64_t *out) { return get_u64(env, prop(name), out); };
    auto bytes = [&](napi_value v, const uint8_t **data, size_t *len) { void *d; bool ok = buffer_info(env, v, &d, len); *data = (const uint8_t *)d; return ok; };
    auto words = [&](const char *name, std::vector<uint32_t> &out) {
        napi_value arr = prop(name);
        uint32_t n = 0;
        if (napi_get_array_length(env, arr, &n) != napi_ok) return false;
        out.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            napi_value e;
            uint64_t x;
            if (napi_get_element(env, arr, i, &e) != napi_ok || !get_u64(env, e, &x)) return false;
            out[i] = (uint32_t)x;
        }
        return true;
    };
    gs_prover_job job;
    memset(&job, 0, sizeof job);
    uint64_t t, ef, exe, fri, alg, regs, vmregs, tables, segments, seglen;
    const uint8_t *rou, *consts, *svals, *first;
    size_t nrou, nconsts, nsvals, nfirst;
    std::vector<uint32_t> degrees, tcode, icode, ecode, periods, lens32;
    if (!u64("steps", &t) || !u64("extensionFactor", &ef) || !u64("exeQueryCount", &exe) || !u64("friQueryCount", &fri) || !u64("hashAlg", &alg) ||
        !u64("registers", &regs) || !u64("vmRegs", &vmregs) || !u64("staticTables", &tables) || !u64("segments", &segments) || !u64("segmentLen", &seglen) ||
        !bytes(prop("rootOfUnity"), &rou, &nrou) || nrou != es || !bytes(prop("consts"), &consts, &nconsts) || nconsts % es ||
        !bytes(prop("staticValues"), &svals, &nsvals) || !bytes(prop("firstRows"), &first, &nfirst) || !words("degrees", degrees) || !words("tCode", tcode) ||
        !words("iCode", icode) || !words("eCode", ecode) || !words("staticPeriods", periods) || !words("staticLens", lens32) || tcode.size() % 4 || icode.size() % 4 ||
        ecode.size() % 4 || lens32.size() != periods.size() || nfirst != (segments ? segments : 1) * regs * es ||
        nsvals < es * std::accumulate(periods.begin(), periods.end(), (uint64_t)0)) {
        napi_throw_type_error(env, nullptr, "proveGenericSerialized: malformed job");
        return nullptr;
    }
    std::vector<uint64_t> lens(lens32.begin(), lens32.end());
    // optional: secret registers and input registers (include/gstark_prover.h, round 6).  secretTraces: BigInt[] (device pointers: the secret
    // registers' extensions; prove) or nsecret (verify); inputRegisters: 5 numbers per register {parent + 1, peer + 1 (0 = none), steps, shift
    // as uint32, secret}; inputShapes: per register rank, dimensions...; staticSources: {kind, index} pairs; publicInputs: Buffer +
    // publicInputCounts; rootOfUnityLog2
    auto has = [&](const char *name) { bool h = false; return napi_has_named_property(env, argv[2], name, &h) == napi_ok && h; };
    std::vector<uint32_t> in_regs, in_shapes, sources, pub_counts32;
    std::vector<uint64_t> secret_ptrs, pub_counts;
    std::vector<const void *> secret_traces;
    std::vector<gs_input_register> decls;
    std::vector<gs_static_source> srcs;
    const uint8_t *pub = nullptr;
    size_t npub = 0;
    uint64_t nsecret = 0, root_log2 = 0;
    bool extra_ok = true;
    if (has("secretTraces")) {
        napi_value arr = prop("secretTraces");
        uint32_t n = 0;
        extra_ok = napi_get_array_length(env, arr, &n) == napi_ok && n <= 64;
        secret_ptrs.resize(extra_ok ? n : 0);
        for (uint32_t i = 0; i < n && extra_ok; i++) { napi_value e; extra_ok = napi_get_element(env, arr, i, &e) == napi_ok && get_u64(env, e, &secret_ptrs[i]) && secret_ptrs[i]; }
        for (uint64_t p : secret_ptrs) secret_traces.push_back((const void *)(uintptr_t)p);
        nsecret = secret_ptrs.size();
    } else if (has("nsecret")) extra_ok = u64("nsecret", &nsecret) && nsecret <= 64;
    if (extra_ok && has("inputRegisters")) {
        extra_ok = words("inputRegisters", in_regs) && in_regs.size() % 5 == 0 && in_regs.size() / 5 <= 255;
        for (size_t j = 0; extra_ok && j < in_regs.size() / 5; j++) {
            gs_input_register d;
            d.parent = (int32_t)in_regs[5 * j] - 1; d.peer = (int32_t)in_regs[5 * j + 1] - 1; d.steps = in_regs[5 * j + 2];
            d.shift = (int32_t)in_regs[5 * j + 3]; d.secret = in_regs[5 * j + 4] ? 1u : 0u;
            extra_ok = d.parent < (int32_t)j && d.peer < (int32_t)j;
            decls.push_back(d);
        }
    }
    if (extra_ok && has("inputShapes")) {
        extra_ok = words("inputShapes", in_shapes);
        size_t at = 0, regs_seen = 0;                       // the flat list must hold exactly one (rank, dims...) group per declared register
        while (extra_ok && at < in_shapes.size()) { extra_ok = in_shapes[at] <= 255 && at + 1 + in_shapes[at] <= in_shapes.size(); at += 1 + (extra_ok ? in_shapes[at] : 0); regs_seen++; }
        extra_ok = extra_ok && regs_seen == decls.size();
    }
    if (extra_ok && has("staticSources")) {
        extra_ok = words("staticSources", sources) && sources.size() % 2 == 0;
        for (size_t i = 0; extra_ok && i < sources.size(); i += 2) srcs.push_back(gs_static_source{sources[i], sources[i + 1]});
    }
    if (extra_ok && has("publicInputs")) {
        extra_ok = bytes(prop("publicInputs"), &pub, &npub) && words("publicInputCounts", pub_counts32);
        uint64_t total = 0;
        for (uint32_t c : pub_counts32) { pub_counts.push_back(c); total += c; }
        extra_ok = extra_ok && npub >= total * es;
    }
    if (extra_ok && has("rootOfUnityLog2")) extra_ok = u64("rootOfUnityLog2", &root_log2) && root_log2 < 64;
    if (!extra_ok) { napi_throw_type_error(env, nullptr, "proveGenericSerialized: malformed job (secret / input registers)"); return nullptr; }
    job.steps = t; job.extension_factor = (uint32_t)ef; job.exe_query_count = (uint32_t)exe; job.fri_query_count = (uint32_t)fri; job.hash_alg = (int32_t)alg;
    memcpy(job.root_of_unity, rou, es);
    gs_prover_air &a = job.air;
    a.kind = 1; a.registers = (uint32_t)regs; a.nconstraints = (uint32_t)degrees.size(); a.degrees = degrees.data();
    a.t_code = tcode.data(); a.t_ninstr = (uint32_t)(tcode.size() / 4);
    a.i_code = icode.empty() ? nullptr : icode.data(); a.i_ninstr = (uint32_t)(icode.size() / 4);
    a.e_code = ecode.data(); a.e_ninstr = (uint32_t)(ecode.size() / 4);
    a.consts = consts; a.nconsts = (uint32_t)(nconsts / es); a.vm_regs = (uint32_t)vmregs;
    a.static_values = svals; a.static_periods = periods.data(); a.nstatic = (uint32_t)periods.size();
    a.static_tables = (const void *)(uintptr_t)tables; a.static_lens = lens.data();
    a.first_rows = first; a.segments = segments; a.segment_len = seglen;
    a.nsecret = (uint32_t)nsecret;
    a.secret_traces = secret_traces.empty() ? nullptr : secret_traces.data();
    if (!decls.empty()) {
        a.inputs = decls.data(); a.ninputs = (uint32_t)decls.size();
        a.input_shapes = in_shapes.empty() ? nullptr : in_shapes.data();
        if (!srcs.empty()) {      // verify: one source per static register; staticPeriods / staticValues then list the cyclic ones only
            uint32_t cyclic = 0;
            for (const gs_static_source &q : srcs) cyclic += q.kind == GS_STATIC_CYCLE;
            if (cyclic != periods.size()) { napi_throw_type_error(env, nullptr, "proveGenericSerialized: staticPeriods must list exactly the cyclic static registers"); return nullptr; }
            a.static_sources = srcs.data();
            a.nstatic = (uint32_t)srcs.size();
        }
        a.public_inputs = pub; a.public_input_counts = pub_counts.empty() ? nullptr : pub_counts.data(); a.npublic_inputs = (uint32_t)pub_counts.size();
    }
    job.root_of_unity_log2 = (uint32_t)root_log2;
    napi_value arr = prop("assertions");
    uint32_t na = 0;
    NAPI_OK(env, napi_get_array_length(env, arr, &na));
    std::vector<gs_assertion> as(na);
    for (uint32_t i = 0; i < na; i++) {
        napi_value e, v;
        NAPI_OK(env, napi_get_element(env, arr, i, &e));
        uint64_t step, reg;
        const uint8_t *val; size_t nval;
        napi_get_named_property(env, e, "step", &v);
        bool ok = get_u64(env, v, &step);
        napi_get_named_property(env, e, "register", &v);
        ok = ok && get_u64(env, v, &reg);
        napi_get_named_property(env, e, "value", &v);
        ok = ok && bytes(v, &val, &nval) && nval == es;
        if (!ok) { napi_throw_type_error(env, nullptr, "proveGenericSerialized: malformed assertion"); return nullptr; }
        as[i].step = step; as[i].reg = (uint32_t)reg; memcpy(as[i].value, val, es);
    }
    job.assertions = as.data(); job.nassertions = na;
    if (diagnose) return diagnosis_of(env, drv, job, ctx, es);
    if (argc >= 4) return verify_instead(env, drv, argv[3], job, ctx, argc >= 5 ? argv[4] : nullptr);
    static thread_local std::vector<uint8_t> out;      // (kept between calls: a fresh vector of this size is 4 MB of zeroing per proof)
    if (out.size() < (1u << 22)) out.resize(1u << 22);
    uint64_t n = 0;
    char err[512] = {0};
    int rcode = ((prove_on_fn)dlsym(drv->dl, "gs_prover_prove_on"))(drv->binding, (gs_ctx *)ctx, &job, out.data(), out.size(), &n, err, sizeof err);
    if (rcode != GS_OK) { napi_throw_error(env, nullptr, (std::string("native prove() failed: ") + err).c_str()); return nullptr; }
    napi_value buf;
    NAPI_OK(env, napi_create_buffer_copy(env, (size_t)n, out.data(), nullptr, &buf));
    return buf;
}

// packElements(values: BigInt[], elementSize) -> Buffer of their little-endian elements (values must be non-negative and fit: the caller
// reduces them), unpackElements(buffer, elementSize) -> BigInt[].  A column of an input register is 10^4..10^5 elements per proof; in
// JavaScript a BigInt costs 0.5-2 us to take apart or put together, here a copy of its words.
napi_value PackElements(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    bool is_array = false;
    uint32_t es = 0, n = 0;
    if (argc < 2 || napi_is_array(env, argv[0], &is_array) != napi_ok || !is_array || napi_get_value_uint32(env, argv[1], &es) != napi_ok ||
        (es != 16 && es != 32)) {
        napi_throw_type_error(env, nullptr, "packElements(values: BigInt[], elementSize: 16 | 32)");
        return nullptr;
    }
    NAPI_OK(env, napi_get_array_length(env, argv[0], &n));
    void *data = nullptr;
    napi_value buf;
    NAPI_OK(env, napi_create_buffer(env, (size_t)n * es, &data, &buf));
    uint8_t *out = (uint8_t *)data;
    const size_t max_words = es / 8;
    for (uint32_t i = 0; i < n; i++) {
        napi_value v;
        NAPI_OK(env, napi_get_element(env, argv[0], i, &v));
        uint64_t words[4] = {0, 0, 0, 0};
        size_t count = max_words;
        int sign = 0;
        if (napi_get_value_bigint_words(env, v, &sign, &count, words) != napi_ok) {
            napi_throw_type_error(env, nullptr, "packElements: every value must be a BigInt");
            return nullptr;
        }
        // (count comes back as the number of words the value NEEDS: more than the element holds means it does not fit)
        if (sign || count > max_words) {
            napi_throw_range_error(env, nullptr, "packElements: a value is negative or wider than the element");
            return nullptr;
        }
        memcpy(out + (size_t)i * es, words, es);
    }
    return buf;
}
napi_value UnpackElements(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    bool is_buffer = false;
    uint32_t es = 0;
    if (argc < 2 || napi_is_buffer(env, argv[0], &is_buffer) != napi_ok || !is_buffer || napi_get_value_uint32(env, argv[1], &es) != napi_ok ||
        (es != 16 && es != 32)) {
        napi_throw_type_error(env, nullptr, "unpackElements(buffer: Buffer, elementSize: 16 | 32)");
        return nullptr;
    }
    void *data = nullptr;
    size_t len = 0;
    NAPI_OK(env, napi_get_buffer_info(env, argv[0], &data, &len));
    if (len % es) { napi_throw_range_error(env, nullptr, "unpackElements: the buffer is not a whole number of elements"); return nullptr; }
    const size_t n = len / es;
    napi_value arr;
    NAPI_OK(env, napi_create_array_with_length(env, n, &arr));
    for (size_t i = 0; i < n; i++) {
        uint64_t words[4];
        memcpy(words, (const uint8_t *)data + i * es, es);
        napi_value v;
        NAPI_OK(env, napi_create_bigint_words(env, 0, es / 8, words, &v));
        NAPI_OK(env, napi_set_element(env, arr, (uint32_t)i, v));
    }
    return arr;
}

// modulus getter of a library object: the library's modulus as little-endian bytes (a runtime-modulus library's after gs_set_modulus)
napi_value LibModulus(napi_env env, napi_callback_info info) {
    napi_value info_obj = FieldInfo(env, info), v;
    if (!info_obj) return nullptr;
    NAPI_OK(env, napi_get_named_property(env, info_obj, "modulus", &v));
    return v;
}

// open(path) -> a library object: { backend, elementSize, modulus (getter: Buffer), fieldInfo(), ctxCreate(), ctxDestroy(), alloc(),
// call(), merkleProveBatch(), proveMimcSerialized(), proveGenericSerialized() } — the module's members, on THIS library (a library
// object's members refuse contexts another library created).  Several can be open at once: one per field flavour.
napi_value Open(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    if (argc < 1) { napi_throw_type_error(env, nullptr, "open(path)"); return nullptr; }
    Lib *L = open_lib(env, argv[0], "open(path)");
    if (!L) return nullptr;
    napi_value backend, es;
    NAPI_OK(env, napi_create_string_utf8(env, L->backend.c_str(), NAPI_AUTO_LENGTH, &backend));
    NAPI_OK(env, napi_create_uint32(env, (uint32_t)L->es, &es));
    const napi_property_descriptor props[] = {
        {"backend", nullptr, nullptr, nullptr, nullptr, backend, napi_enumerable, nullptr},
        {"elementSize", nullptr, nullptr, nullptr, nullptr, es, napi_enumerable, nullptr},
        {"modulus", nullptr, nullptr, LibModulus, nullptr, nullptr, napi_enumerable, L},
        {"fieldInfo", nullptr, FieldInfo, nullptr, nullptr, nullptr, napi_default, L},
        {"ctxCreate", nullptr, CtxCreate, nullptr, nullptr, nullptr, napi_default, L},
        {"ctxDestroy", nullptr, CtxDestroy, nullptr, nullptr, nullptr, napi_default, L},
        {"alloc", nullptr, Alloc, nullptr, nullptr, nullptr, napi_default, L},
        {"call", nullptr, Call, nullptr, nullptr, nullptr, napi_default, L},
        {"has", nullptr, Has, nullptr, nullptr, nullptr, napi_default, L},
        {"merkleProveBatch", nullptr, MerkleProveBatch, nullptr, nullptr, nullptr, napi_default, L},
        {"proveMimcSerialized", nullptr, ProveMimcSerialized, nullptr, nullptr, nullptr, napi_default, L},
        {"proveGenericSerialized", nullptr, ProveGenericSerialized, nullptr, nullptr, nullptr, napi_default, L},
        {"diagnoseGenericSerialized", nullptr, DiagnoseGenericSerialized, nullptr, nullptr, nullptr, napi_default, L},
    };
    napi_value out;
    NAPI_OK(env, napi_create_object(env, &out));
    NAPI_OK(env, napi_define_properties(env, out, sizeof props / sizeof props[0], props));
    return out;
}

napi_value Init(napi_env env, napi_value exports) {
    const struct { const char *name; napi_callback cb; } fns[] = {
        {"load", Load}, {"open", Open}, {"fieldInfo", FieldInfo}, {"ctxCreate", CtxCreate}, {"ctxDestroy", CtxDestroy}, {"alloc", Alloc}, {"call", Call}, {"has", Has},
        {"merkleProveBatch", MerkleProveBatch}, {"proveMimcSerialized", ProveMimcSerialized}, {"proveGenericSerialized", ProveGenericSerialized}, {"diagnoseGenericSerialized", DiagnoseGenericSerialized},
        {"packElements", PackElements}, {"unpackElements", UnpackElements},
    };
    for (auto &f : fns) {
        napi_value fn;
        if (napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.cb, nullptr, &fn) != napi_ok) return nullptr;
        if (napi_set_named_property(env, exports, f.name, fn) != napi_ok) return nullptr;
    }
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
