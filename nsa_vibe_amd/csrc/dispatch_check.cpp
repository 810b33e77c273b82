// Host check of the C ABI's dispatch layer (tests/test_dispatch_host.py runs it; no GPU).  A plain host program that loads the library and
// answers the HIP calls of its host code itself: hipMalloc comes from the heap, the memsets fill host memory, and hipLaunchKernel is counted
// and refused -- no kernel runs.  A refused launch comes back through the entry point as "HIP error ... in <launcher> launch", so calling an
// entry point again and again with the refusal moved one launch further walks its whole route: every case prints the launchers in order,
// each launch's grid / block / LDS bytes, the host memsets, and the status and nsa_hip_last_error() of the complete call.
//   dispatch_check <path of libnsa_sel_hip.so>      prints one JSON object, a member per case
//   dispatch_check <library> ragged | layer_ragged  the cases of the entry points with per-sequence positions instead
//   dispatch_check <library> paged                  the cases of the ragged decode step over paged caches (nsa_sel_decode_paged)
//   dispatch_check <library> band_paged             the cases of the ragged band forward over paged caches (nsa_band_attn_fwd_paged)
//   dispatch_check <library> layer_paged            the cases of the layer's paged call (nsa_layer_decode_paged)
//   dispatch_check <library> decode_long            the four ragged / paged entry points beyond the unsplit forms (switch DECODE_LONG)
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/nsa_sel_hip.h"
#include "layer_fused.hpp"
#include "sel_attn_params.hpp"
#include "sel_scores_params.hpp"

// ---- the HIP runtime as this program answers it ------------------------------------------------
static const hipError_t REFUSED = hipErrorNotSupported;
static int g_refuse_at = -1;  // index of the launch that is refused (-1: none)
static int g_launches = 0, g_memsets = 0;
static hipError_t g_last = hipSuccess;
static std::vector<std::string> g_geom;
struct Peek {  // copy `bytes` of kernel argument `arg` of launch `launch` (an argument block or a scalar passed by value)
    int launch, arg;
    std::vector<unsigned char> bytes;
};
static std::vector<Peek> g_peeks;
struct Config {
    dim3 grid, block;
    size_t shmem;
    hipStream_t stream;
};
static std::vector<Config> g_config;
static std::function<void(int, const void *, void **)> g_on_launch;  // when set: sees every launch (index, host function, arguments)

extern "C" {
__attribute__((visibility("default"))) hipError_t hipMalloc(void **p, size_t n) {
    *p = aligned_alloc(256, (n + 255) & ~(size_t)255);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
__attribute__((visibility("default"))) hipError_t hipFree(void *p) {
    free(p);
    return hipSuccess;
}
__attribute__((visibility("default"))) hipError_t hipMemsetAsync(void *dst, int value, size_t n, hipStream_t) {
    ++g_memsets;
    memset(dst, value, n);
    return hipSuccess;
}
__attribute__((visibility("default"))) hipError_t hipMemsetD32Async(hipDeviceptr_t dst, int value, size_t count, hipStream_t) {
    ++g_memsets;
    for (size_t i = 0; i < count; ++i) ((int *)dst)[i] = value;
    return hipSuccess;
}
__attribute__((visibility("default"))) hipError_t hipGetLastError(void) {
    const hipError_t e = g_last;
    g_last = hipSuccess;
    return e;
}
__attribute__((visibility("default"))) const char *hipGetErrorString(hipError_t e) { return e == REFUSED ? "launch refused" : "other"; }
__attribute__((visibility("default"))) hipError_t hipGetDevice(int *dev) {
    *dev = 0;
    return hipSuccess;
}
__attribute__((visibility("default"))) hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) {
    *v = 256;  // compute units of the MI355X (the only attribute the library asks for)
    return hipSuccess;
}
__attribute__((visibility("default"))) hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
__attribute__((visibility("default"))) hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
    g_config.push_back({grid, block, shmem, stream});
    return hipSuccess;
}
__attribute__((visibility("default"))) hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *shmem, hipStream_t *stream) {
    const Config c = g_config.back();
    g_config.pop_back();
    *grid = c.grid; *block = c.block; *shmem = c.shmem; *stream = c.stream;
    return hipSuccess;
}
__attribute__((visibility("default"))) hipError_t hipLaunchKernel(const void *fn, dim3 grid, dim3 block, void **args, size_t shmem, hipStream_t) {
    const int i = g_launches++;
    char s[96];
    snprintf(s, sizeof(s), "%u,%u,%u/%u,%u,%u/%zu", grid.x, grid.y, grid.z, block.x, block.y, block.z, shmem);
    g_geom.push_back(s);
    for (Peek &p : g_peeks)
        if (p.launch == i) memcpy(p.bytes.data(), args[p.arg], p.bytes.size());
    if (g_on_launch) g_on_launch(i, fn, args);
    if (i == g_refuse_at) return g_last = REFUSED;
    return hipSuccess;
}
}  // extern "C"

// ---- the library --------------------------------------------------------------------------------
static void *g_lib;
#define NSA_FN(name) ((decltype(&name))sym(#name))
static void *sym(const char *name) {
    void *p = dlsym(g_lib, name);
    if (!p) {
        fprintf(stderr, "missing symbol %s\n", name);
        exit(2);
    }
    return p;
}

static void *dev(size_t bytes, int fill = 0) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) exit(2);
    memset(p, fill, bytes);
    return p;
}
static void *off(void *p, size_t bytes) { return (unsigned char *)p + bytes; }
static bool all_zero(const void *p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (((const unsigned char *)p)[i]) return false;
    return true;
}

static bool g_first = true;
static std::string quoted(const std::string &s) {
    std::string o = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') o += '\\';
        o += c;
    }
    return o + "\"";
}
static std::string list(const std::vector<std::string> &v) {
    std::string o = "[";
    for (size_t i = 0; i < v.size(); ++i) o += (i ? ", " : "") + quoted(v[i]);
    return o + "]";
}

// Walks the route of one call: refuses launch 0, 1, 2, ... until the call ends without a refused launch.  `after` may add fields
// ("key": value, ...) from what the complete call left behind.
static std::vector<std::string> g_names;  // the launchers of the call walked last
static void run(const char *label, const std::function<int()> &call, const std::function<std::string()> &after = nullptr) {
    auto last_error = NSA_FN(nsa_hip_last_error);
    std::vector<std::string> &names = g_names;
    names.clear();
    int rc = 0;
    std::string err;
    for (int n = 0; n < 64; ++n) {
        g_refuse_at = n;
        g_launches = g_memsets = 0;
        g_geom.clear();
        g_last = hipSuccess;
        rc = call();
        err = rc ? last_error() : "";
        const size_t in = err.find(" in ");
        if (rc == NSA_ERR_HIP && g_launches == n + 1 && in != std::string::npos) {
            names.push_back(err.substr(in + 4));
            continue;
        }
        break;
    }
    const std::string geometry = list(g_geom);
    const int memsets = g_memsets;
    const std::string more = after ? ", " + after() : "";  // (last: `after` may call the entry point again)
    printf("%s\n%s: {\"rc\": %d, \"error\": %s, \"launches\": %s, \"geometry\": %s, \"memsets\": %d%s}", g_first ? "" : ",", quoted(label).c_str(), rc,
           quoted(err).c_str(), list(names).c_str(), geometry.c_str(), memsets, more.c_str());
    g_first = false;
    g_peeks.clear();
}

template <class P>
static void peek(int launch, int arg = 0) {
    g_peeks.push_back({launch, arg, std::vector<unsigned char>(sizeof(P), 0)});
}
template <class P>
static P peeked(size_t i = 0) {
    P p;
    memcpy(&p, g_peeks[i].bytes.data(), sizeof(P));
    return p;
}
template <class P>
static std::string peeked_scale() {
    const P p = peeked<P>();
    char s[64];
    snprintf(s, sizeof(s), "\"scale\": %.9g", (double)p.scale);
    return s;
}

// ---- the argument blocks of the one-launch decode step (decode_step_kernel(DecStepParams, SelectParams, int, DecAttnArgs, DecBandPair)):
// every scalar member, and for a pointer the test buffer it points into and the offset -- what tells two swapped neighbours of a
// positional list apart where the launch geometry does not
struct Named {
    const char *name;
    const void *base;
    size_t bytes;
};
static std::vector<Named> g_named;
static std::string where(const void *p) {
    if (!p) return "null";
    for (const Named &b : g_named)
        if ((const unsigned char *)p >= (const unsigned char *)b.base && (const unsigned char *)p < (const unsigned char *)b.base + b.bytes)
            return std::string(b.name) + "+" + std::to_string((const unsigned char *)p - (const unsigned char *)b.base);
    return "other";
}
// walks `call` like run(), then calls it once more to copy the blocks of its decode_step / decode_rows launch ("step": null without one)
static void run_step(const char *label, const std::function<int()> &call) {
    run(label, call, [&] {
        int at = -1;
        for (size_t i = 0; i < g_names.size(); ++i)
            if (g_names[i] == "decode_step launch" || g_names[i] == "decode_rows launch") at = (int)i;
        if (at < 0) return std::string("\"step\": null");
        peek<nsa::DecStepParams>(at);
        peek<nsa::DecAttnArgs>(at, 3);
        g_refuse_at = -1;
        g_launches = 0;
        call();
        const nsa::DecStepParams P = peeked<nsa::DecStepParams>(0);
        const nsa::DecAttnArgs A = peeked<nsa::DecAttnArgs>(1);
        char s[1024];
        snprintf(s, sizeof(s),
                 "\"step\": {\"Q\": \"%s\", \"Kc\": \"%s\", \"part_g\": \"%s\", \"halo_g\": \"%s\", \"pg_g\": \"%s\", \"cnt\": \"%s\", \"R\": %d, \"G\": %d, "
                 "\"h\": %d, \"S_cmp\": %d, \"S_sel\": %d, \"NS\": %d, \"nchunk\": %d, \"cpg\": %d, \"t_token\": %d, \"spin\": %d, \"csb\": %lld, \"csg\": %lld, "
                 "\"css\": %lld, \"c2\": %.9g, \"S\": %d}, \"attn\": {\"Q\": \"%s\", \"K\": \"%s\", \"V\": \"%s\", \"O\": \"%s\", \"G\": %d, \"h\": %d, "
                 "\"S_kv\": %d, \"n\": %d, \"ksb\": %lld, \"ksg\": %lld, \"kss\": %lld, \"vsb\": %lld, \"vsg\": %lld, \"vss\": %lld, \"c2\": %.9g}",
                 where(P.Q).c_str(), where(P.Kc).c_str(), where(P.part_g).c_str(), where(P.halo_g).c_str(), where(P.pg_g).c_str(), where(P.cnt).c_str(), P.R,
                 P.G, P.h, P.S_cmp, P.S_sel, P.NS, P.nchunk, P.cpg, P.t_token, P.spin, (long long)P.csb, (long long)P.csg, (long long)P.css, (double)P.c2,
                 P.S, where(A.Q).c_str(), where(A.K).c_str(), where(A.V).c_str(), where(A.O).c_str(), A.G, A.h, A.S_kv, A.n, (long long)A.ksb,
                 (long long)A.ksg, (long long)A.kss, (long long)A.vsb, (long long)A.vsg, (long long)A.vss, (double)A.c2);
        return std::string(s);
    });
}

// ---- the argument blocks of the scorer and selector family (sel_scores_params.hpp), member by member
struct Obj {
    std::string s;
    Obj &raw(const char *k, const std::string &v) {
        s += (s.empty() ? "\"" : ", \"") + std::string(k) + "\": " + v;
        return *this;
    }
    Obj &i(const char *k, long long v) { return raw(k, std::to_string(v)); }
    Obj &f(const char *k, double v) {
        char b[40];
        snprintf(b, sizeof(b), "%.9g", v);
        return raw(k, b);
    }
    Obj &p(const char *k, const void *v) { return raw(k, quoted(where(v))); }
    std::string str() const { return "{" + s + "}"; }
};
#define M_I(m) i(#m, P.m)
#define M_P(m) p(#m, P.m)
static std::string show(const nsa::PcmpParams &P) {
    return Obj().M_P(Q).M_P(Kc).M_P(p_cmp).M_I(row0).M_I(nrows).M_I(S).M_I(G).M_I(h).M_I(Dk).M_I(S_cmp).M_I(csb).M_I(csg).M_I(css).f("scale", P.scale)
        .M_I(q0).M_I(norm).M_I(l).M_I(d).str();
}
static std::string show(const nsa::MapParams &P) {
    return Obj().M_P(p_cmp).M_P(csc_ptr).M_P(csc_rows).M_P(csc_vals).M_P(p_slc).M_P(p_grp).M_I(R).M_I(h).M_I(S_cmp_cur).M_I(S_sel).str();
}
static std::string show(const nsa::DecodeParams &P) {
    return Obj().M_P(Q).M_P(Kc).M_P(x).M_P(part).M_P(p_grp).M_P(csc_ptr).M_P(csc_rows).M_P(csc_vals).M_I(R).M_I(S).M_I(G).M_I(h).M_I(Dk).M_I(S_cmp)
        .M_I(S_sel).M_I(csb).M_I(csg).M_I(css).f("c2", P.c2).M_I(stencil).M_I(q0).M_I(norm).M_I(l).M_I(d).str();
}
static std::string show(const nsa::ScoresMfmaParams &P) {
    return Obj().M_P(Q).M_P(Kc).M_P(p_grp).M_I(B).M_I(S).M_I(G).M_I(h).M_I(S_cmp).M_I(S_sel).M_I(csb).M_I(csg).M_I(css).f("scale", P.scale)
        .M_I(causal_skip).M_I(d_stride).M_I(big_out).M_I(q0).M_I(norm).M_I(l).str();
}
static std::string show(const nsa::SelectParams &P) {
    return Obj().M_P(p_grp).M_P(t_rows).M_P(out).M_I(R).M_I(S).M_I(G).M_I(t0).M_I(S_sel).M_I(l_sel).M_I(n_top).M_I(force_init).M_I(force_local).M_I(mode)
        .M_I(W).M_I(k_actual).M_I(n_forced).M_I(keepmask).M_I(all_valid).M_I(l_sel_shift).M_I(forced_plain).str();
}
static std::string show(const int &v) { return std::to_string(v); }
// ---- the argument blocks of the attention family (sel_attn_params.hpp), member by member.  `select` points at the launcher's caller's own
// SelectParams (host memory): "set" or "null"; the copy the kernel takes is argument 1 of the launch
static std::string show(const nsa::SelAttnParams &P) {
    return Obj().M_P(Q).M_P(K).M_P(V).M_P(ranges).M_P(O).M_P(lse).M_I(R).M_I(S).M_I(G).M_I(h).M_I(Dk).M_I(Dv).M_I(S_kv).M_I(n).M_I(ksb).M_I(ksg).M_I(kss)
        .M_I(vsb).M_I(vsg).M_I(vss).f("scale", P.scale).M_P(part).M_I(nsplit).M_I(map_mode).M_I(defer_combine).M_I(fuse_select)
        .raw("select", P.select ? "\"set\"" : "\"null\"").M_I(tpw).M_I(nw).M_I(wave_lds).M_P(ks_ws).M_I(ks_bytes).M_I(ks_r1).M_I(ks_r2).M_I(ks_w1).M_I(ks_w2)
        .M_I(ks_wa).M_I(ks_wb).M_I(ks_wc).str();
}
static std::string show(const nsa::SelAttnBwdParams &P) {
    return Obj().M_P(Q).M_P(K).M_P(V).M_P(ranges).M_P(O).M_P(lse).M_P(dO).M_P(dQ).M_P(dK).M_P(dV).M_I(R).M_I(S).M_I(G).M_I(h).M_I(Dk).M_I(Dv).M_I(S_kv).M_I(n)
        .M_I(ksb).M_I(ksg).M_I(kss).M_I(vsb).M_I(vsg).M_I(vss).f("scale", P.scale).M_I(skip_delta_dq).str();
}
static std::string show(const nsa::BandAttnParams &P) {
    return Obj().M_P(Q).M_P(K).M_P(V).M_P(O).M_P(lse).M_I(B).M_I(S).M_I(G).M_I(h).M_I(Dk).M_I(Dv).M_I(S_kv).M_I(ksb).M_I(ksg).M_I(kss).M_I(vsb).M_I(vsg).M_I(vss)
        .f("scale", P.scale).M_I(t0).M_I(a).M_I(dd).M_I(c).M_I(w).M_P(part).M_I(nsplit).M_I(map_mode).M_I(tpw).M_I(defer_combine).str();
}
static std::string show(const nsa::DecAttnArgs &P) {
    return Obj().M_P(Q).M_P(K).M_P(V).M_P(O).M_I(G).M_I(h).M_I(S_kv).M_I(n).M_I(ksb).M_I(ksg).M_I(kss).M_I(vsb).M_I(vsg).M_I(vss).f("c2", P.c2).str();
}
static std::string show(const nsa::DecBandPair &P) {
    return Obj().raw("w", show(P.w)).raw("c", show(P.c)).i("mg_on", P.mg.on).p("gates", P.mg.gates).i("n_sel", P.n_sel).i("n_w", P.n_w).str();
}
// nsa_band_attn_fwd_paged: the table block, argument 1 of the paged band kernels
static std::string show(const nsa::BandPageTable &P) { return Obj().p("table", P.table).i("stride", P.stride).i("n_pages", P.n_pages).i("shift", P.shift).str(); }
struct BandBwdExtraArg {  // band_attn_mfma.hip: BandBwdExtra, argument 1 of the band dQ kernel
    const void *dO, *lse, *delta, *dQ;
};
static std::string show(const BandBwdExtraArg &P) { return Obj().M_P(dO).M_P(lse).M_P(delta).M_P(dQ).str(); }
struct PtrArg {  // a pointer passed by value
    const void *p;
};
static std::string show(const PtrArg &v) { return quoted(where(v.p)); }
static std::string show(const int64_t &v) { return std::to_string(v); }
static std::string show(const unsigned &v) { return std::to_string(v); }
#undef M_I
#undef M_P

// one kernel argument of every launch of `launcher` (as nsa_hip_last_error() names it): its index, its size and how to print it
struct Want {
    std::string launcher;
    int arg;
    size_t bytes;
    const char *key;
    std::function<std::string(const void *)> print;
};
template <class P>
static Want want(const char *launcher, const char *key, int arg = 0) {
    return {std::string(launcher) + " launch", arg, sizeof(P), key, [](const void *b) {
                P p;
                memcpy(&p, b, sizeof(P));
                return show(p);
            }};
}
// walks `call` like run(), then calls it once more and prints the wanted arguments of its launches, in launch order:
// "args": [{"launch": index, "<key>": value, ...}, ...]
static void run_args(const std::string &label, const std::function<int()> &call, const std::vector<Want> &wants) {
    run(label.c_str(), call, [&] {
        std::vector<const Want *> of;
        for (size_t i = 0; i < g_names.size(); ++i)
            for (const Want &w : wants)
                if (w.launcher == g_names[i]) {
                    g_peeks.push_back({(int)i, w.arg, std::vector<unsigned char>(w.bytes, 0)});
                    of.push_back(&w);
                }
        g_refuse_at = -1;
        g_launches = 0;
        call();
        std::string o = "\"args\": [";
        for (size_t k = 0; k < g_peeks.size(); ++k) {
            const bool first = k == 0 || g_peeks[k].launch != g_peeks[k - 1].launch;
            if (first) o += std::string(k ? "}, " : "") + "{\"launch\": " + std::to_string(g_peeks[k].launch);
            o += ", " + quoted(of[k]->key) + ": " + of[k]->print(g_peeks[k].bytes.data());
        }
        return o + (g_peeks.empty() ? "]" : "}]");
    });
}

// ---- the few-row projection family (layer_fused.hip: the launchers linear_small* and qkv_rope_append*).  walks `call` like run(), then calls
// it once more and prints, for every launch of the family, what tells its route:
//   "kernel": the ordinal of the launched host function among the family's functions seen so far -- two launches share a template instance
//             (all-loads-first chunks NC, weight rows per wave, 4 or 8 MFMA waves) exactly when they share an ordinal;
//   the operand the launch reads and whether norm weights ride along, M, N, K, and the epilogue's or the mix's operands.
// The VALU kernels take (A policy, W, M, N, K, epilogue policy), the MFMA kernel (RopeAppendParams, X, W, out, M, N, K, epi, res, mix).
// "linear_small_mix" names a launch of either: the weights are argument 1 of the VALU kernels and argument 2 of the MFMA kernel.
static std::vector<const void *> g_kernels;
static void run_proj(const std::string &label, const std::function<int()> &call) {
    struct RowsArg { const void *A, *norm_w; float eps; };
    struct MixArg { const void *Oc, *Os, *Ow, *gates; int G; };
    struct EpiArg { const void *out, *res; int epi, N; };
    struct MfmaMixArg { const void *Os, *Ow, *gates; int G; };
    run(label.c_str(), call, [&] {
        std::string o;
        g_on_launch = [&](int i, const void *fn, void **a) {
            auto get = [&](int k, auto v) {
                memcpy(&v, a[k], sizeof(v));
                return v;
            };
            const std::string name = i < (int)g_names.size() ? g_names[i] : "";
            const bool qkv = name.rfind("qkv_rope_append", 0) == 0, mix = name == "linear_small_mix launch";
            if (!qkv && name.rfind("linear_small", 0) != 0) return;
            size_t ord = 0;
            while (ord < g_kernels.size() && g_kernels[ord] != fn) ++ord;
            if (ord == g_kernels.size()) g_kernels.push_back(fn);
            const bool mfma = name.find("mfma") != std::string::npos || (mix && where(get(1, (const void *)nullptr)).rfind("W_", 0) != 0);
            Obj e;
            e.i("launch", i).i("kernel", (long long)ord);
            const int m0 = mfma ? 4 : 2;  // M, N, K
            if (mfma) {
                const MfmaMixArg x = get(9, MfmaMixArg{});
                e.p("A", get(1, (const void *)nullptr)).p("norm_w", nullptr).p("W", get(2, (const void *)nullptr));
                if (mix) e.p("Os", x.Os).p("Ow", x.Ow).p("gates", x.gates).i("G", x.G);
            } else if (mix) {
                const MixArg x = get(0, MixArg{});
                e.p("A", x.Oc).p("norm_w", nullptr).p("W", get(1, (const void *)nullptr)).p("Os", x.Os).p("Ow", x.Ow).p("gates", x.gates).i("G", x.G);
            } else {
                const RowsArg x = get(0, RowsArg{});
                e.p("A", x.A).p("norm_w", x.norm_w).p("W", get(1, (const void *)nullptr));
                if (x.norm_w) e.f("eps", x.eps);
            }
            e.i("M", get(m0, 0)).i("N", get(m0 + 1, 0)).i("K", get(m0 + 2, 0));
            if (qkv) {
                const nsa::RopeAppendParams P = get(mfma ? 0 : 5, nsa::RopeAppendParams{});
                e.p("proj", P.proj).p("Q_out", P.Q_out).i("B", P.B).i("S", P.S).i("t0", P.t0);
            } else if (mfma) {
                e.p("out", get(3, (const void *)nullptr)).i("epi", get(7, 0)).p("res", get(8, (const void *)nullptr));
            } else {
                const EpiArg x = get(5, EpiArg{});
                e.p("out", x.out).i("epi", x.epi).p("res", x.res);
            }
            o += (o.empty() ? "" : ", ") + e.str();
        };
        g_refuse_at = -1;
        g_launches = 0;
        call();
        g_on_launch = nullptr;
        return "\"proj\": [" + o + "]";
    });
}

// ---- the tail of a layer decode call (step, rows, ragged, paged): calls `call` once more, every launch let through, and returns the members
// "finish" (DecodeFinishParams of the decode_finish launch), "gate" (GateCombineParams of the gate_combine launch) and "out" (the output
// projection: the last launch of the linear_small family, read as run_proj reads it), each null without its launch.  The launchers' names
// are those of the walk before it (g_names), so it goes behind a run() of the same call or into its `after`.
static std::string tail_fields(const std::function<int()> &call) {
    struct RowsArg { const void *A, *norm_w; float eps; };
    struct MixArg { const void *Oc, *Os, *Ow, *gates; int G; };
    struct EpiArg { const void *out, *res; int epi, N; };
    struct MfmaMixArg { const void *Os, *Ow, *gates; int G; };
    std::string fin = "null", gate = "null", out = "null";
    g_on_launch = [&](int i, const void *, void **a) {
        auto get = [&](int k, auto v) {
            memcpy(&v, a[k], sizeof(v));
            return v;
        };
        const std::string name = i < (int)g_names.size() ? g_names[i] : "";
        if (name == "decode_finish launch") {
            const nsa::DecodeFinishParams P = get(0, nsa::DecodeFinishParams{});
            Obj o;
            o.raw("ns", "[" + std::to_string(P.ns[0]) + ", " + std::to_string(P.ns[1]) + ", " + std::to_string(P.ns[2]) + "]");
            o.raw("part", list({where(P.part[0]), where(P.part[1]), where(P.part[2])})).raw("O", list({where(P.O[0]), where(P.O[1]), where(P.O[2])}));
            fin = o.i("R", P.R).p("Q", P.Q).p("O_out", P.O_out).p("gates_out", P.gates_out).p("w1", P.w1).p("b1", P.b1).p("w2", P.w2).p("b2", P.b2)
                      .i("h", P.h).i("Dk", P.Dk).i("Dv", P.Dv).i("Hd", P.Hd).f("tau", P.tau).str();
        } else if (name == "gate_combine launch") {
            const nsa::GateCombineParams P = get(0, nsa::GateCombineParams{});
            gate = Obj().raw("O", list({where(P.O_cmp), where(P.O_sel), where(P.O_win)})).i("R", P.R).p("Q", P.Q).p("O_out", P.O_out).p("gates_out", P.gates_out)
                       .p("w1", P.w1).p("b1", P.b1).p("w2", P.w2).p("b2", P.b2).i("h", P.h).i("Dk", P.Dk).i("Dv", P.Dv).i("Hd", P.Hd).f("tau", P.tau).str();
        } else if (name.rfind("linear_small", 0) == 0) {
            const bool mix = name == "linear_small_mix launch";
            const bool mfma = name.find("mfma") != std::string::npos || (mix && where(get(1, (const void *)nullptr)).rfind("W_", 0) != 0);
            Obj e;
            e.i("launch", i);
            const int m0 = mfma ? 4 : 2;  // M, N, K
            if (mfma) {
                const MfmaMixArg x = get(9, MfmaMixArg{});
                e.p("A", get(1, (const void *)nullptr)).p("W", get(2, (const void *)nullptr));
                if (mix) e.p("Os", x.Os).p("Ow", x.Ow).p("gates", x.gates).i("G", x.G);
                e.p("out", get(3, (const void *)nullptr)).i("epi", get(7, 0)).p("res", get(8, (const void *)nullptr));
            } else if (mix) {
                const MixArg x = get(0, MixArg{});
                const EpiArg y = get(5, EpiArg{});
                e.p("A", x.Oc).p("W", get(1, (const void *)nullptr)).p("Os", x.Os).p("Ow", x.Ow).p("gates", x.gates).i("G", x.G).p("out", y.out).i("epi", y.epi).p("res", y.res);
            } else {
                const RowsArg x = get(0, RowsArg{});
                const EpiArg y = get(5, EpiArg{});
                e.p("A", x.A).p("norm_w", x.norm_w).p("W", get(1, (const void *)nullptr)).p("out", y.out).i("epi", y.epi).p("res", y.res);
            }
            out = e.i("M", get(m0, 0)).i("N", get(m0 + 1, 0)).i("K", get(m0 + 2, 0)).str();
        }
    };
    g_refuse_at = -1;
    g_launches = 0;
    const int rc = call();
    g_on_launch = nullptr;
    return "\"tail_rc\": " + std::to_string(rc) + ", \"finish\": " + fin + ", \"gate\": " + gate + ", \"out\": " + out;
}

// ---- dispatch_check <library> ragged: the entry points with per-sequence positions (nsa_sel_decode_ragged, nsa_band_attn_fwd_ragged), cases
// of their own so that the default output keeps its cases and members.  The position array is a device pointer the host must never read: it
// is handed over as an address inside a named buffer and shows up again in the argument block of the launch.
// long_mode (dispatch_check <library> decode_long): not the cases below but the shapes beyond the unsplit forms, with the switch DECODE_LONG at 1
// (one launch in form 3), at the limit, past it, and with the switch back at 0 (the declines as they were)
static void ragged_cases(bool long_mode = false) {
    const int dt = NSA_DT_BF16, G = 2, h = 6, n = 16;
    const size_t MB = 1 << 20;
    void *Q = dev(MB), *K = dev(MB), *V = dev(MB), *Kc = dev(MB), *O = dev(MB), *ws = dev(16 * MB);
    float *lse = (float *)dev(MB), *csc_vals = (float *)dev(MB);
    int32_t *ranges = (int32_t *)dev(MB), *t_pos = (int32_t *)dev(MB, 0x7f), *csc_ptr = (int32_t *)dev(MB), *csc_rows = (int32_t *)dev(MB);
    g_named = {{"Q", Q, MB}, {"K", K, MB}, {"V", V, MB}, {"K_cmp", Kc, MB}, {"O", O, MB}, {"ranges", ranges, MB}, {"t_pos", t_pos, MB}, {"ws", ws, 16 * MB},
               {"lse", lse, MB}};
    auto ncmp = [](int t) { return t + 1 < 32 ? 0 : (t + 1 - 32) / 16 + 1; };
    auto ragged_fn = NSA_FN(nsa_sel_decode_ragged);
    auto plan_fn = NSA_FN(nsa_sel_decode_ragged_plan);
    struct Case {
        int B = 3, S = 1, D = 64, t_max = 100, dtype = NSA_DT_BF16;
        void *K = nullptr;
        const int32_t *t_pos = nullptr;
    };
    auto ragged_case = [&](const char *label, const std::function<void(Case &)> &tweak) {
        Case c;
        c.K = K;
        c.t_pos = t_pos + 5;
        tweak(c);
        const int S_kv = c.t_max + 1, S_cmp = ncmp(c.t_max), S_sel = (S_kv + 63) / 64;
        const int64_t ccg = (int64_t)S_cmp * c.D, ksg = (int64_t)S_kv * c.D;
        auto call = [&] {
            return ragged_fn(Q, Kc, c.K, V, csc_ptr, csc_rows, csc_vals, ranges, O, c.t_pos, c.t_max, c.B, c.S, G, h, c.D, c.D, S_cmp, S_sel, S_kv, 32, 16, 64, n, G * ccg,
                             ccg, c.D, G * ksg, ksg, c.D, G * ksg, ksg, c.D, c.dtype, 0.f, nullptr, 0, nullptr);
        };
        run((std::string("sel_decode_ragged/") + label).c_str(), call, [&] {
            int launches = -1, form = -2;
            const int prc = plan_fn(c.B, c.S, G, h, c.D, c.D, S_cmp, S_sel, S_kv, n, c.dtype, c.t_max, &launches, &form);
            std::string o = Obj().i("rc", prc).i("launches", launches).i("form", form).str();
            o = "\"plan\": " + o;
            int at = -1;
            for (size_t i = 0; i < g_names.size(); ++i)
                if (g_names[i] == "decode_step launch" || g_names[i] == "decode_rows launch") at = (int)i;
            if (at < 0) return o + ", \"step\": null";
            peek<nsa::DecStepParams>(at);
            g_refuse_at = -1;
            g_launches = 0;
            call();
            const nsa::DecStepParams P = peeked<nsa::DecStepParams>(0);
            return o + ", \"step\": " +
                   Obj().p("Q", P.Q).p("Kc", P.Kc).i("R", P.R).i("G", P.G).i("h", P.h).i("S_cmp", P.S_cmp).i("S_sel", P.S_sel).i("NS", P.NS).i("nchunk", P.nchunk)
                       .i("S", P.S).p("t_pos", P.t_pos).i("t_max", P.t_max).str();
        });
    };
    if (long_mode) {
        NSA_FN(nsa_hip_set_tuning)("DECODE_LONG", 1);
        ragged_case("long_D128_t_max20000", [](Case &c) { c.D = 128; c.t_max = 20000; });
        ragged_case("long_t_max70000", [](Case &c) { c.B = 1; c.t_max = 70000; });
        ragged_case("long_B200_t_max40000", [](Case &c) { c.B = 200; c.t_max = 40000; });
        ragged_case("long_t_max131071", [](Case &c) { c.B = 1; c.t_max = 131071; });
        ragged_case("long_D128_S4_t_max131071", [](Case &c) { c.D = 128; c.S = 4; c.t_max = 131071; });
        ragged_case("long_t_max131072_declined", [](Case &c) { c.B = 1; c.t_max = 131072; });
        ragged_case("long_t_max100_form0", [](Case &) {});
        ragged_case("long_t_max40000_form1", [](Case &c) { c.B = 1; c.t_max = 40000; });
        NSA_FN(nsa_hip_set_tuning)("DECODE_STEP", 0);
        ragged_case("long_DECODE_STEP_0_declined", [](Case &c) { c.B = 1; c.t_max = 70000; });
        NSA_FN(nsa_hip_set_tuning)("DECODE_STEP", 1);
        NSA_FN(nsa_hip_set_tuning)("DECODE_LONG", 0);
        ragged_case("off_D128_t_max20000_declined", [](Case &c) { c.D = 128; c.t_max = 20000; });
        ragged_case("off_t_max70000_declined", [](Case &c) { c.B = 1; c.t_max = 70000; });
        ragged_case("off_B200_t_max40000_declined", [](Case &c) { c.B = 200; c.t_max = 40000; });
        return;
    }
    ragged_case("t_max100", [](Case &) {});
    ragged_case("t_max100_S4", [](Case &c) { c.S = 4; });
    ragged_case("t_max20_no_compressed_token", [](Case &c) { c.t_max = 20; });
    ragged_case("t_max40000_form1", [](Case &c) { c.B = 1; c.t_max = 40000; });
    ragged_case("D128_t_max20000_declined", [](Case &c) { c.D = 128; c.t_max = 20000; });
    ragged_case("t_max70000_declined", [](Case &c) { c.B = 1; c.t_max = 70000; });
    ragged_case("B200_t_max40000_declined", [](Case &c) { c.B = 200; c.t_max = 40000; });
    ragged_case("f32_declined", [](Case &c) { c.dtype = NSA_DT_F32; });
    ragged_case("S17_declined", [](Case &c) { c.S = 17; });
    ragged_case("K_2_bytes_off", [&](Case &c) { c.K = off(K, 2); });
    ragged_case("null_t_pos", [](Case &c) { c.t_pos = nullptr; });
    NSA_FN(nsa_hip_set_tuning)("DECODE_STEP", 0);
    ragged_case("DECODE_STEP_0_declined", [](Case &) {});
    NSA_FN(nsa_hip_set_tuning)("DECODE_STEP", 1);
    NSA_FN(nsa_hip_set_tuning)("DECODE_ROWS", 0);  // the rows form's own switch does not apply
    ragged_case("DECODE_ROWS_0_still_one_launch", [](Case &) {});
    NSA_FN(nsa_hip_set_tuning)("DECODE_ROWS", -1);

    // the band call: launches and split count are the scalar call's (planned from the row count), the positions ride in the argument block
    auto band_fn = NSA_FN(nsa_band_attn_fwd_ragged);
    auto band_ws = NSA_FN(nsa_band_attn_fwd_ragged_workspace);
    const std::vector<Want> blocks = {want<nsa::BandAttnParams>("band_attn_fwd(split)", "BandAttnParams"), want<nsa::BandAttnParams>("band_attn_fwd", "BandAttnParams"),
                                      want<nsa::BandAttnParams>("band_attn_fwd_generic", "BandAttnParams")};
    auto band_case = [&](const char *label, int B, int S, int dtype, int t_max, bool compressed, bool with_ws) {
        const int D = 64, S_kv = compressed ? ncmp(t_max) : t_max + 1;
        const int64_t sg = (int64_t)S_kv * D;
        run_args(std::string("band_attn_fwd_ragged/") + label, [&] {
            return band_fn(Q, K, V, O, lse, t_pos + 5, t_max, B, S, G, h, D, D, S_kv, G * sg, sg, D, G * sg, sg, D, compressed ? 32 : 0, compressed ? 16 : 1,
                           compressed ? 1 : 0, compressed ? 1 << 30 : 512, dtype, 0.f, 0, with_ws ? ws : nullptr, with_ws ? 16 * MB : 0, nullptr);
        }, blocks);
        // (what show(BandAttnParams) leaves out: the ragged members, from the first launch)
        peek<nsa::BandAttnParams>(0);
        run((std::string("band_attn_fwd_ragged/") + label + "_positions").c_str(), [&] {
            return band_fn(Q, K, V, O, lse, t_pos + 5, t_max, B, S, G, h, D, D, S_kv, G * sg, sg, D, G * sg, sg, D, compressed ? 32 : 0, compressed ? 16 : 1,
                           compressed ? 1 : 0, compressed ? 1 << 30 : 512, dtype, 0.f, 0, with_ws ? ws : nullptr, with_ws ? 16 * MB : 0, nullptr);
        }, [&] {
            const nsa::BandAttnParams P = peeked<nsa::BandAttnParams>();
            return Obj().p("t_pos", P.t_pos).i("t_max", P.t_max).i("t0", P.t0).i("nsplit", P.nsplit).i("workspace", (long long)band_ws(B, S, G, h, D, D, dtype)).s;
        });
    };
    band_case("sliding_B5_S1_split", 5, 1, dt, 4100, false, true);
    band_case("sliding_B5_S1_no_workspace", 5, 1, dt, 4100, false, false);
    band_case("compressed_B5_S3_split", 5, 3, dt, 5002, true, true);
    band_case("sliding_B600_S3_unsplit", 600, 3, dt, 1000, false, true);
    band_case("sliding_f32_generic", 5, 1, NSA_DT_F32, 1000, false, true);
}

// ---- dispatch_check <library> paged: the ragged decode step over paged caches (nsa_sel_decode_paged), cases of their own like `ragged`.  The
// block table, like the position array, is a device pointer the host must never read: it is handed over as an address inside a named buffer
// filled with 0x7f bytes (no valid page id) and shows up again in the argument block of the launch, with its stride, n_pages and the
// three page strides.
static void paged_cases(bool long_mode = false) {  // long_mode: as ragged_cases
    const int G = 2, h = 6, n = 16;
    const size_t MB = 1 << 20;
    void *Q = dev(MB), *K = dev(MB), *V = dev(MB), *Kc = dev(MB), *O = dev(MB);
    float *csc_vals = (float *)dev(MB);
    int32_t *ranges = (int32_t *)dev(MB), *t_pos = (int32_t *)dev(MB, 0x7f), *table = (int32_t *)dev(MB, 0x7f), *csc_ptr = (int32_t *)dev(MB),
            *csc_rows = (int32_t *)dev(MB);
    g_named = {{"Q", Q, MB}, {"K_pool", K, MB}, {"V_pool", V, MB}, {"Kc_pool", Kc, MB}, {"O", O, MB}, {"ranges", ranges, MB}, {"t_pos", t_pos, MB},
               {"table", table, MB}};
    auto ncmp = [](int t) { return t + 1 < 32 ? 0 : (t + 1 - 32) / 16 + 1; };
    auto paged_fn = NSA_FN(nsa_sel_decode_paged);
    auto plan_fn = NSA_FN(nsa_sel_decode_paged_plan);
    struct Case {
        int B = 3, S = 1, D = 64, t_max = 100, dtype = NSA_DT_BF16, page_tokens = 1024, n_pages = 40, max_pages = 0 /* 0: what t_max needs */;
        int64_t table_stride = 0 /* 0: max_pages + 3 */, k_page_stride = 0 /* 0: G * 1024 * D */;
        void *K = nullptr;
        const int32_t *table = nullptr, *t_pos = nullptr;
    };
    auto paged_case = [&](const char *label, const std::function<void(Case &)> &tweak) {
        Case c;
        c.K = K;
        c.table = table + 7;
        c.t_pos = t_pos + 5;
        tweak(c);
        const int max_pages = c.max_pages ? c.max_pages : c.t_max / 1024 + 1;
        const int cap = max_pages * 1024, te = c.t_max < cap - 1 ? c.t_max : cap - 1;
        const int S_cmp = ncmp(te), S_sel = (te + 1 + 63) / 64;
        const int64_t tstride = c.table_stride ? c.table_stride : max_pages + 3;
        const int64_t kg = (int64_t)1024 * c.D, cg = (int64_t)64 * c.D, kp = c.k_page_stride ? c.k_page_stride : G * kg;
        auto call = [&] {
            return paged_fn(Q, Kc, c.K, V, c.table, tstride, c.n_pages, max_pages, c.page_tokens, csc_ptr, csc_rows, csc_vals, ranges, O, c.t_pos, c.t_max, c.B, c.S, G,
                            h, c.D, c.D, S_cmp, S_sel, 32, 16, 64, n, G * cg, cg, c.D, kp, kg, c.D, G * kg, kg, c.D, c.dtype, 0.f, nullptr, 0, nullptr);
        };
        run((std::string("sel_decode_paged/") + label).c_str(), call, [&] {
            int launches = -1, form = -2;
            const int prc = plan_fn(c.B, c.S, G, h, c.D, c.D, S_cmp, S_sel, max_pages, c.page_tokens, n, c.dtype, c.t_max, &launches, &form);
            std::string o = "\"plan\": " + Obj().i("rc", prc).i("launches", launches).i("form", form).str();
            int at = -1;
            for (size_t i = 0; i < g_names.size(); ++i)
                if (g_names[i] == "decode_paged launch") at = (int)i;
            if (at < 0) return o + ", \"step\": null";
            peek<nsa::DecStepParams>(at);
            peek<nsa::DecAttnArgs>(at, 3);
            g_refuse_at = -1;
            g_launches = 0;
            call();
            const nsa::DecStepParams P = peeked<nsa::DecStepParams>(0);
            const nsa::DecAttnArgs A = peeked<nsa::DecAttnArgs>(1);
            return o + ", \"step\": " +
                   Obj().p("Q", P.Q).p("Kc", P.Kc).i("R", P.R).i("G", P.G).i("h", P.h).i("S_cmp", P.S_cmp).i("S_sel", P.S_sel).i("NS", P.NS).i("nchunk", P.nchunk)
                       .i("S", P.S).p("t_pos", P.t_pos).i("t_max", P.t_max).p("block_table", P.block_table).i("bt_stride", P.bt_stride).i("n_pages", P.n_pages)
                       .i("kc_page_stride", P.csb).p("K", A.K).p("V", A.V).i("k_page_stride", A.ksb).i("v_page_stride", A.vsb).i("capacity", A.S_kv).str();
        });
    };
    if (long_mode) {
        NSA_FN(nsa_hip_set_tuning)("DECODE_LONG", 1);
        paged_case("long_D128_t_max20000", [](Case &c) { c.D = 128; c.t_max = 20000; });
        paged_case("long_t_max70000", [](Case &c) { c.B = 1; c.t_max = 70000; });
        paged_case("long_B200_t_max40000", [](Case &c) { c.B = 200; c.t_max = 40000; });
        paged_case("long_t_max131071", [](Case &c) { c.B = 1; c.t_max = 131071; });
        paged_case("long_t_max131071_max_pages4096", [](Case &c) { c.B = 1; c.t_max = 131071; c.max_pages = 4096; });
        paged_case("long_t_max131072_declined", [](Case &c) { c.B = 1; c.t_max = 131072; });
        paged_case("long_t_max100_form0", [](Case &) {});
        NSA_FN(nsa_hip_set_tuning)("DECODE_LONG", 0);
        paged_case("off_D128_t_max20000_declined", [](Case &c) { c.D = 128; c.t_max = 20000; });
        paged_case("off_t_max70000_declined", [](Case &c) { c.B = 1; c.t_max = 70000; });
        paged_case("off_B200_t_max40000_declined", [](Case &c) { c.B = 200; c.t_max = 40000; });
        return;
    }
    paged_case("t_max100", [](Case &) {});
    paged_case("t_max100_S4", [](Case &c) { c.S = 4; });
    paged_case("t_max20_no_compressed_token", [](Case &c) { c.t_max = 20; });
    paged_case("t_max5000_max_pages9", [](Case &c) { c.t_max = 5000; c.max_pages = 9; });
    paged_case("t_max40000_form1", [](Case &c) { c.B = 1; c.t_max = 40000; });
    paged_case("k_page_stride_3GiB", [](Case &c) { c.k_page_stride = (int64_t)3 << 29; });  // elements of 2 bytes: 3 GiB between pages
    paged_case("page_tokens64_declined", [](Case &c) { c.page_tokens = 64; });
    paged_case("null_table", [](Case &c) { c.table = nullptr; });
    paged_case("max_pages_minus1", [](Case &c) { c.max_pages = -1; });
    paged_case("n_pages0", [](Case &c) { c.n_pages = 0; });
    paged_case("table_stride_below_max_pages", [](Case &c) { c.t_max = 5000; c.table_stride = 4; });
    paged_case("D128_t_max20000_declined", [](Case &c) { c.D = 128; c.t_max = 20000; });
    paged_case("t_max70000_declined", [](Case &c) { c.B = 1; c.t_max = 70000; });
    paged_case("B200_t_max40000_declined", [](Case &c) { c.B = 200; c.t_max = 40000; });
    paged_case("f32_declined", [](Case &c) { c.dtype = NSA_DT_F32; });
    paged_case("S17_declined", [](Case &c) { c.S = 17; });
    paged_case("K_pool_2_bytes_off", [&](Case &c) { c.K = off(K, 2); });
    paged_case("k_page_stride_not_8", [](Case &c) { c.k_page_stride = (int64_t)2 * 1024 * 64 + 4; });
    paged_case("null_t_pos", [](Case &c) { c.t_pos = nullptr; });
    NSA_FN(nsa_hip_set_tuning)("DECODE_STEP", 0);
    paged_case("DECODE_STEP_0_declined", [](Case &) {});
    NSA_FN(nsa_hip_set_tuning)("DECODE_STEP", 1);

    // a row stride that puts a page's 1024 rows outside the 32-bit in-plane offsets (V rows must be contiguous, so it is K's): 2^20 elements
    // = 2 MiB a row, 2 GiB a plane
    {
        const int64_t kss = (int64_t)1 << 20, kg = 1024 * kss, cg = 64 * 64;
        run("sel_decode_paged/k_row_stride_2MiB", [&] {
            return paged_fn(Q, Kc, K, V, table + 7, 4, 40, 1, 1024, csc_ptr, csc_rows, csc_vals, ranges, O, t_pos + 5, 100, 3, 1, G, h, 64, 64, ncmp(100), 2, 32, 16, 64, n,
                            G * cg, cg, 64, G * kg, kg, kss, (int64_t)G * 1024 * 64, 1024 * 64, 64, NSA_DT_BF16, 0.f, nullptr, 0, nullptr);
        });
    }
}

// ---- dispatch_check <library> band_paged: the ragged band forward over paged caches (nsa_band_attn_fwd_paged), cases of their own like
// `ragged` and `paged`.  Every case prints the launches and their geometry, the two argument blocks of the band launch -- BandAttnParams
// (ksb / vsb: the page strides, S_kv: the capacity) and BandPageTable (the table pointer, its stride, n_pages, the page shift) -- as they
// arrive, the split count and the workspace query, or the decline with its message.  The table and the positions are device pointers the
// host must never read: addresses inside buffers of 0x7f bytes.
static void band_paged_cases() {
    const int G = 2, h = 6;
    const size_t MB = 1 << 20;
    void *Q = dev(MB), *K = dev(MB), *V = dev(MB), *O = dev(MB), *ws = dev(16 * MB);
    float *lse = (float *)dev(MB);
    int32_t *t_pos = (int32_t *)dev(MB, 0x7f), *table = (int32_t *)dev(MB, 0x7f);
    g_named = {{"Q", Q, MB}, {"K_pool", K, MB}, {"V_pool", V, MB}, {"O", O, MB}, {"lse", lse, MB}, {"t_pos", t_pos, MB}, {"table", table, MB}, {"ws", ws, 16 * MB}};
    auto fn = NSA_FN(nsa_band_attn_fwd_paged);
    auto ws_fn = NSA_FN(nsa_band_attn_fwd_paged_workspace);
    auto scalar_ws_fn = NSA_FN(nsa_band_attn_fwd_workspace);
    const std::vector<Want> blocks = {want<nsa::BandAttnParams>("band_attn_fwd(split)", "BandAttnParams"), want<nsa::BandPageTable>("band_attn_fwd(split)", "BandPageTable", 1),
                                      want<nsa::BandAttnParams>("band_attn_fwd", "BandAttnParams"), want<nsa::BandPageTable>("band_attn_fwd", "BandPageTable", 1)};
    struct Case {
        int B = 5, S = 1, D = 64, Dv = 0 /* 0: D */, hh = 6, t_max = 4100, dtype = NSA_DT_BF16, page_rows = 0 /* 0: 1024 sliding, 64 compressed */, n_pages = 40,
            max_pages = 0 /* 0: what t_max needs */, w = 0 /* 0: 512 sliding, 2^30 compressed */;
        bool compressed = false, with_ws = true;
        int64_t table_stride = 0 /* 0: max_pages + 3 */, k_page_stride = 0 /* 0: G * page_rows * D */, k_row_stride = 0 /* 0: D */;
        void *K = nullptr, *O = nullptr;
        const int32_t *table = nullptr, *t_pos = nullptr;
    };
    auto band_case = [&](const char *label, const std::function<void(Case &)> &tweak) {
        Case c;
        c.K = K, c.O = O, c.table = table + 7, c.t_pos = t_pos + 5;
        tweak(c);
        const int rows = c.page_rows ? c.page_rows : (c.compressed ? 64 : 1024);
        const int keys = c.compressed ? (c.t_max + 1 < 32 ? 0 : (c.t_max + 1 - 32) / 16 + 1) : c.t_max + 1;
        const int max_pages = c.max_pages ? c.max_pages : (keys + rows - 1) / rows + (keys == 0);
        const int64_t tstride = c.table_stride ? c.table_stride : max_pages + 3;
        const int64_t kss = c.k_row_stride ? c.k_row_stride : c.D, kg = (int64_t)rows * kss, kp = c.k_page_stride ? c.k_page_stride : G * kg;
        const int Dv = c.Dv ? c.Dv : c.D;
        const int64_t vg = (int64_t)rows * Dv;
        const int w = c.w ? c.w : (c.compressed ? 1 << 30 : 512);
        run_args(std::string("band_attn_fwd_paged/") + label, [&] {
            return fn(Q, c.K, V, c.table, tstride, c.n_pages, max_pages, rows, c.O, lse, c.t_pos, c.t_max, c.B, c.S, G, c.hh, c.D, Dv, kp, kg, kss, G * vg, vg, Dv,
                      c.compressed ? 32 : 0, c.compressed ? 16 : 1, c.compressed ? 1 : 0, w, c.dtype, 0.f, c.with_ws ? ws : nullptr, c.with_ws ? 16 * MB : 0, nullptr);
        }, blocks);
        // (what show(BandAttnParams) leaves out: the ragged members; and the workspace query beside the scalar call's)
        peek<nsa::BandAttnParams>(0);
        run((std::string("band_attn_fwd_paged/") + label + "_positions").c_str(), [&] {
            return fn(Q, c.K, V, c.table, tstride, c.n_pages, max_pages, rows, c.O, lse, c.t_pos, c.t_max, c.B, c.S, G, c.hh, c.D, Dv, kp, kg, kss, G * vg, vg, Dv,
                      c.compressed ? 32 : 0, c.compressed ? 16 : 1, c.compressed ? 1 : 0, w, c.dtype, 0.f, c.with_ws ? ws : nullptr, c.with_ws ? 16 * MB : 0, nullptr);
        }, [&] {
            const nsa::BandAttnParams P = peeked<nsa::BandAttnParams>();
            return Obj().p("t_pos", P.t_pos).i("t_max", P.t_max).i("t0", P.t0).i("nsplit", P.nsplit).i("workspace", (long long)ws_fn(c.B, c.S, G, c.hh, c.D, Dv, c.dtype))
                .i("scalar_workspace", (long long)scalar_ws_fn(c.B, c.S, G, c.hh, c.D, Dv, c.dtype)).s;
        });
    };
    (void)h;
    // the cases of the `ragged` mode's band calls at the same (B, S, G, h, D): launches and geometry must be theirs
    band_case("sliding_B5_S1_split", [](Case &) {});
    band_case("sliding_B5_S1_no_workspace", [](Case &c) { c.with_ws = false; });
    band_case("compressed_B5_S3_split", [](Case &c) { c.S = 3; c.t_max = 5002; c.compressed = true; });
    band_case("sliding_B600_S3_unsplit", [](Case &c) { c.B = 600; c.S = 3; c.t_max = 1000; });
    band_case("sliding_B600_S256_nt3", [](Case &c) { c.B = 600; c.S = 256; c.t_max = 1500; });
    band_case("sliding_D128_B5_S1_split", [](Case &c) { c.D = 128; });
    band_case("sliding_page_rows32", [](Case &c) { c.page_rows = 32; });
    band_case("sliding_page_rows65536", [](Case &c) { c.page_rows = 65536; });
    band_case("k_page_stride_3GiB", [](Case &c) { c.k_page_stride = (int64_t)3 << 29; });  // elements of 2 bytes: 3 GiB between pages
    band_case("max_pages_2pow20", [](Case &c) { c.max_pages = 1 << 20; c.table_stride = 1 << 20; });
    // the declines
    band_case("f32_declined", [](Case &c) { c.dtype = NSA_DT_F32; });
    band_case("Dk_ne_Dv_declined", [](Case &c) { c.Dv = 128; });
    band_case("D96_declined", [](Case &c) { c.D = 96; });
    band_case("h17_declined", [](Case &c) { c.hh = 17; });
    band_case("w_below_1_declined", [](Case &c) { c.w = -1; });
    band_case("null_table", [](Case &c) { c.table = nullptr; });
    band_case("null_t_pos", [](Case &c) { c.t_pos = nullptr; });
    band_case("max_pages_minus1", [](Case &c) { c.max_pages = -1; });
    band_case("max_pages_above_2pow20", [](Case &c) { c.max_pages = (1 << 20) + 1; c.table_stride = 1 << 21; });
    band_case("n_pages0", [](Case &c) { c.n_pages = 0; });
    band_case("table_stride_below_max_pages", [](Case &c) { c.table_stride = 4; });
    band_case("page_rows16_declined", [](Case &c) { c.page_rows = 16; });
    band_case("page_rows96_declined", [](Case &c) { c.page_rows = 96; });
    band_case("page_rows131072_declined", [](Case &c) { c.page_rows = 131072; });
    band_case("K_pool_2_bytes_off", [&](Case &c) { c.K = off(K, 2); });
    band_case("O_4_bytes_off", [&](Case &c) { c.O = off(O, 4); });
    band_case("k_page_stride_not_8", [](Case &c) { c.k_page_stride = (int64_t)2 * 1024 * 64 + 4; });
    band_case("k_row_stride_2MiB_plane_limit", [](Case &c) { c.k_row_stride = (int64_t)1 << 20; });  // 1024 rows of 2 MiB: a plane of 2 GiB
}

// ---- dispatch_check <library> layer_ragged: the layer's ragged call (nsa_layer_decode_ragged), cases of their own like `ragged`.  Every
// case prints the launchers in order with their geometry, the plan's answer for the same shape, and "positions": the position pointer and the
// bound te as they arrive in the argument blocks of the four launches that depend on the position (projection, pooling, the selected branch,
// the band pair: both of its blocks).
static void layer_ragged_cases(bool long_mode = false) {  // long_mode: the layer twins of ragged_cases' long shapes, beside an in-range plan
    const size_t MB = 1 << 20;
    void *x = dev(MB), *y = dev(MB), *W_qkv = dev(MB), *W_out = dev(MB), *gw = dev(MB), *ws = dev(64 * MB);
    void *cache[8];
    static const char *cname[8] = {"K_sel", "V_sel", "K_win", "V_win", "K_raw", "V_raw", "K_cmp", "V_cmp"};
    int32_t *t_pos = (int32_t *)dev(MB, 0x7f), *ranges = (int32_t *)dev(MB);
    float *gates = (float *)dev(MB);
    g_named = {{"x", x, MB}, {"y", y, MB}, {"W_qkv", W_qkv, MB}, {"W_out", W_out, MB}, {"t_pos", t_pos, MB}, {"ranges", ranges, MB}, {"gates", gates, MB},
               {"ws", ws, 64 * MB}};
    for (int i = 0; i < 8; ++i) {
        cache[i] = dev(MB);
        g_named.push_back({cname[i], cache[i], MB});
    }
    g_named.push_back({"gate_w", gw, MB});
    auto fn = NSA_FN(nsa_layer_decode_ragged);
    auto plan_fn = NSA_FN(nsa_layer_decode_ragged_plan);
    auto ws_fn = NSA_FN(nsa_layer_decode_ragged_workspace);
    struct Case {
        int B = 3, S = 8, D = 64, dim = 768, S_max = 1072, t_max = 1059, dtype = NSA_DT_BF16;
        const int32_t *t_pos = nullptr;
        bool with_ws = true;
        int K_cmp_off = 0, K_sel_off = 0, n_cmp_short = 0 /* 1: n_cmp_max one short of n_cmp(te + 1) */, S_sel_short = 0;
    };
    auto positions = [](const char *launcher, int arg, size_t bytes, const char *key, std::function<std::string(const void *)> print) {
        return Want{std::string(launcher) + " launch", arg, bytes, key, std::move(print)};
    };
    auto rope = [](const void *b) {
        nsa::RopeAppendParams P;
        memcpy(&P, b, sizeof(P));
        return Obj().p("t_pos", P.t_pos).i("t_max", P.t_max).i("t0", P.t0).i("B", P.B).i("S", P.S).i("S_max", P.S_max).p("Q_out", P.Q_out).str();
    };
    auto pool = [](const void *b) {
        nsa::CmpPoolParams P;
        memcpy(&P, b, sizeof(P));
        return Obj().p("t_pos", P.t_pos).i("t_max", P.t_max).i("S", P.S).i("G", P.G).i("nbg", P.nbg).i("S_max", P.S_max).i("n_cmp_max", P.n_cmp_max).str();
    };
    auto step = [](const void *b) {
        nsa::DecStepParams P;
        memcpy(&P, b, sizeof(P));
        return Obj().p("t_pos", P.t_pos).i("t_max", P.t_max).i("S", P.S).i("R", P.R).i("S_cmp", P.S_cmp).i("nchunk", P.nchunk).str();
    };
    auto band = [](const void *b) {
        nsa::BandAttnParams P;
        memcpy(&P, b, sizeof(P));
        return Obj().p("t_pos", P.t_pos).i("t_max", P.t_max).i("t0", P.t0).i("S_kv", P.S_kv).i("nsplit", P.nsplit).i("defer_combine", P.defer_combine).p("K", P.K).str();
    };
    const std::vector<Want> wants = {
        positions("qkv_rope_append(rows, mfma)", 0, sizeof(nsa::RopeAppendParams), "rope", rope),
        positions("qkv_rope_append(rows)", 5, sizeof(nsa::RopeAppendParams), "rope", rope),
        positions("cmp_pool(ragged)", 0, sizeof(nsa::CmpPoolParams), "pool", pool),
        positions("decode_rows", 0, sizeof(nsa::DecStepParams), "step", step),
        positions("band_attn_fwd_dual", 0, sizeof(nsa::BandAttnParams), "band_w", band),
        positions("band_attn_fwd_dual", 1, sizeof(nsa::BandAttnParams), "band_c", band),
        positions("band_attn_fwd(split)", 0, sizeof(nsa::BandAttnParams), "band", band),
    };
    auto layer_case = [&](const char *label, const std::function<void(Case &)> &tweak) {
        Case c;
        c.t_pos = t_pos + 5;
        tweak(c);
        nsa_layer_desc L{};
        L.dim = c.dim; L.G = 2; L.h = 6; L.Dk = L.Dv = c.D; L.l = 32; L.d = 16; L.l_sel = 64; L.n_sel = 16; L.w = 512; L.gate_hidden = 32; L.dtype = c.dtype;
        L.rope_base = 10000.f; L.rope_scale = 1.f; L.gate_tau = 1.f;
        L.W_qkv = W_qkv; L.W_out = W_out; L.gate_w1 = L.gate_b1 = L.gate_w2 = L.gate_b2 = gw;
        nsa_kv_desc kv{};
        kv.K_sel = cache[0]; kv.V_sel = cache[1]; kv.K_win = cache[2]; kv.V_win = cache[3]; kv.K_raw = cache[4]; kv.V_raw = cache[5]; kv.K_cmp = cache[6];
        kv.V_cmp = cache[7];
        kv.B = c.B; kv.S_max = c.S_max; kv.n_cmp_max = (c.S_max - 32) / 16 + 1;
        const int te = c.t_max < c.S_max - 1 ? c.t_max : c.S_max - 1, S_sel = (te + 64) / 64 - c.S_sel_short;
        kv.K_cmp = off(kv.K_cmp, c.K_cmp_off); kv.K_sel = off(kv.K_sel, c.K_sel_off);
        if (c.n_cmp_short) kv.n_cmp_max = (te + 1 - 32) / 16 + 1 - 1;
        const std::function<int()> call = [&] {
            return fn(&L, &kv, x, y, c.t_pos, c.t_max, c.S, nullptr, nullptr, nullptr, S_sel, ranges, gates, c.with_ws ? ws : nullptr, c.with_ws ? 64 * MB : 0, nullptr);
        };
        run_args(std::string("layer_decode_ragged/") + label, call, wants);
        g_refuse_at = -1;
        if (call() == NSA_OK)  // the tail of a call that runs: a member of its own, behind the members the case had before
            printf(",\n%s: {%s}", quoted(std::string("layer_decode_ragged/") + label + "_tail").c_str(), tail_fields(call).c_str());
        int launches = -7, route = -7;
        const int prc = plan_fn(&L, c.B, c.S, c.S_max, c.t_max, S_sel, &launches, &route);
        printf(",\n%s: %s", quoted(std::string("layer_decode_ragged/") + label + "_plan").c_str(),
               Obj().i("rc", prc).i("launches", launches).i("route", route).i("workspace", (long long)ws_fn(&L, c.B, c.S, c.S_max)).str().c_str());
    };
    if (long_mode) {
        NSA_FN(nsa_hip_set_tuning)("DECODE_LONG", 1);
        layer_case("in_range_m7c_B3_S8", [](Case &) {});
        layer_case("in_range_D128_B3_S4", [](Case &c) { c.D = 128; c.dim = 1536; c.S = 4; });
        layer_case("long_t_max70000", [](Case &c) { c.S_max = 131072; c.t_max = 70000; });
        layer_case("long_t_max131071", [](Case &c) { c.S_max = 131072; c.t_max = 131071; });
        layer_case("long_D128_t_max20000", [](Case &c) { c.D = 128; c.dim = 1536; c.S = 4; c.S_max = 32768; c.t_max = 20000; });
        layer_case("long_t_max131072_declined", [](Case &c) { c.S_max = 140000; c.t_max = 131072; });
        NSA_FN(nsa_hip_set_tuning)("DECODE_LONG", 0);
        layer_case("off_t_max70000_declined", [](Case &c) { c.S_max = 131072; c.t_max = 70000; });
        return;
    }
    layer_case("m7c_B3_S8", [](Case &) {});
    layer_case("m7c_B3_S8_no_token_due", [](Case &c) { c.t_max = 1063; });
    layer_case("m7c_B16_S1", [](Case &c) { c.B = 16; c.S = 1; });
    layer_case("m7c_B1_S2_chunk_loop", [](Case &c) { c.B = 1; c.S = 2; });
    layer_case("D128_B3_S4", [](Case &c) { c.D = 128; c.dim = 1536; c.S = 4; });
    layer_case("t_max_beyond_capacity", [](Case &c) { c.t_max = 5000; });
    layer_case("t_max_below_S", [](Case &c) { c.t_max = 3; });  // nobody can be live: planned from position 0, never a negative one
    layer_case("f32_declined", [](Case &c) { c.dtype = NSA_DT_F32; });
    layer_case("t_max70000_declined", [](Case &c) { c.S_max = 131072; c.t_max = 70000; });
    layer_case("D128_t_max20000_declined", [](Case &c) { c.D = 128; c.dim = 1536; c.S_max = 32768; c.t_max = 20000; });
    layer_case("S17_refused", [](Case &c) { c.S = 17; });
    layer_case("null_t_pos", [](Case &c) { c.t_pos = nullptr; });
    layer_case("t_pos_2_bytes_off", [&](Case &c) { c.t_pos = (const int32_t *)off(t_pos, 2); });
    layer_case("no_workspace", [](Case &c) { c.with_ws = false; });
    NSA_FN(nsa_hip_set_tuning)("DECODE_UNFUSED", 1);
    layer_case("DECODE_UNFUSED_1_declined", [](Case &) {});
    NSA_FN(nsa_hip_set_tuning)("DECODE_UNFUSED", -1);
    // the declines nothing above walks
    layer_case("K_cmp_2_bytes_off", [](Case &c) { c.K_cmp_off = 2; });
    layer_case("K_sel_2_bytes_off", [](Case &c) { c.K_sel_off = 2; });
    layer_case("n_cmp_max_one_short", [](Case &c) { c.n_cmp_short = 1; });
    layer_case("S_sel_one_short", [](Case &c) { c.S_sel_short = 1; });
    layer_case("D96_declined", [](Case &c) { c.D = 96; });
    layer_case("B0", [](Case &c) { c.B = 0; });
    layer_case("t_max_minus_1", [](Case &c) { c.t_max = -1; });
    // two defects at once: which message wins (the order of the checks is behaviour)
    layer_case("S17_and_null_t_pos", [](Case &c) { c.S = 17; c.t_pos = nullptr; });
    layer_case("f32_and_S_sel_one_short", [](Case &c) { c.dtype = NSA_DT_F32; c.S_sel_short = 1; });
    layer_case("t_max70000_declined_and_no_workspace", [](Case &c) { c.S_max = 131072; c.t_max = 70000; c.with_ws = false; });
    layer_case("K_cmp_2_bytes_off_and_no_workspace", [](Case &c) { c.K_cmp_off = 2; c.with_ws = false; });
}

// ---- dispatch_check <library> layer_paged: the layer's paged call (nsa_layer_decode_paged), cases of their own like `layer_ragged`.  Every
// case prints the launchers in order with their geometry, the plan's answer for the same shape, the verdict launch's block, BOTH writers'
// argument blocks in full (RopePagedParams, CmpPoolPagedParams: the pools, the capacities, the table block) and the position array and the
// table as they arrive at the readers.  The positions, the table and the pools are device memory the host must never read: addresses inside
// buffers of 0x7f bytes.  Every launch behind the pre-pass must name ws + <the offset of t_live> as its position array, never t_pos.
static void layer_paged_cases(bool long_mode = false) {  // long_mode: as layer_ragged_cases
    const size_t MB = 1 << 20;
    void *x = dev(MB), *y = dev(MB), *W_qkv = dev(MB), *W_out = dev(MB), *gw = dev(MB), *ws = dev(128 * MB);
    void *pool[8];
    static const char *pname[8] = {"K_sel", "V_sel", "K_win", "V_win", "K_raw", "V_raw", "K_cmp", "V_cmp"};
    int32_t *t_pos = (int32_t *)dev(MB, 0x7f), *table = (int32_t *)dev(MB, 0x7f), *ranges = (int32_t *)dev(MB);
    float *gates = (float *)dev(MB);
    g_named = {{"x", x, MB}, {"y", y, MB}, {"W_qkv", W_qkv, MB}, {"W_out", W_out, MB}, {"t_pos", t_pos, MB}, {"table", table, MB}, {"ranges", ranges, MB},
               {"gates", gates, MB}, {"ws", ws, 128 * MB}};
    for (int i = 0; i < 8; ++i) {
        pool[i] = dev(MB, 0x7f);
        g_named.push_back({pname[i], pool[i], MB});
    }
    g_named.push_back({"gate_w", gw, MB});
    auto fn = NSA_FN(nsa_layer_decode_paged);
    auto plan_fn = NSA_FN(nsa_layer_decode_paged_plan);
    auto ws_fn = NSA_FN(nsa_layer_decode_paged_workspace);
    struct Case {
        int B = 3, S = 8, D = 64, dim = 768, h = 6, w = 512, max_pages = 2, n_pages = 7, t_max = 1059, dtype = NSA_DT_BF16;
        int64_t table_stride = 0 /* 0: max_pages + 3 */;
        const int32_t *t_pos = nullptr, *table = nullptr;
        void *K_win = nullptr;
        bool with_ws = true;
        int S_sel_short = 0;
    };
    auto block = [](const char *launcher, int arg, size_t bytes, const char *key, std::function<std::string(const void *)> print) {
        return Want{std::string(launcher) + " launch", arg, bytes, key, std::move(print)};
    };
    auto pgt = [](const nsa::LayerPageTable &T) { return Obj().p("table", T.table).i("stride", T.stride).i("n_pages", T.n_pages).i("max_pages", T.max_pages).str(); };
    auto live = [pgt](const void *b) {
        nsa::PagedLiveParams P;
        memcpy(&P, b, sizeof(P));
        return Obj().p("t_pos", P.t_pos).p("t_live", P.t_live).raw("pg", pgt(P.pg)).i("B", P.B).i("S", P.S).i("te", P.te).str();
    };
    auto rope = [pgt](const void *b) {
        nsa::RopePagedParams P;
        memcpy(&P, b, sizeof(P));
        Obj o;
        o.p("proj", P.proj).p("Q_out", P.Q_out);
        for (int i = 0; i < 6; ++i) o.p(pname[i], P.cache[i]);
        return o.i("B", P.B).i("S", P.S).i("G", P.G).i("h", P.h).i("Dk", P.Dk).i("Dv", P.Dv).i("S_max", P.S_max).i("t0", P.t0).f("rope_base", P.rope_base)
            .f("inv_scale", P.inv_scale).p("t_pos", P.t_pos).i("t_max", P.t_max).raw("pg", pgt(P.pg)).str();
    };
    auto pool_block = [pgt](const void *b) {
        nsa::CmpPoolPagedParams P;
        memcpy(&P, b, sizeof(P));
        return Obj().p("K_raw", P.K_raw).p("V_raw", P.V_raw).p("K_cmp", P.K_cmp).p("V_cmp", P.V_cmp).i("nbg", P.nbg).i("S_max", P.S_max).i("n_cmp_max", P.n_cmp_max)
            .i("Dk", P.Dk).i("Dv", P.Dv).i("l", P.l).i("d", P.d).f("rope_base", P.rope_base).f("inv_scale", P.inv_scale).p("t_pos", P.t_pos).i("t_max", P.t_max)
            .i("S", P.S).i("G", P.G).raw("pg", pgt(P.pg)).str();
    };
    auto step = [](const void *b) {
        nsa::DecStepParams P;
        memcpy(&P, b, sizeof(P));
        return Obj().p("t_pos", P.t_pos).i("t_max", P.t_max).i("S", P.S).i("R", P.R).i("S_cmp", P.S_cmp).i("nchunk", P.nchunk).p("Kc", P.Kc).i("csb", P.csb)
            .p("table", P.block_table).i("table_stride", P.bt_stride).i("n_pages", P.n_pages).str();
    };
    auto band = [](const void *b) {
        nsa::BandAttnParams P;
        memcpy(&P, b, sizeof(P));
        return Obj().p("t_pos", P.t_pos).i("t_max", P.t_max).i("t0", P.t0).i("S_kv", P.S_kv).i("nsplit", P.nsplit).i("defer_combine", P.defer_combine).p("K", P.K)
            .p("V", P.V).i("ksb", P.ksb).i("ksg", P.ksg).i("a", P.a).i("dd", P.dd).i("w", P.w).str();
    };
    auto band_table = [](const void *b) {
        nsa::BandPageTable P;
        memcpy(&P, b, sizeof(P));
        return show(P);
    };
    const std::vector<Want> wants = {
        block("paged_live", 0, sizeof(nsa::PagedLiveParams), "live", live),
        block("qkv_rope_append(paged, mfma)", 0, sizeof(nsa::RopePagedParams), "rope", rope),
        block("qkv_rope_append(paged)", 5, sizeof(nsa::RopePagedParams), "rope", rope),
        block("cmp_pool(paged)", 0, sizeof(nsa::CmpPoolPagedParams), "pool", pool_block),
        block("decode_paged", 0, sizeof(nsa::DecStepParams), "step", step),
        block("band_attn_fwd(split)", 0, sizeof(nsa::BandAttnParams), "band", band),
        block("band_attn_fwd(split)", 1, sizeof(nsa::BandPageTable), "band_table", band_table),
        block("band_attn_fwd", 0, sizeof(nsa::BandAttnParams), "band", band),
        block("band_attn_fwd", 1, sizeof(nsa::BandPageTable), "band_table", band_table),
    };
    auto layer_case = [&](const char *label, const std::function<void(Case &)> &tweak) {
        Case c;
        c.t_pos = t_pos + 5, c.table = table + 7, c.K_win = pool[2];
        tweak(c);
        nsa_layer_desc L{};
        L.dim = c.dim; L.G = 2; L.h = c.h; L.Dk = L.Dv = c.D; L.l = 32; L.d = 16; L.l_sel = 64; L.n_sel = 16; L.w = c.w; L.gate_hidden = 32; L.dtype = c.dtype;
        L.rope_base = 10000.f; L.rope_scale = 1.f; L.gate_tau = 1.f;
        L.W_qkv = W_qkv; L.W_out = W_out; L.gate_w1 = L.gate_b1 = L.gate_w2 = L.gate_b2 = gw;
        nsa_paged_kv_desc kv{};
        kv.K_sel = pool[0]; kv.V_sel = pool[1]; kv.K_win = c.K_win; kv.V_win = pool[3]; kv.K_raw = pool[4]; kv.V_raw = pool[5]; kv.K_cmp = pool[6]; kv.V_cmp = pool[7];
        kv.block_table = c.table;
        kv.table_stride = c.table_stride ? c.table_stride : c.max_pages + 3;
        kv.n_pages = c.n_pages; kv.B = c.B; kv.max_pages = c.max_pages;
        const long long cap = (long long)c.max_pages * 1024;
        const int te = c.t_max < cap - 1 ? c.t_max : (int)(cap - 1 > 0 ? cap - 1 : 0), S_sel = (te + 64) / 64 - c.S_sel_short;
        const std::function<int()> call = [&] {
            return fn(&L, &kv, x, y, c.t_pos, c.t_max, c.S, nullptr, nullptr, nullptr, S_sel, ranges, gates, c.with_ws ? ws : nullptr, c.with_ws ? 128 * MB : 0, nullptr);
        };
        run_args(std::string("layer_decode_paged/") + label, call, wants);
        g_refuse_at = -1;
        if (call() == NSA_OK)  // the tail of a call that runs: a member of its own, behind the members the case had before
            printf(",\n%s: {%s}", quoted(std::string("layer_decode_paged/") + label + "_tail").c_str(), tail_fields(call).c_str());
        int launches = -7, route = -7;
        const int prc = plan_fn(&L, c.B, c.S, c.max_pages, c.t_max, S_sel, &launches, &route);
        printf(",\n%s: %s", quoted(std::string("layer_decode_paged/") + label + "_plan").c_str(),
               Obj().i("rc", prc).i("launches", launches).i("route", route).i("workspace", (long long)ws_fn(&L, c.B, c.S, c.max_pages)).str().c_str());
    };
    if (long_mode) {
        NSA_FN(nsa_hip_set_tuning)("DECODE_LONG", 1);
        layer_case("in_range_m7c_B3_S8", [](Case &) {});
        layer_case("in_range_D128_B3_S4", [](Case &c) { c.D = 128; c.dim = 1536; c.S = 4; });
        layer_case("long_t_max70000", [](Case &c) { c.max_pages = 128; c.t_max = 70000; });
        layer_case("long_t_max131071", [](Case &c) { c.max_pages = 128; c.t_max = 131071; });
        layer_case("long_D128_t_max20000", [](Case &c) { c.D = 128; c.dim = 1536; c.S = 4; c.max_pages = 32; c.t_max = 20000; });
        layer_case("long_t_max131072_declined", [](Case &c) { c.max_pages = 200; c.t_max = 131072; });
        NSA_FN(nsa_hip_set_tuning)("DECODE_LONG", 0);
        layer_case("off_t_max70000_declined", [](Case &c) { c.max_pages = 128; c.t_max = 70000; });
        return;
    }
    layer_case("m7c_B3_S8", [](Case &) {});
    layer_case("m7c_B16_S1", [](Case &c) { c.B = 16; c.S = 1; });
    layer_case("m7c_B1_S2_chunk_loop", [](Case &c) { c.B = 1; c.S = 2; });
    layer_case("m7c_B600_S3_unsplit_bands", [](Case &c) { c.B = 600; c.S = 3; });
    layer_case("D128_B3_S4", [](Case &c) { c.D = 128; c.dim = 1536; c.S = 4; });
    layer_case("t_max_beyond_capacity", [](Case &c) { c.t_max = 5000; });
    layer_case("t_max_below_S", [](Case &c) { c.t_max = 3; });
    layer_case("max_pages_2pow20", [](Case &c) { c.max_pages = 1 << 20; c.table_stride = 1 << 20; });
    // the declines: each with its message and no launch
    layer_case("f32_declined", [](Case &c) { c.dtype = NSA_DT_F32; });
    layer_case("D96_declined", [](Case &c) { c.D = 96; });
    layer_case("h17_declined", [](Case &c) { c.h = 17; });
    layer_case("w0_declined", [](Case &c) { c.w = 0; });
    layer_case("t_max70000_declined", [](Case &c) { c.max_pages = 128; c.t_max = 70000; });
    layer_case("D128_t_max20000_declined", [](Case &c) { c.D = 128; c.dim = 1536; c.max_pages = 32; c.t_max = 20000; });
    layer_case("S17_refused", [](Case &c) { c.S = 17; });
    layer_case("null_t_pos", [](Case &c) { c.t_pos = nullptr; });
    layer_case("t_pos_2_bytes_off", [&](Case &c) { c.t_pos = (const int32_t *)off(t_pos, 2); });
    layer_case("null_table", [](Case &c) { c.table = nullptr; });
    layer_case("table_2_bytes_off", [&](Case &c) { c.table = (const int32_t *)off(table, 2); });
    layer_case("table_stride_below_max_pages", [](Case &c) { c.table_stride = 1; });
    layer_case("max_pages0", [](Case &c) { c.max_pages = 0; c.table_stride = 4; });
    layer_case("max_pages_above_2pow20", [](Case &c) { c.max_pages = (1 << 20) + 1; c.table_stride = 1 << 21; });
    layer_case("n_pages0", [](Case &c) { c.n_pages = 0; });
    layer_case("null_pool", [](Case &c) { c.K_win = nullptr; });
    layer_case("K_win_2_bytes_off", [&](Case &c) { c.K_win = off(pool[2], 2); });
    layer_case("no_workspace", [](Case &c) { c.with_ws = false; });
    NSA_FN(nsa_hip_set_tuning)("DECODE_UNFUSED", 1);
    layer_case("DECODE_UNFUSED_1_declined", [](Case &) {});
    NSA_FN(nsa_hip_set_tuning)("DECODE_UNFUSED", -1);
    // the declines nothing above walks
    layer_case("S_sel_one_short", [](Case &c) { c.S_sel_short = 1; });
    layer_case("B0", [](Case &c) { c.B = 0; });
    layer_case("t_max_minus_1", [](Case &c) { c.t_max = -1; });
    // two defects at once: which message wins (the order of the checks is behaviour)
    layer_case("table_stride_below_max_pages_and_f32", [](Case &c) { c.table_stride = 1; c.dtype = NSA_DT_F32; });
    layer_case("table_stride_below_max_pages_and_max_pages0", [](Case &c) { c.table_stride = -1; c.max_pages = 0; });
    layer_case("K_win_2_bytes_off_and_t_max70000_declined", [&](Case &c) { c.K_win = off(pool[2], 2); c.max_pages = 128; c.t_max = 70000; });
    layer_case("K_win_2_bytes_off_and_no_workspace", [&](Case &c) { c.K_win = off(pool[2], 2); c.with_ws = false; });
    layer_case("null_table_and_S17", [](Case &c) { c.table = nullptr; c.S = 17; });
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: dispatch_check <libnsa_sel_hip.so> [ragged | layer_ragged | layer_paged | paged | band_paged | decode_long]\n");
        return 2;
    }
    g_lib = dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL);
    if (!g_lib) {
        fprintf(stderr, "%s\n", dlerror());
        return 2;
    }
    if (argc >= 3 && !strcmp(argv[2], "ragged")) {  // the cases of the ragged entry points alone (tests/test_dispatch_ragged_host.py)
        printf("{");
        ragged_cases();
        printf("\n}\n");
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[2], "paged")) {  // the paged decode step alone (tests/test_dispatch_paged_host.py)
        printf("{");
        paged_cases();
        printf("\n}\n");
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[2], "band_paged")) {  // the paged band forward alone (tests/test_dispatch_band_paged_host.py)
        printf("{");
        band_paged_cases();
        printf("\n}\n");
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[2], "layer_ragged")) {  // the layer's ragged call alone (tests/test_layer_decode_ragged_host.py)
        printf("{");
        layer_ragged_cases();
        printf("\n}\n");
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[2], "layer_paged")) {  // the layer's paged call alone (tests/test_layer_decode_paged_host.py)
        printf("{");
        layer_paged_cases();
        printf("\n}\n");
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[2], "decode_long")) {  // the long-row form of the ragged / paged step (tests/test_dispatch_decode_long_host.py)
        printf("{");
        ragged_cases(true);
        paged_cases(true);
        layer_ragged_cases(true);
        layer_paged_cases(true);
        printf("\n}\n");
        return 0;
    }
    auto set_tuning = NSA_FN(nsa_hip_set_tuning);
    const int dt = NSA_DT_BF16;
    const int B = 1, S = 128, G = 2, h = 6, D = 64, S_kv = 128, n = 16;
    const int64_t sb = (int64_t)G * S_kv * D, sg = (int64_t)S_kv * D;
    const size_t MB = 1 << 20;
    void *Q = dev(MB), *K = dev(MB), *V = dev(MB), *O = dev(MB), *dO = dev(MB), *dQ = dev(MB), *ws = dev(64 * MB);
    float *lse = (float *)dev(MB), *dK = (float *)dev(MB), *dV = (float *)dev(MB), *p_grp = (float *)dev(MB);
    int32_t *ranges = (int32_t *)dev(MB);
    const size_t dkv_bytes = sizeof(float) * (size_t)B * G * S_kv * D;
    printf("{");

    // ---- selection attention forward: the MFMA route asks for aligned operands, everything else keeps the generic (VALU) kernel
    auto fwd = NSA_FN(nsa_sel_attn_fwd);
    auto sel_fwd = [&](void *K_, int64_t kss, int variant, float scale, int n_ranges = 16, float *lse_ = nullptr) {
        return fwd(Q, K_, V, ranges, O, lse_, B, S, G, h, D, D, S_kv, n_ranges, sb, sg, kss, sb, sg, D, dt, scale, variant, ws, 64 * MB, nullptr);
    };
    run("sel_attn_fwd/aligned", [&] { return sel_fwd(K, D, 0, 0.f); });
    run("sel_attn_fwd/K_2_bytes_off", [&] { return sel_fwd(off(K, 2), D, 0, 0.f); });
    run("sel_attn_fwd/K_8_bytes_off", [&] { return sel_fwd(off(K, 8), D, 0, 0.f); });
    run("sel_attn_fwd/kss_not_8", [&] { return sel_fwd(K, D + 4, 0, 0.f); });
    run("sel_attn_fwd/forced_mfma_unaligned", [&] { return sel_fwd(off(K, 2), D, 2, 0.f); });
    run("sel_attn_fwd/forced_mfma_aligned", [&] { return sel_fwd(K, D, 2, 0.f); });
    run("sel_attn_fwd/no_ranges", [&] { memset(O, 0xff, 4096); return sel_fwd(K, D, 0, 0.f, 0, lse); },
        [&] { return std::string("\"O_zero\": ") + (all_zero(O, (size_t)B * S * G * h * D * 2) ? "true" : "false"); });
    peek<nsa::SelAttnParams>(0);
    run("sel_attn_fwd/scale_default", [&] { return sel_fwd(K, D, 1, 0.f); }, peeked_scale<nsa::SelAttnParams>);
    peek<nsa::SelAttnParams>(0);
    run("sel_attn_fwd/scale_negative", [&] { return sel_fwd(K, D, 1, -1.f); }, peeked_scale<nsa::SelAttnParams>);
    peek<nsa::SelAttnParams>(0);
    run("sel_attn_fwd/scale_given", [&] { return sel_fwd(K, D, 1, 0.25f); }, peeked_scale<nsa::SelAttnParams>);

    // ---- selection attention backward: the generic kernel accumulates into dK / dV, so the host zeroes them on that route only
    auto bwd = NSA_FN(nsa_sel_attn_bwd);
    const size_t bwd_need = NSA_FN(nsa_sel_attn_bwd_workspace)(B, S, G, h, D, D, S_kv, dt, 0);
    auto sel_bwd = [&](void *K_, void *dO_, int variant, float scale, int n_ranges = 16, size_t ws_bytes = 64 * MB) {
        memset(dK, 0xff, dkv_bytes);
        memset(dV, 0xff, dkv_bytes);
        memset(dQ, 0xff, 4096);
        return bwd(Q, K_, V, ranges, O, lse, dO_, dQ, dK, dV, B, S, G, h, D, D, S_kv, n_ranges, sb, sg, D, sb, sg, D, dt, scale, variant, ws, ws_bytes,
                   nullptr);
    };
    auto zeroed = [&] {
        return std::string("\"dK_zero\": ") + (all_zero(dK, dkv_bytes) ? "true" : "false") + ", \"dV_zero\": " + (all_zero(dV, dkv_bytes) ? "true" : "false") +
               ", \"dQ_zero\": " + (all_zero(dQ, (size_t)B * S * G * h * D * 2) ? "true" : "false");
    };
    run("sel_attn_bwd/aligned", [&] { return sel_bwd(K, dO, 0, 0.f); }, zeroed);
    run("sel_attn_bwd/K_2_bytes_off", [&] { return sel_bwd(off(K, 2), dO, 0, 0.f); }, zeroed);
    run("sel_attn_bwd/dO_8_bytes_off", [&] { return sel_bwd(K, off(dO, 8), 0, 0.f); }, zeroed);
    run("sel_attn_bwd/workspace_one_byte_short", [&] { return sel_bwd(K, dO, 0, 0.f, 16, bwd_need - 1); }, zeroed);
    run("sel_attn_bwd/generic_asked", [&] { return sel_bwd(K, dO, 1, 0.f); }, zeroed);
    run("sel_attn_bwd/forced_mfma_unaligned", [&] { return sel_bwd(off(K, 2), dO, 2, 0.f); }, zeroed);
    run("sel_attn_bwd/no_ranges", [&] { return sel_bwd(K, dO, 0, 0.f, 0); }, zeroed);
    peek<nsa::SelAttnBwdParams>(0);
    run("sel_attn_bwd/scale_default", [&] { return sel_bwd(K, dO, 1, 0.f); }, peeked_scale<nsa::SelAttnBwdParams>);
    peek<nsa::SelAttnBwdParams>(0);
    run("sel_attn_bwd/scale_given", [&] { return sel_bwd(K, dO, 1, 0.25f); }, peeked_scale<nsa::SelAttnBwdParams>);

    // ---- band attention forward and backward
    auto bfwd = NSA_FN(nsa_band_attn_fwd);
    auto band_fwd = [&](void *K_, void *O_, int variant, float scale) {
        return bfwd(Q, K_, V, O_, nullptr, B, S, G, h, D, D, S_kv, sb, sg, D, sb, sg, D, 0, 0, 1, 0, 64, dt, scale, variant, ws, 64 * MB, nullptr);
    };
    run("band_attn_fwd/aligned", [&] { return band_fwd(K, O, 0, 0.f); });
    run("band_attn_fwd/K_2_bytes_off", [&] { return band_fwd(off(K, 2), O, 0, 0.f); });
    run("band_attn_fwd/O_4_bytes_off", [&] { return band_fwd(K, off(O, 4), 0, 0.f); });
    run("band_attn_fwd/forced_mfma_unaligned", [&] { return band_fwd(off(K, 2), O, 2, 0.f); });
    peek<nsa::BandAttnParams>(0);
    run("band_attn_fwd/scale_default", [&] { return band_fwd(K, O, 1, 0.f); }, peeked_scale<nsa::BandAttnParams>);
    peek<nsa::BandAttnParams>(0);
    run("band_attn_fwd/scale_given", [&] { return band_fwd(K, O, 1, 0.25f); }, peeked_scale<nsa::BandAttnParams>);
    auto bbwd = NSA_FN(nsa_band_attn_bwd);
    const size_t bband_need = NSA_FN(nsa_band_attn_bwd_workspace)(B, S, G, h, D, D, S_kv, dt, 0);
    auto band_bwd = [&](void *K_, void *dO_, int variant, size_t ws_bytes = 64 * MB) {
        memset(dK, 0xff, dkv_bytes);
        memset(dV, 0xff, dkv_bytes);
        memset(dQ, 0xff, 4096);
        return bbwd(Q, K_, V, O, lse, dO_, dQ, dK, dV, B, S, G, h, D, D, S_kv, sb, sg, D, sb, sg, D, 0, 0, 1, 0, 64, dt, 0.f, variant, ws, ws_bytes,
                    nullptr);
    };
    run("band_attn_bwd/aligned", [&] { return band_bwd(K, dO, 0); }, zeroed);
    run("band_attn_bwd/K_2_bytes_off", [&] { return band_bwd(off(K, 2), dO, 0); }, zeroed);
    run("band_attn_bwd/dO_8_bytes_off", [&] { return band_bwd(K, off(dO, 8), 0); }, zeroed);
    run("band_attn_bwd/forced_mfma_unaligned", [&] { return band_bwd(off(K, 2), dO, 2); }, zeroed);
    run("band_attn_bwd/workspace_one_byte_short", [&] { return band_bwd(K, dO, 0, bband_need - 1); }, zeroed);
    run("band_attn_bwd/workspace_exact", [&] { return band_bwd(K, dO, 0, bband_need); }, zeroed);

    // ---- selector + attention: one launch only with SEL_FUSE on aligned operands
    auto ssa = NSA_FN(nsa_sel_select_attn_fwd);
    // (with fewer than 1024 rows the attention splits the keys and is never fused: S = 512 is the shape on which SEL_FUSE decides)
    auto select_attn = [&](void *K_, int S_) {
        return ssa(p_grp, 0, nullptr, (S_ + 63) / 64, 64, n, 1, 2, NSA_SEL_SEQUENTIAL, S_, ranges, n, Q, K_, V, O, nullptr, B, S_, G, h, D, D, S_, (int64_t)G * S_ * D,
                   (int64_t)S_ * D, D, (int64_t)G * S_ * D, (int64_t)S_ * D, D, dt, 0.f, ws, 64 * MB, nullptr);
    };
    for (int S_ : {128, 512}) {
        const std::string at = "sel_select_attn_fwd/S" + std::to_string(S_);
        run((at + "_two_launches").c_str(), [&] { return select_attn(K, S_); });
        set_tuning("SEL_FUSE", 1);
        run((at + "_SEL_FUSE").c_str(), [&] { return select_attn(K, S_); });
        run((at + "_SEL_FUSE_K_2_bytes_off").c_str(), [&] { return select_attn(off(K, 2), S_); });
        set_tuning("SEL_FUSE", 0);
    }

    // ---- scorer: default scale; decode-normalised rows leave the decode-shaped route at S = 64
    auto scores_rows = NSA_FN(nsa_sel_scores_rows);
    void *Kc = dev(MB);
    int32_t *csc_ptr = (int32_t *)dev(MB), *csc_rows = (int32_t *)dev(MB);
    float *csc_vals = (float *)dev(MB);
    auto scores = [&](int S_, int norm, int variant, float scale) {
        const int n_cmp = (S_ - 32) / 16 + 1;
        return scores_rows(Q, Kc, p_grp, B, S_, G, h, D, n_cmp, (int64_t)G * n_cmp * D, (int64_t)n_cmp * D, D, csc_ptr, csc_rows, csc_vals, (S_ + 63) / 64,
                           32, 16, 64, 0, variant, dt, scale, 0, norm, ws, 64 * MB, nullptr);
    };
    for (int S_ : {63, 64})
        for (int norm : {0, 1}) {
            char label[64];
            snprintf(label, sizeof(label), "sel_scores_rows/S%d_norm%d", S_, norm);
            run(label, [&] { return scores(S_, norm, 0, 0.f); });
        }
    for (float scale : {0.f, -1.f, 0.25f}) {
        char label[64];
        snprintf(label, sizeof(label), "sel_scores_rows/generic_scale_%g", scale);
        peek<nsa::PcmpParams>(0);
        run(label, [&] { return scores(64, 0, 1, scale); }, peeked_scale<nsa::PcmpParams>);
        snprintf(label, sizeof(label), "pcmp_all/scale_%g", scale);
        peek<nsa::PcmpParams>(0);
        run(label, [&] { return NSA_FN(nsa_pcmp_all)(Q, Kc, p_grp, B, 64, G, h, D, 3, (int64_t)G * 3 * D, 3 * D, D, dt, scale, nullptr); }, peeked_scale<nsa::PcmpParams>);
    }

    // ---- the scorer and selector family with its argument blocks.  64 rows of h = 6 at norm = 1 are the tiled (MFMA) scorers' shape: with
    // norm = 0 the 128 rows of B = 1, G = 2 stay under DECODE_MAX_ROWS and take the decode-shaped pair
    float *p_slc = (float *)dev(MB);
    int32_t *t_rows = (int32_t *)dev(MB);
    g_named = {{"Q", Q, MB}, {"O", O, MB}, {"ranges", ranges, MB}, {"ws", ws, 64 * MB}, {"p_grp", p_grp, MB}, {"Kc", Kc, MB}, {"csc_ptr", csc_ptr, MB},
               {"csc_rows", csc_rows, MB}, {"csc_vals", csc_vals, MB}, {"p_slc", p_slc, MB}, {"t_rows", t_rows, MB}};
    struct ScoresCase {
        int B = 1, S = 64, h = 6, S_cmp = 3, dtype = NSA_DT_BF16, causal_skip = 0, variant = 0, q0 = 0, norm = 1;
        void *Kc = nullptr;
        int64_t css = 64;
        size_t ws_bytes = (size_t)64 << 20;
        // the selection of nsa_sel_scores_select_rows
        int mode = NSA_SEL_SEQUENTIAL, out_width = 16;
    };
    typedef std::function<void(ScoresCase &)> Tweak;
    const std::vector<Want> scorer_blocks = {want<nsa::PcmpParams>("pcmp", "PcmpParams"), want<nsa::MapParams>("map_pcmp", "MapParams"),
                                             want<nsa::DecodeParams>("decode_logits", "DecodeParams"), want<nsa::DecodeParams>("decode_pgrp", "DecodeParams"),
                                             want<nsa::ScoresMfmaParams>("scores_mfma", "ScoresMfmaParams"),
                                             want<nsa::ScoresMfmaParams>("scores_mfma32", "ScoresMfmaParams"),
                                             want<nsa::SelectParams>("scores_mfma32", "SelectParams", 1), want<nsa::SelectParams>("select_topn", "SelectParams")};
    auto scores_case = [&](const char *label, const Tweak &tweak) {
        ScoresCase c;
        c.Kc = Kc;
        tweak(c);
        run_args(std::string("sel_scores_rows/") + label, [&] {
            return scores_rows(Q, c.Kc, p_grp, c.B, c.S, G, c.h, D, c.S_cmp, (int64_t)G * c.S_cmp * c.css, (int64_t)c.S_cmp * c.css, c.css, csc_ptr, csc_rows,
                               csc_vals, (c.q0 + c.S + 63) / 64, 32, 16, 64, c.causal_skip, c.variant, c.dtype, 0.f, c.q0, c.norm, ws, c.ws_bytes, nullptr);
        }, scorer_blocks);
    };
    scores_case("v1", [](ScoresCase &c) { c.variant = 1; });
    scores_case("mfma32_h6", [](ScoresCase &) {});
    scores_case("mfma_h4", [](ScoresCase &c) { c.h = 4; });
    for (int form : {0, 1}) {
        set_tuning("SCORES_FORM", form);
        scores_case(form ? "h6_SCORES_FORM_1" : "h6_SCORES_FORM_0", [](ScoresCase &) {});
    }
    set_tuning("SCORES_FORM", -1);
    scores_case("v3", [](ScoresCase &c) { c.variant = 3; });
    scores_case("f32_norm0", [](ScoresCase &c) { c.dtype = NSA_DT_F32; c.norm = 0; });
    scores_case("f32_norm1", [](ScoresCase &c) { c.dtype = NSA_DT_F32; });
    for (int variant : {0, 1, 2}) {  // (the entry point itself never leaves the tiled route of a shape: its callers ask for variant 1)
        const std::string v = variant == 2 ? "_forced_v2" : variant ? "_v1" : "";
        scores_case(("K_cmp_8_bytes_off" + v).c_str(), [&](ScoresCase &c) { c.Kc = off(Kc, 8); c.variant = variant; });
        scores_case(("css_not_8" + v).c_str(), [&](ScoresCase &c) { c.css = 68; c.variant = variant; });
    }
    for (int variant : {0, 1, 3})
        scores_case(("q0_100_v" + std::to_string(variant)).c_str(), [&](ScoresCase &c) { c.q0 = 100; c.S_cmp = 9; c.variant = variant; });
    for (int skip : {0, 1, 2}) scores_case(("causal_skip_" + std::to_string(skip)).c_str(), [&](ScoresCase &c) { c.causal_skip = skip; });
    scores_case("S_cmp_0", [](ScoresCase &c) { c.S_cmp = 0; });
    // the generic scorer walks its rows in chunks of what the workspace holds: three rows' worth on a call of ten
    scores_case("v1_10_rows_workspace_of_3", [](ScoresCase &c) { c.variant = 1; c.S = 5; c.S_cmp = 9; c.norm = 0; c.ws_bytes = 3 * sizeof(float) * 6 * 9; });

    auto select_rows_fn = NSA_FN(nsa_sel_scores_select_rows);
    auto select_rows_case = [&](const char *label, const Tweak &tweak) {
        ScoresCase c;
        c.Kc = Kc;
        tweak(c);
        run_args(std::string("sel_scores_select_rows/") + label, [&] {
            return select_rows_fn(Q, c.Kc, p_grp, c.B, c.S, G, c.h, D, c.S_cmp, (int64_t)G * c.S_cmp * c.css, (int64_t)c.S_cmp * c.css, c.css, csc_ptr, csc_rows,
                                  csc_vals, (c.q0 + c.S + 63) / 64, 32, 16, 64, c.causal_skip, c.dtype, 0.f, c.q0, n, 1, 2, c.mode, c.S, ranges, c.out_width,
                                  c.q0, c.norm, ws, c.ws_bytes, nullptr);
        }, scorer_blocks);
    };
    auto width = NSA_FN(nsa_batched_ranges_width);
    select_rows_case("mfma32_sequential", [](ScoresCase &) {});
    set_tuning("SCORES_SELECT", 1);
    select_rows_case("mfma32_sequential_SCORES_SELECT_1", [](ScoresCase &) {});
    select_rows_case("mfma32_batched_SCORES_SELECT_1", [&](ScoresCase &c) { c.mode = NSA_SEL_BATCHED; c.out_width = width(64, 1, 64, n, 1, 2); });
    set_tuning("SCORES_SELECT", -1);
    select_rows_case("mfma32_batched", [&](ScoresCase &c) { c.mode = NSA_SEL_BATCHED; c.out_width = width(64, 1, 64, n, 1, 2); });
    select_rows_case("mfma32_q0_100", [](ScoresCase &c) { c.q0 = 100; c.S_cmp = 9; });
    select_rows_case("mfma_h4", [](ScoresCase &c) { c.h = 4; });
    select_rows_case("norm0_decode_shaped", [](ScoresCase &c) { c.norm = 0; });
    select_rows_case("K_cmp_8_bytes_off", [&](ScoresCase &c) { c.Kc = off(Kc, 8); });
    select_rows_case("sequential_wrong_out_width", [](ScoresCase &c) { c.out_width = 15; });
    select_rows_case("batched_wrong_out_width", [&](ScoresCase &c) { c.mode = NSA_SEL_BATCHED; c.out_width = width(64, 1, 64, n, 1, 2) + 1; });
    select_rows_case("no_rows", [](ScoresCase &c) { c.B = 0; });

    auto topn_fn = NSA_FN(nsa_select_topn_ranges);
    for (int S_sel : {64, 65}) {
        const std::string at = "select_topn_ranges/S_sel" + std::to_string(S_sel);
        const int S_ = 64 * S_sel, wb = width(S_, S_sel, 64, n, 1, 2);
        const std::vector<Want> sp = {want<nsa::SelectParams>("select_topn", "SelectParams")};
        run_args(at + "_batched", [&] { return topn_fn(p_grp, (int64_t)S_ * G, S_, G, 0, nullptr, S_sel, 64, n, 1, 2, NSA_SEL_BATCHED, S_, ranges, wb, nullptr); }, sp);
        run_args(at + "_sequential", [&] { return topn_fn(p_grp, (int64_t)4 * G, 4, G, 7, nullptr, S_sel, 64, n, 1, 2, NSA_SEL_SEQUENTIAL, 4, ranges, n, nullptr); }, sp);
        run_args(at + "_t_rows", [&] { return topn_fn(p_grp, (int64_t)4 * G, 4, G, 7, t_rows, S_sel, 64, n, 0, 1, NSA_SEL_SEQUENTIAL, 4, ranges, n, nullptr); }, sp);
    }
    for (float *slc : {(float *)nullptr, p_slc})
        run_args(slc ? "map_pcmp_to_pgrp/with_p_slc" : "map_pcmp_to_pgrp/without_p_slc",
                 [&] { return NSA_FN(nsa_map_pcmp_to_pgrp)((const float *)ws, 10, h, 9, csc_ptr, csc_rows, csc_vals, 3, slc, p_grp, nullptr); },
                 {want<nsa::MapParams>("map_pcmp", "MapParams")});

    // ---- the layer calls on real pointers (the m7c layer, capacity 1024)
    nsa_layer_desc L{};
    L.dim = 768; L.G = 2; L.h = 6; L.Dk = 64; L.Dv = 64; L.l = 32; L.d = 16; L.l_sel = 64; L.n_sel = 16; L.w = 512; L.gate_hidden = 32; L.dtype = dt;
    L.rope_base = 10000.f; L.rope_scale = 1.f; L.gate_tau = 1.f;
    L.W_qkv = dev(4 * MB); L.W_out = dev(4 * MB); L.gate_w1 = dev(MB); L.gate_b1 = dev(MB); L.gate_w2 = dev(MB); L.gate_b2 = dev(MB);
    nsa_kv_desc kv{};
    kv.K_sel = dev(MB); kv.V_sel = dev(MB); kv.K_win = dev(MB); kv.V_win = dev(MB); kv.K_raw = dev(MB); kv.V_raw = dev(MB);
    void *Kcmp = dev(MB);
    kv.K_cmp = Kcmp; kv.V_cmp = dev(MB);
    kv.B = 1; kv.S_max = 1024; kv.n_cmp_max = 63;
    void *proj = dev(4 * MB), *O_mix = dev(MB), *x = dev(MB), *y = dev(MB);
    const int S_sel_max = 16;
    auto prefill_fn = NSA_FN(nsa_layer_prefill);
    auto extend_fn = NSA_FN(nsa_layer_extend);
    auto decode_fn = NSA_FN(nsa_layer_decode_step);
    auto prefill = [&](int S_, size_t ws_bytes = 64 * MB, int selector = NSA_SEL_BATCHED) {
        return prefill_fn(&L, &kv, proj, S_, selector, csc_ptr, csc_rows, csc_vals, S_sel_max, ranges, selector == NSA_SEL_BATCHED ? width(S_, S_sel_max, 64, 16, 1, 2) : 16, O_mix, nullptr,
                          ws, ws_bytes, nullptr);
    };
    auto extend = [&](int t0, int S_, size_t ws_bytes = 64 * MB) {
        return extend_fn(&L, &kv, proj, t0, S_, csc_ptr, csc_rows, csc_vals, S_sel_max, ranges, O_mix, nullptr, ws, ws_bytes, nullptr);
    };
    auto decode = [&](int t, size_t ws_bytes = 64 * MB) {
        return decode_fn(&L, &kv, x, y, t, csc_ptr, csc_rows, csc_vals, S_sel_max, nullptr, nullptr, ws, ws_bytes, nullptr);
    };
    const size_t need_p = NSA_FN(nsa_layer_prefill_workspace)(&L, 1, 100, S_sel_max);
    const size_t need_e = NSA_FN(nsa_layer_extend_workspace)(&L, 1, 100, 924, S_sel_max);
    const size_t need_d = NSA_FN(nsa_layer_decode_step_workspace)(&L, 1, 1024);
    run("layer_prefill/S100_sequential", [&] { return prefill(100, 64 * MB, NSA_SEL_SEQUENTIAL); });
    run("layer_prefill/S16_no_compressed_token", [&] { return prefill(16); });
    run("layer_prefill/workspace_exact", [&] { return prefill(100, need_p); });
    run("layer_prefill/workspace_one_byte_short", [&] { return prefill(100, need_p - 1); });
    run("layer_extend/t100_S28", [&] { return extend(100, 28); });
    run("layer_extend/t100_S64", [&] { return extend(100, 64); });
    run("layer_extend/to_capacity", [&] { return extend(924, 100); });
    run("layer_extend/to_capacity_workspace_exact", [&] { return extend(924, 100, need_e); });
    run("layer_extend/workspace_one_byte_short", [&] { return extend(924, 100, need_e - 1); });
    run("layer_extend/past_capacity", [&] { return extend(925, 100); });
    // prefill alone decides on SEL_FUSE and on the alignment of K_cmp (S = 512: 1024 rows, the shape on which the choice shows)
    for (int fuse : {0, 1})
        for (int shift : {0, 8})
            for (int S_ : {100, 512}) {
                set_tuning("SEL_FUSE", fuse);
                kv.K_cmp = off(Kcmp, shift);
                const std::string at = "S" + std::to_string(S_) + (fuse ? "_SEL_FUSE" : "") + (shift ? "_K_cmp_8_bytes_off" : "");
                run(("layer_prefill/" + at).c_str(), [&] { return prefill(S_); });
                run(("layer_extend/t0_" + at).c_str(), [&] { return extend(0, S_); });
            }
    set_tuning("SEL_FUSE", 0);
    kv.K_cmp = Kcmp;
    run("layer_decode_step/t100", [&] { return decode(100); });
    run("layer_decode_step/t31_first_compressed_token", [&] { return decode(31); });
    run("layer_decode_step/t5_no_compressed_token", [&] { return decode(5); });
    run("layer_decode_step/workspace_exact", [&] { return decode(100, need_d); });
    run("layer_decode_step/workspace_one_byte_short", [&] { return decode(100, need_d - 1); });
    run("layer_decode_step/position_at_capacity", [&] { return decode(1024); });
    L.Dk = L.Dv = 128;
    run("layer_decode_step/D128_t100", [&] { return decode(100); });
    run("layer_prefill/D128_S100", [&] { return prefill(100); });

    // ---- the decode-step family (m7c layer, capacity 1024), with the argument blocks of the one-launch kernels
    L.Dk = L.Dv = 64;
    g_named.insert(g_named.end(), {{"K_sel", kv.K_sel, MB}, {"V_sel", kv.V_sel, MB}, {"K_cmp", Kcmp, MB}});
    const int64_t csb = (int64_t)L.G * 1024 * D, csg = (int64_t)1024 * D, ccb = (int64_t)L.G * 63 * D, ccg = (int64_t)63 * D;
    auto ncmp = [](int S_) { return S_ < 32 ? 0 : (S_ - 32) / 16 + 1; };
    auto sel_step_fn = NSA_FN(nsa_sel_decode_step);
    auto sel_step_need = [&](int t, int n_top) { return NSA_FN(nsa_sel_decode_step_workspace)(1, L.G, L.h, D, D, ncmp(t + 1), S_sel_max, n_top, dt); };
    auto sel_step = [&](int t, void *Kc_ = nullptr, int n_top = 16, size_t ws_bytes = 64 * MB, int d_ = 16, int l_ = 32, int l_sel_ = 64) {
        return sel_step_fn(Q, Kc_ ? Kc_ : Kcmp, kv.K_sel, kv.V_sel, csc_ptr, csc_rows, csc_vals, ranges, O, 1, L.G, L.h, D, D, (t + 1 - l_) / d_ + 1, S_sel_max, t + 1,
                           l_, d_, l_sel_, n_top, t, ccb, ccg, D, csb, csg, D, csb, csg, D, dt, 0.f, ws, ws_bytes, nullptr);
    };
    run_step("sel_decode_step/t100", [&] { return sel_step(100); });
    run_step("sel_decode_step/t5_no_compressed_token", [&] { return sel_step(5); });
    run_step("sel_decode_step/K_cmp_8_bytes_off", [&] { return sel_step(100, off(Kcmp, 8)); });
    run_step("sel_decode_step/n_top_2", [&] { return sel_step(100, nullptr, 2); });
    run_step("sel_decode_step/workspace_one_byte_short", [&] { return sel_step(100, nullptr, 16, sel_step_need(100, 16) - 1); });
    auto sel_rows_fn = NSA_FN(nsa_sel_decode_rows);
    auto sel_rows = [&](int t0, int S_, void *K_ = nullptr) {
        return sel_rows_fn(Q, Kcmp, K_ ? K_ : kv.K_sel, kv.V_sel, csc_ptr, csc_rows, csc_vals, ranges, O, 1, S_, L.G, L.h, D, D, ncmp(t0 + S_), S_sel_max, t0 + S_, 32, 16,
                           64, 16, t0, ccb, ccg, D, csb, csg, D, csb, csg, D, dt, 0.f, ws, 64 * MB, nullptr);
    };
    run_step("sel_decode_rows/t100_S4", [&] { return sel_rows(100, 4); });
    run_step("sel_decode_rows/t31_S2_first_compressed_token", [&] { return sel_rows(31, 2); });
    run_step("sel_decode_rows/t20_S4_no_compressed_token_at_t0", [&] { return sel_rows(20, 4); });
    run_step("sel_decode_rows/t100_S17", [&] { return sel_rows(100, 17); });
    set_tuning("DECODE_ROWS", 0);
    run_step("sel_decode_rows/t100_S4_DECODE_ROWS_0", [&] { return sel_rows(100, 4); });
    set_tuning("DECODE_ROWS", -1);
    run_step("sel_decode_rows/t100_S4_K_2_bytes_off", [&] { return sel_rows(100, 4, off(kv.K_sel, 2)); });
    auto layer_rows_fn = NSA_FN(nsa_layer_decode_rows);
    auto layer_rows = [&](int t0, int S_, size_t ws_bytes = 64 * MB) {
        return layer_rows_fn(&L, &kv, x, y, t0, S_, csc_ptr, csc_rows, csc_vals, S_sel_max, nullptr, nullptr, ws, ws_bytes, nullptr);
    };
    const size_t need_r = NSA_FN(nsa_layer_decode_rows_workspace)(&L, 1, 4, 1024);
    run_step("layer_decode_rows/t100_S4", [&] { return layer_rows(100, 4); });
    run_step("layer_decode_rows/t100_S1", [&] { return layer_rows(100, 1); });
    run_step("layer_decode_rows/t30_S4_pooling", [&] { return layer_rows(30, 4); });
    run_step("layer_decode_rows/workspace_exact", [&] { return layer_rows(100, 4, need_r); });
    run_step("layer_decode_rows/workspace_one_byte_short", [&] { return layer_rows(100, 4, need_r - 1); });
    run_step("layer_decode_rows/S17", [&] { return layer_rows(100, 17); });
    run_step("layer_decode_rows/past_capacity", [&] { return layer_rows(1021, 4); });
    for (int band : {0, 1}) {  // the tail's other two arms: the band pair as its own dual launch, and riding without the merge
        set_tuning("DECODE_BAND", band);
        run_step(("layer_decode_step/t100_DECODE_BAND_" + std::to_string(band)).c_str(), [&] { return decode(100); });
    }
    set_tuning("DECODE_BAND", -1);
    // the step's separate launches (DECODE_STEP 0): scores + top-n in one launch, or the three-kernel scorer and the select kernel
    // (DECODE_UNFUSED 1), then the attention; a block geometry other than l = 2d, l' = 4d leaves the closed-form stencil
    set_tuning("DECODE_STEP", 0);
    for (int unfused : {-1, 1}) {
        set_tuning("DECODE_UNFUSED", unfused);
        const std::string at = std::string("sel_decode_step/t100_DECODE_STEP_0") + (unfused > 0 ? "_DECODE_UNFUSED_1" : "");
        const std::vector<Want> blocks = {want<nsa::DecodeParams>("decode_score_select", "DecodeParams"), want<nsa::SelectParams>("decode_score_select", "SelectParams", 1),
                                          want<int>("decode_score_select", "cand", 2), want<int>("decode_score_select", "t_token", 3),
                                          want<nsa::DecodeParams>("decode_logits", "DecodeParams"), want<nsa::DecodeParams>("decode_pgrp", "DecodeParams"),
                                          want<nsa::SelectParams>("select_topn", "SelectParams")};
        run_args(at, [&] { return sel_step(100); }, blocks);
        run_args(at + "_geometry_16_16_32", [&] { return sel_step(100, nullptr, 16, 64 * MB, 16, 16, 32); }, blocks);
    }
    set_tuning("DECODE_UNFUSED", -1);
    set_tuning("DECODE_STEP", 1);
    L.Dk = L.Dv = 128;
    run_step("layer_decode_rows/D128_t100_S4", [&] { return layer_rows(100, 4); });

    // ---- the few-row projection family: the smallest shapes on each side of every branch of its route
    L.Dk = L.Dv = 64;
    void *A_lin = dev(MB), *W_lin = dev(MB), *out_lin = dev(MB), *res_lin = dev(MB);
    nsa_block_desc Bk{};
    Bk.attn = L;
    Bk.norm1_w = dev(MB); Bk.norm2_w = dev(MB); Bk.mlp_w1 = dev(8 * MB); Bk.mlp_w2 = dev(8 * MB); Bk.mlp_hidden = 3072; Bk.norm_eps = 1e-5f;
    int32_t *tokens = (int32_t *)dev(MB), *next_tokens = (int32_t *)dev(MB);
    void *embed = dev(8 * MB), *norm_f_w = dev(MB), *lm_head = dev(8 * MB), *logits = dev(MB);
    g_named.insert(g_named.end(), {{"A", A_lin, MB}, {"W_lin", W_lin, MB}, {"out", out_lin, MB}, {"res", res_lin, MB}, {"x", x, MB}, {"y", y, MB},
                                   {"W_qkv", L.W_qkv, 4 * MB}, {"W_out", L.W_out, 4 * MB}, {"norm1_w", Bk.norm1_w, MB}, {"norm2_w", Bk.norm2_w, MB},
                                   {"W_fc1", Bk.mlp_w1, 8 * MB}, {"W_fc2", Bk.mlp_w2, 8 * MB}, {"norm_f_w", norm_f_w, MB}, {"W_lm", lm_head, 8 * MB},
                                   {"logits", logits, MB}});
    auto lin_fn = NSA_FN(nsa_linear_small);
    auto lin = [&](int M, int N, int K, int dtype = NSA_DT_BF16, int epi = 0, size_t a_off = 0) {
        const std::string label = std::string("linear_small/") + (dtype == NSA_DT_F32 ? "f32_" : "") + "M" + std::to_string(M) + "_N" + std::to_string(N) + "_K" +
                                  std::to_string(K) + (epi ? "_epi" + std::to_string(epi) : "") + (a_off ? "_A_2_bytes_off" : "");
        run_proj(label, [&] { return lin_fn(off(A_lin, a_off), W_lin, out_lin, M, N, K, dtype, epi, epi == 2 ? res_lin : nullptr, nullptr); });
    };
    const int few[][2] = {{40, 8}, {37, 520}, {36, 1032}, {36, 3072}, {36, 4096}, {36, 4104}, {4097, 8}, {4100, 1000}, {4100, 1536}};
    for (int M : {1, 2})
        for (const auto &nk : few) lin(M, nk[0], nk[1]);
    lin(2, 37, 520, dt, 0, 2);
    lin(2, 4100, 1000, dt, 0, 2);
    lin(1, 36, 1032, NSA_DT_F32);
    lin(2, 4100, 1000, NSA_DT_F32);
    lin(5, 37, 520, NSA_DT_F32);
    lin(3, 40, 64);
    lin(3, 40, 40);
    lin(3, 40, 64, dt, 0, 2);
    lin(9, 36, 2016);
    lin(9, 36, 2048);
    lin(70, 37, 1024);
    for (int epi : {1, 2}) {  // (epi 0: above) the all-loads-first form, the chunk loop, the MFMA form
        lin(1, 37, 520, dt, epi);
        lin(1, 36, 4104, dt, epi);
        lin(3, 40, 64, dt, epi);
    }
    lin(0, 40, 8);
    lin(1, 0, 8);

    // the block and the model step (m7c block: dim 768, hidden 3072): from three rows on both norms are launches of their own
    auto block_fn = NSA_FN(nsa_block_decode_step);
    auto block = [&](const nsa_block_desc &b, int B_, void *x_) {
        kv.B = B_;
        return block_fn(&b, &kv, x_, y, 100, csc_ptr, csc_rows, csc_vals, S_sel_max, nullptr, nullptr, ws, 64 * MB, nullptr);
    };
    for (int B_ : {1, 2, 3}) run_proj("block_decode_step/B" + std::to_string(B_), [&] { return block(Bk, B_, x); });
    run_proj("block_decode_step/B1_x_2_bytes_off", [&] { return block(Bk, 1, off(x, 2)); });
    nsa_block_desc Bk776 = Bk;  // K % 32 != 0: no MFMA form, the chunk loop folds the norms at three rows
    Bk776.attn.dim = 776;
    run_proj("block_decode_step/dim776_B3", [&] { return block(Bk776, 3, x); });
    auto model_fn = NSA_FN(nsa_model_decode_step);
    const nsa_block_desc two[2] = {Bk, Bk};
    for (int vocab : {131, 4100})
        for (int B_ : {1, 3})
            for (int32_t *next : {(int32_t *)nullptr, next_tokens})
                run_proj("model_decode_step/vocab" + std::to_string(vocab) + "_B" + std::to_string(B_) + (next ? "_next_tokens" : ""), [&] {
                    kv.B = B_;
                    const nsa_kv_desc kvs[2] = {kv, kv};
                    return model_fn(two, kvs, 2, tokens, embed, norm_f_w, lm_head, vocab, logits, next, 100, csc_ptr, csc_rows, csc_vals, S_sel_max, ws, 64 * MB, nullptr);
                });
    // the layer step by batch: the mix rides in the output projection up to 32 rows (DECODE_BAND 3: at any batch)
    for (int B_ : {2, 3, 32, 33})
        run_proj("layer_decode_step/B" + std::to_string(B_) + "_t100", [&] { kv.B = B_; return decode(100); });
    set_tuning("DECODE_BAND", 3);
    run_proj("layer_decode_step/B33_t100_DECODE_BAND_3", [&] { kv.B = 33; return decode(100); });
    set_tuning("DECODE_BAND", -1);
    for (int B_ : {1, 2})
        run_proj("layer_decode_rows/B" + std::to_string(B_) + "_t100_S2", [&] { kv.B = B_; return layer_rows(100, 2); });

    // ---- the attention family: every member of the argument blocks of its launches.  1024 rows (S = 512) are where selection attention
    // stops splitting the keys of a row over waves: the block, row and key-split forms show from there on
    kv.B = 1;
    g_named.insert(g_named.end(), {{"K", K, MB}, {"V", V, MB}, {"lse", lse, MB}, {"dO", dO, MB}, {"dQ", dQ, MB}, {"dK", dK, MB}, {"dV", dV, MB},
                                   {"K_win", kv.K_win, MB}, {"V_win", kv.V_win, MB}, {"K_raw", kv.K_raw, MB}, {"V_raw", kv.V_raw, MB}, {"V_cmp", kv.V_cmp, MB},
                                   {"proj", proj, 4 * MB}, {"O_mix", O_mix, MB}});
    std::vector<Want> attn_blocks;
    for (const char *k : {"sel_attn_fwd_mfma", "sel_attn_blocks_mfma", "sel_attn_rows_mfma"}) {
        attn_blocks.push_back(want<nsa::SelAttnParams>(k, "SelAttnParams"));
        attn_blocks.push_back(want<nsa::SelectParams>(k, "SelectParams", 1));
        attn_blocks.push_back(want<int>(k, "cand", 2));
    }
    for (const char *k : {"sel_attn_combine", "band_attn_combine", "sel_attn_fwd_generic", "sel_head_causal"}) attn_blocks.push_back(want<nsa::SelAttnParams>(k, "SelAttnParams"));
    {
        const char *names[] = {"ml", "acc", "O", "lse"}, *ints[] = {"nbg", "S", "G", "h", "r1", "r2"};
        for (int i = 0; i < 4; ++i) attn_blocks.push_back(want<PtrArg>("sel_attn_ksplit_combine", names[i], i));
        for (int i = 0; i < 6; ++i) attn_blocks.push_back(want<int>("sel_attn_ksplit_combine", ints[i], 4 + i));
        const char *fk_p[] = {"V", "ranges", "O"}, *fk_i[] = {"S", "G", "h", "Dv", "n", "S_kv"}, *fk_l[] = {"vsb", "vsg", "vss"};
        for (int i = 0; i < 3; ++i) attn_blocks.push_back(want<PtrArg>("sel_first_key", fk_p[i], i));
        attn_blocks.push_back(want<int64_t>("sel_first_key", "R", 3));
        for (int i = 0; i < 6; ++i) attn_blocks.push_back(want<int>("sel_first_key", fk_i[i], 4 + i));
        for (int i = 0; i < 3; ++i) attn_blocks.push_back(want<int64_t>("sel_first_key", fk_l[i], 10 + i));
        const char *br_i[] = {"S", "G", "S_kv", "t0", "a", "dd", "c", "w"};
        attn_blocks.push_back(want<PtrArg>("band_ranges", "ranges", 0));
        attn_blocks.push_back(want<int64_t>("band_ranges", "R", 1));
        for (int i = 0; i < 8; ++i) attn_blocks.push_back(want<int>("band_ranges", br_i[i], 2 + i));
    }
    attn_blocks.push_back(want<nsa::DecAttnArgs>("sel_attn_decode_wg", "DecAttnArgs"));
    attn_blocks.push_back(want<PtrArg>("sel_attn_decode_wg", "ranges", 1));
    for (const char *k : {"bwd_dq_rows", "bwd_dq", "bwd_dkdv"}) {
        attn_blocks.push_back(want<nsa::SelAttnBwdParams>(k, "SelAttnBwdParams"));
        attn_blocks.push_back(want<PtrArg>(k, "delta", 1));
    }
    attn_blocks.push_back(want<nsa::SelAttnBwdParams>("sel_attn_bwd_generic", "SelAttnBwdParams"));
    for (const char *k : {"band_attn_fwd(split)", "band_attn_fwd", "band_attn_fwd_generic", "band_attn_fwd_dual", "band_attn_bwd_dq"})
        attn_blocks.push_back(want<nsa::BandAttnParams>(k, "BandAttnParams"));
    attn_blocks.push_back(want<nsa::BandAttnParams>("band_attn_fwd_dual", "BandAttnParams1", 1));
    attn_blocks.push_back(want<unsigned>("band_attn_fwd_dual", "grid0", 2));
    attn_blocks.push_back(want<BandBwdExtraArg>("band_attn_bwd_dq", "BandBwdExtra", 1));
    for (const char *k : {"decode_step", "decode_rows"}) {
        attn_blocks.push_back(want<nsa::DecAttnArgs>(k, "DecAttnArgs", 3));
        attn_blocks.push_back(want<nsa::DecBandPair>(k, "DecBandPair", 4));
    }

    struct AttnCase {
        int B = 1, S = 128, G = 2, h = 6, D = 64, S_kv = 128, n = 16, dtype = NSA_DT_BF16, variant = 0;
        int64_t kss = 0;  // 0: D
        void *O = nullptr, *ws = nullptr;
        float *lse = nullptr;
        size_t ws_bytes = (size_t)64 << 20;
        float scale = 0.f;
        int t0 = 0, a = 0, dd = 1, c = 0, w = 64;  // the band (sliding by default)
    };
    typedef std::function<void(AttnCase &)> AttnTweak;
    auto attn_case = [&](const AttnTweak &tweak) {
        AttnCase c;
        c.O = O;
        c.ws = ws;
        tweak(c);
        if (!c.kss) c.kss = c.D;
        return c;
    };
    auto sel_fwd_case = [&](const char *label, const AttnTweak &tweak) {
        const AttnCase c = attn_case(tweak);
        const int64_t ksg = c.S_kv * c.kss, vsg = (int64_t)c.S_kv * c.D;
        run_args(std::string("sel_attn_fwd/") + label, [&] {
            return fwd(Q, K, V, ranges, c.O, c.lse, c.B, c.S, c.G, c.h, c.D, c.D, c.S_kv, c.n, c.G * ksg, ksg, c.kss, c.G * vsg, vsg, c.D, c.dtype, c.scale, c.variant,
                       c.ws, c.ws_bytes, nullptr);
        }, attn_blocks);
    };
    sel_fwd_case("blocks", [](AttnCase &c) { c.S = c.S_kv = 512; });
    sel_fwd_case("blocks_lse", [&](AttnCase &c) { c.S = c.S_kv = 512; c.lse = lse; });
    sel_fwd_case("split_base_shape", [](AttnCase &) {});
    sel_fwd_case("S1_decode_wg", [](AttnCase &c) { c.S = 1; });
    sel_fwd_case("S1_lse_split", [&](AttnCase &c) { c.S = 1; c.lse = lse; });
    sel_fwd_case("S1_lse_null_workspace", [&](AttnCase &c) { c.S = 1; c.lse = lse; c.ws = nullptr; c.ws_bytes = 0; });
    sel_fwd_case("S1_lse_workspace_8_bytes_off", [&](AttnCase &c) { c.S = 1; c.lse = lse; c.ws = off(ws, 8); });
    sel_fwd_case("S128_Skv32768", [](AttnCase &c) { c.S_kv = 32768; });
    sel_fwd_case("S512_Skv32768_key_split", [](AttnCase &c) { c.S = 512; c.S_kv = 32768; });
    sel_fwd_case("S512_Skv32768_null_workspace", [](AttnCase &c) { c.S = 512; c.S_kv = 32768; c.ws = nullptr; c.ws_bytes = 0; });
    sel_fwd_case("D128_base_shape", [](AttnCase &c) { c.D = 128; });
    sel_fwd_case("D128_S512_rows", [](AttnCase &c) { c.D = 128; c.S = c.S_kv = 512; });
    sel_fwd_case("S512_Skv33280_key_split_rows_in_two", [](AttnCase &c) { c.S = 512; c.S_kv = 33280; });
    sel_fwd_case("S512_kss72_rows", [](AttnCase &c) { c.S = c.S_kv = 512; c.kss = 72; });
    sel_fwd_case("S512_kss72_h16_one_row_per_wave", [](AttnCase &c) { c.S = c.S_kv = 512; c.kss = 72; c.h = 16; });
    sel_fwd_case("variant_1", [](AttnCase &c) { c.variant = 1; });
    sel_fwd_case("f32", [](AttnCase &c) { c.dtype = NSA_DT_F32; });
    sel_fwd_case("h32", [](AttnCase &c) { c.h = 32; });
    sel_fwd_case("O_4_bytes_off", [&](AttnCase &c) { c.O = off(O, 4); });
    sel_fwd_case("S512_O_4_bytes_off", [&](AttnCase &c) { c.S = c.S_kv = 512; c.O = off(O, 4); });
    sel_fwd_case("slab_2GiB", [](AttnCase &c) { c.S_kv = 1 << 20; c.kss = 1024; });
    sel_fwd_case("S1_V_slab_2GiB", [](AttnCase &c) { c.S = 1; c.S_kv = 1 << 24; });
    sel_fwd_case("S1_V_slab_under_2GiB", [](AttnCase &c) { c.S = 1; c.S_kv = (1 << 24) - 1; });

    auto sel_bwd_case = [&](const char *label, const AttnTweak &tweak) {
        const AttnCase c = attn_case(tweak);
        const int64_t sg_ = (int64_t)c.S_kv * c.D;
        run_args(std::string("sel_attn_bwd/") + label, [&] {
            return bwd(Q, K, V, ranges, O, lse, dO, dQ, dK, dV, c.B, c.S, c.G, c.h, c.D, c.D, c.S_kv, c.n, c.G * sg_, sg_, c.D, c.G * sg_, sg_, c.D, c.dtype, c.scale,
                       c.variant, c.ws, c.ws_bytes, nullptr);
        }, attn_blocks);
    };
    sel_bwd_case("mfma_members", [](AttnCase &) {});
    sel_bwd_case("generic_members", [](AttnCase &c) { c.variant = 1; });
    sel_bwd_case("D128_members", [](AttnCase &c) { c.D = 128; c.scale = 0.5f; });

    run_args("sel_attn_first_key_parity/members", [&] {
        return NSA_FN(nsa_sel_attn_first_key_parity)(V, ranges, O, B, S, G, h, D, S_kv, n, sb, sg, D, dt, nullptr);
    }, attn_blocks);
    run_args("sel_attn_first_key_parity/f32", [&] {
        return NSA_FN(nsa_sel_attn_first_key_parity)(V, ranges, O, B, S, G, h, D, S_kv, n, sb, sg, D, NSA_DT_F32, nullptr);
    }, attn_blocks);
    run_args("sel_attn_head_causal_parity/members", [&] {
        return NSA_FN(nsa_sel_attn_head_causal_parity)(Q, K, V, ranges, O, B, S, G, h, D, D, S_kv, n, sb, sg, D, sb, sg, D, dt, 0.f, nullptr);
    }, attn_blocks);

    auto band_fwd_case = [&](const char *label, const AttnTweak &tweak) {
        const AttnCase c = attn_case(tweak);
        const int64_t ksg = c.S_kv * c.kss, vsg = (int64_t)c.S_kv * c.D;
        run_args(std::string("band_attn_fwd/") + label, [&] {
            return bfwd(Q, K, V, c.O, c.lse, c.B, c.S, c.G, c.h, c.D, c.D, c.S_kv, c.G * ksg, ksg, c.kss, c.G * vsg, vsg, c.D, c.t0, c.a, c.dd, c.c, c.w, c.dtype, c.scale,
                        c.variant, c.ws, c.ws_bytes, nullptr);
        }, attn_blocks);
    };
    auto compressed = [](AttnCase &c) { c.t0 = 100; c.a = 32; c.dd = 16; c.c = 1; c.w = 1 << 30; };
    band_fwd_case("sliding_members", [&](AttnCase &c) { c.t0 = 7; c.lse = lse; });
    band_fwd_case("compressed_members", [&](AttnCase &c) { compressed(c); c.S_kv = 13; });
    band_fwd_case("S4096_sliding_members", [&](AttnCase &c) { c.S = c.S_kv = 4096; c.lse = lse; });
    band_fwd_case("S4096_compressed_members", [&](AttnCase &c) { compressed(c); c.t0 = 0; c.S = 4096; c.S_kv = 255; });
    band_fwd_case("S1_split", [&](AttnCase &c) { c.S = 1; c.t0 = 127; });
    band_fwd_case("S1_null_workspace", [&](AttnCase &c) { c.S = 1; c.t0 = 127; c.ws = nullptr; c.ws_bytes = 0; });
    band_fwd_case("slab_2GiB_generic", [](AttnCase &c) { c.S_kv = 1 << 20; c.kss = 1024; });
    band_fwd_case("generic_members", [&](AttnCase &c) { compressed(c); c.S_kv = 13; c.variant = 1; });
    band_fwd_case("w_0", [](AttnCase &c) { c.w = 0; });

    auto band_bwd_case = [&](const char *label, const AttnTweak &tweak) {
        const AttnCase c = attn_case(tweak);
        const int64_t sg_ = (int64_t)c.S_kv * c.D;
        run_args(std::string("band_attn_bwd/") + label, [&] {
            return bbwd(Q, K, V, O, lse, dO, dQ, dK, dV, c.B, c.S, c.G, c.h, c.D, c.D, c.S_kv, c.G * sg_, sg_, c.D, c.G * sg_, sg_, c.D, c.t0, c.a, c.dd, c.c, c.w, c.dtype,
                        c.scale, c.variant, c.ws, c.ws_bytes, nullptr);
        }, attn_blocks);
    };
    band_bwd_case("mfma_members", [&](AttnCase &c) { compressed(c); c.S_kv = 13; });
    band_bwd_case("generic_fallback", [&](AttnCase &c) { compressed(c); c.S_kv = 13; c.variant = 1; });
    band_bwd_case("f32_fallback", [](AttnCase &c) { c.dtype = NSA_DT_F32; });

    for (int S_ : {512, 32768}) {
        set_tuning("SEL_FUSE", 1);
        run_args("sel_select_attn_fwd/S" + std::to_string(S_) + "_SEL_FUSE_members", [&] { return select_attn(K, S_); }, attn_blocks);
        set_tuning("SEL_FUSE", 0);
    }
    run_args("sel_select_attn_fwd/S512_two_launches_members", [&] { return select_attn(K, 512); }, attn_blocks);

    // the layer calls: the attention launches of their three branches
    run_args("layer_prefill/S100_attention", [&] { return prefill(100); }, attn_blocks);
    set_tuning("SEL_FUSE", 1);
    run_args("layer_prefill/S512_SEL_FUSE_attention", [&] { return prefill(512); }, attn_blocks);
    set_tuning("SEL_FUSE", 0);
    run_args("layer_extend/t100_S28_attention", [&] { return extend(100, 28); }, attn_blocks);
    run_args("layer_decode_step/t100_attention", [&] { return decode(100); }, attn_blocks);
    set_tuning("DECODE_STEP", 0);  // the separate launches: the deferred split of the selected branch and the dual band launch
    run_args("layer_decode_step/t100_DECODE_STEP_0_attention", [&] { return decode(100); }, attn_blocks);
    set_tuning("DECODE_WG", 0);
    run_args("layer_decode_step/t100_DECODE_STEP_0_DECODE_WG_0_attention", [&] { return decode(100); }, attn_blocks);
    run_args("layer_decode_rows/t100_S4_DECODE_STEP_0_DECODE_WG_0_attention", [&] { return layer_rows(100, 4); }, attn_blocks);
    set_tuning("DECODE_WG", -1);
    set_tuning("DECODE_STEP", 1);
    run_args("layer_decode_rows/t100_S4_attention", [&] { return layer_rows(100, 4); }, attn_blocks);
    set_tuning("DECODE_ROWS", 0);
    run_args("layer_decode_rows/t100_S4_DECODE_ROWS_0_attention", [&] { return layer_rows(100, 4); }, attn_blocks);
    set_tuning("DECODE_ROWS", -1);
    L.Dk = L.Dv = 128;
    run_args("layer_decode_step/D128_t100_DECODE_STEP_0_attention", [&] { set_tuning("DECODE_STEP", 0); const int rc = decode(100); set_tuning("DECODE_STEP", 1); return rc; }, attn_blocks);
    L.Dk = L.Dv = 64;

    // ---- the step and the rows call: a compressed cache one token short (the step refuses it behind its first launch, the rows call before
    // any), and the tail blocks of every form of the two that runs (tail_fields)
    kv.n_cmp_max = ncmp(101) - 1;
    run("layer_decode_step/t100_n_cmp_max_one_short", [&] { return decode(100); });
    run("layer_decode_rows/t100_S4_n_cmp_max_one_short", [&] { return layer_rows(100, 4); });
    kv.n_cmp_max = 63;
    g_named.insert(g_named.end(), {{"gate_w1", L.gate_w1, MB}, {"gate_b1", L.gate_b1, MB}, {"gate_w2", L.gate_w2, MB}, {"gate_b2", L.gate_b2, MB}});
    auto tail = [&](const std::string &label, const std::function<int()> &call) {
        run((label + "_tail").c_str(), call, [&] { return tail_fields(call); });
    };
    for (int D_ : {64, 128}) {
        L.Dk = L.Dv = D_;
        const std::string at = D_ == 128 ? "D128_" : "";
        tail("layer_decode_step/" + at + "t100", [&] { return decode(100); });
        tail("layer_decode_rows/" + at + "t100_S4", [&] { return layer_rows(100, 4); });
    }
    L.Dk = L.Dv = 64;
    tail("layer_decode_step/t31_first_compressed_token", [&] { return decode(31); });
    tail("layer_decode_step/t5_no_compressed_token", [&] { return decode(5); });
    tail("layer_decode_rows/t100_S1", [&] { return layer_rows(100, 1); });
    tail("layer_decode_rows/t30_S4_pooling", [&] { return layer_rows(30, 4); });
    for (int band : {0, 1}) {
        set_tuning("DECODE_BAND", band);
        tail("layer_decode_step/t100_DECODE_BAND_" + std::to_string(band), [&] { return decode(100); });
    }
    set_tuning("DECODE_BAND", -1);
    set_tuning("DECODE_STEP", 0);
    tail("layer_decode_step/t100_DECODE_STEP_0", [&] { return decode(100); });
    set_tuning("DECODE_STEP", 1);
    set_tuning("DECODE_ROWS", 0);
    tail("layer_decode_rows/t100_S4_DECODE_ROWS_0", [&] { return layer_rows(100, 4); });
    set_tuning("DECODE_ROWS", -1);
    for (int B_ : {2, 32, 33}) tail("layer_decode_step/B" + std::to_string(B_) + "_t100", [&] { kv.B = B_; return decode(100); });
    tail("layer_decode_rows/B2_t100_S2", [&] { kv.B = 2; return layer_rows(100, 2); });
    kv.B = 1;
    printf("\n}\n");
    return 0;
}
