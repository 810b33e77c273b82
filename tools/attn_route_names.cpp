// Which kernels does an attention call launch?  Host program in the manner of csrc/dispatch_check.cpp (no GPU): it loads the library, answers
// the HIP calls of its host code itself (no kernel runs) and notes the device name that every kernel was registered under, so that each
// launch can be printed by its template instance.  Reads one case per line from stdin, as `tests/attention_bits_probe.py --routes` prints them:
//   case=NAME entry=sel|fuse|band|selbwd|bandbwd dt= B= S= G= h= D= S_kv= pad= [n= lse= S_sel= mode= t0= a= dd= c= w=] sw=SWITCH:VALUE,...
// and, for `tests/scorer_bits_probe.py --routes`, entry=scores|scoresel (S_kv = S_cmp, skip = causal_skip, t0 = q0, norm; l / d / l' = 32 / 16 / 64)
// and prints per case: NAME <tab> kernel [map_mode=..] [cand=..] | kernel ...
//   hipcc -x c++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/attn_route_names.cpp -o ab/attn_route_names -rdynamic -ldl
//   python tests/attention_bits_probe.py --routes | ab/attn_route_names nsa_vibe_amd/libnsa_sel_hip.so > routes.txt
//   python tests/attention_bits_probe.py --check-routes routes.txt
#include <cxxabi.h>
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../include/nsa_sel_hip.h"
#include "../nsa_vibe_amd/csrc/sel_attn_params.hpp"

static std::map<const void *, std::string> g_name;
static std::vector<std::string> g_launched;
static std::vector<dim3> g_grid, g_block;
static std::vector<size_t> g_shmem;

static std::string demangled(std::string m) {
    // (the demangler may not know the 16-bit float manglings: two unused builtin codes stand in for them, as in tools/isa_compare.py)
    for (auto [from, to] : {std::pair<const char *, const char *>{"DF16_", "Dh"}, {"DF16b", "De"}})
        for (size_t p; (p = m.find(from)) != std::string::npos;) m.replace(p, strlen(from), to);
    int st = 0;
    char *d = abi::__cxa_demangle(m.c_str(), nullptr, nullptr, &st);
    std::string s = st == 0 && d ? d : m;
    free(d);
    for (auto [from, to] : {std::pair<const char *, const char *>{"decimal128", "__bf16"}, {"half", "_Float16"}, {"nsa::", ""}, {"void ", ""}})
        for (size_t p; (p = s.find(from)) != std::string::npos;) s.replace(p, strlen(from), to);
    return s.substr(0, s.find('('));
}

extern "C" {
#define EXPORT __attribute__((visibility("default")))
EXPORT void __hipRegisterFunction(void **modules, const void *host, char *dev, const char *name, unsigned limit, void *tid, void *bid, void *bdim, void *gdim,
                                  int *wsize) {
    g_name[host] = demangled(name);
    using Fn = void (*)(void **, const void *, char *, const char *, unsigned, void *, void *, void *, void *, int *);
    ((Fn)dlsym(RTLD_NEXT, "__hipRegisterFunction"))(modules, host, dev, name, limit, tid, bid, bdim, gdim, wsize);
}
EXPORT hipError_t hipMalloc(void **p, size_t n) { return (*p = calloc(1, n + 256)) ? hipSuccess : hipErrorOutOfMemory; }
EXPORT hipError_t hipFree(void *p) { return free(p), hipSuccess; }
EXPORT hipError_t hipMemsetAsync(void *, int, size_t, hipStream_t) { return hipSuccess; }
EXPORT hipError_t hipMemsetD32Async(hipDeviceptr_t, int, size_t, hipStream_t) { return hipSuccess; }
EXPORT hipError_t hipGetLastError(void) { return hipSuccess; }
EXPORT const char *hipGetErrorString(hipError_t) { return "error"; }
EXPORT hipError_t hipGetDevice(int *dev) { return *dev = 0, hipSuccess; }
EXPORT hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) { return *v = 256, hipSuccess; }
EXPORT hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
EXPORT hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t) {
    g_grid.push_back(grid), g_block.push_back(block), g_shmem.push_back(shmem);
    return hipSuccess;
}
EXPORT hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *shmem, hipStream_t *stream) {
    *grid = g_grid.back(), *block = g_block.back(), *shmem = g_shmem.back(), *stream = nullptr;
    g_grid.pop_back(), g_block.pop_back(), g_shmem.pop_back();
    return hipSuccess;
}
EXPORT hipError_t hipLaunchKernel(const void *fn, dim3, dim3, void **args, size_t, hipStream_t) {
    std::string s = g_name.count(fn) ? g_name[fn] : "?";
    auto starts = [&](const char *p) { return s.rfind(p, 0) == 0; };
    if (starts("sel_attn_fwd_mfma_kernel") || starts("sel_attn_rows_mfma_kernel") || starts("sel_attn_blocks_mfma_kernel")) {
        const nsa::SelAttnParams *P = (const nsa::SelAttnParams *)args[0];
        s += " map_mode=" + std::to_string(P->map_mode);
        if (P->fuse_select) s += " cand=" + std::to_string(*(const int *)args[2]);
    } else if (starts("band_attn_fwd_kernel") || starts("band_attn_bwd_dq_kernel")) {
        s += " map_mode=" + std::to_string(((const nsa::BandAttnParams *)args[0])->map_mode);
    } else if (starts("bwd_dq_kernel") || starts("bwd_dq_rows_kernel")) {
        s += " map_mode=" + std::to_string(*(const int *)args[2]);
    }
    g_launched.push_back(s);
    return hipSuccess;
}
}

int main(int argc, char **argv) {
    void *lib = argc > 1 ? dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL) : nullptr;
    if (!lib) return fprintf(stderr, "usage: attn_route_names <libnsa_sel_hip.so> < cases   (%s)\n", dlerror()), 2;
#define FN(name) ((decltype(&name))dlsym(lib, #name))
    std::string line;
    while (std::getline(std::cin, line)) {
        std::map<std::string, std::string> kv;
        std::istringstream is(line);
        for (std::string tok; is >> tok;) kv[tok.substr(0, tok.find('='))] = tok.substr(tok.find('=') + 1);
        if (!kv.count("case")) continue;
        auto I = [&](const char *k) { return kv.count(k) ? atoi(kv[k].c_str()) : 0; };
        std::vector<std::pair<std::string, int>> saved;  // every switch goes back to the value it had
        std::istringstream sw(kv["sw"]);
        for (std::string tok; std::getline(sw, tok, ',');)
            if (tok.find(':') != std::string::npos) {
                saved.push_back({tok.substr(0, tok.find(':')), 0});
                FN(nsa_hip_get_tuning)(saved.back().first.c_str(), &saved.back().second);
                FN(nsa_hip_set_tuning)(saved.back().first.c_str(), atoi(tok.c_str() + tok.find(':') + 1));
            }
        const int dt = I("dt"), B = I("B"), S = I("S"), G = I("G"), h = I("h"), D = I("D"), S_kv = I("S_kv"), n = I("n"), Dw = D + I("pad");
        const int64_t ss = Dw, sg = (int64_t)S_kv * Dw, sb = sg * G;
        const size_t rows = (size_t)B * S * G;
        auto mem = [](size_t bytes) {  // zeroed, 256-byte aligned host memory that nothing reads
            bytes = (bytes + 511) & ~(size_t)255;
            return memset(aligned_alloc(256, bytes), 0, bytes);
        };
        void *Q = mem(rows * h * D * 2), *O = mem(rows * h * D * 2), *dO = mem(rows * h * D * 2), *dQ = mem(rows * h * D * 2);
        void *K = mem((size_t)B * sb * 2), *V = mem((size_t)B * sb * 2), *dK = mem((size_t)B * G * S_kv * D * 4), *dV = mem((size_t)B * G * S_kv * D * 4);
        void *rg = mem(rows * 64 * 2 * 4), *lse = mem(rows * h * 4), *pg = mem(rows * (size_t)(I("S_sel") + 1) * 4), *ws = nullptr;
        const std::string e = kv["entry"];
        size_t need = 0;
        int rc = -1;
        g_launched.clear();
        if (e == "sel") {
            need = FN(nsa_sel_attn_fwd_workspace_kv)(B, S, G, h, D, D, S_kv, n, dt);
            ws = mem(need);
            rc = FN(nsa_sel_attn_fwd)(Q, K, V, (const int32_t *)rg, O, I("lse") ? (float *)lse : nullptr, B, S, G, h, D, D, S_kv, n, sb, sg, ss, sb, sg, ss, dt, 0.f, 2,
                                      need ? ws : nullptr, need, nullptr);
        } else if (e == "fuse") {
            const int md = I("mode"), W = md == NSA_SEL_BATCHED ? FN(nsa_batched_ranges_width)(S, I("S_sel"), 64, 6, 1, 2) : 6;
            need = FN(nsa_sel_attn_fwd_workspace_kv)(B, S, G, h, D, D, S_kv, W, dt);
            ws = mem(need);
            rc = FN(nsa_sel_select_attn_fwd)((const float *)pg, I("t0"), nullptr, I("S_sel"), 64, 6, 1, 2, md, S, (int32_t *)rg, W, Q, K, V, O, (float *)lse, B, S, G, h,
                                             D, D, S_kv, sb, sg, ss, sb, sg, ss, dt, 0.f, need ? ws : nullptr, need, nullptr);
        } else if (e == "band") {
            need = FN(nsa_band_attn_fwd_workspace)(B, S, G, h, D, D, dt);
            ws = mem(need);
            rc = FN(nsa_band_attn_fwd)(Q, K, V, O, (float *)lse, B, S, G, h, D, D, S_kv, sb, sg, ss, sb, sg, ss, I("t0"), I("a"), I("dd"), I("c"), I("w"), dt, 0.f, 2,
                                       need ? ws : nullptr, need, nullptr);
        } else if (e == "selbwd") {
            need = FN(nsa_sel_attn_bwd_workspace)(B, S, G, h, D, D, S_kv, dt, 2);
            ws = mem(need);
            rc = FN(nsa_sel_attn_bwd)(Q, K, V, (const int32_t *)rg, O, (const float *)lse, dO, dQ, (float *)dK, (float *)dV, B, S, G, h, D, D, S_kv, n, sb, sg, ss, sb, sg,
                                      ss, dt, 0.f, 2, ws, need, nullptr);
        } else if (e == "bandbwd") {
            need = FN(nsa_band_attn_bwd_workspace)(B, S, G, h, D, D, S_kv, dt, 2);
            ws = mem(need);
            rc = FN(nsa_band_attn_bwd)(Q, K, V, O, (const float *)lse, dO, dQ, (float *)dK, (float *)dV, B, S, G, h, D, D, S_kv, sb, sg, ss, sb, sg, ss, I("t0"), I("a"),
                                       I("dd"), I("c"), I("w"), dt, 0.f, 2, ws, need, nullptr);
        } else if (e == "scores") {  // the scorer alone, variant 2 (no workspace)
            rc = FN(nsa_sel_scores_rows)(Q, K, (float *)pg, B, S, G, h, D, S_kv, sb, sg, ss, (const int32_t *)rg, (const int32_t *)rg, (const float *)lse, I("S_sel"), 32, 16,
                                         64, I("skip"), 2, dt, 0.f, I("t0"), I("norm"), nullptr, 0, nullptr);
        } else if (e == "scoresel") {  // scorer + top-16 selection in one call
            const int md = I("mode"), W = md == NSA_SEL_BATCHED ? FN(nsa_batched_ranges_width)(S, I("S_sel"), 64, 16, 1, 2) : 16;
            for (int v : {0, 1}) need = std::max(need, FN(nsa_sel_scores_rows_workspace)(B, S, G, h, D, S_kv, I("S_sel"), 32, 16, 64, dt, v, I("norm")));
            ws = mem(need);
            rc = FN(nsa_sel_scores_select_rows)(Q, K, (float *)pg, B, S, G, h, D, S_kv, sb, sg, ss, (const int32_t *)rg, (const int32_t *)rg, (const float *)lse, I("S_sel"),
                                                32, 16, 64, I("skip"), dt, 0.f, I("t0"), 16, 1, 2, md, S, (int32_t *)O, W, I("t0"), I("norm"), need ? ws : nullptr, need,
                                                nullptr);
        }
        printf("%s\t", kv["case"].c_str());
        if (rc) printf("rc=%d %s", rc, FN(nsa_hip_last_error)());
        for (size_t i = 0; i < g_launched.size(); ++i) printf("%s%s", i ? " | " : "", g_launched[i].c_str());
        printf("\n");
        for (auto it = saved.rbegin(); it != saved.rend(); ++it) FN(nsa_hip_set_tuning)(it->first.c_str(), it->second);
        for (void *p : {Q, K, V, O, dO, dQ, rg, lse, dK, dV, pg, ws}) free(p);
    }
    return 0;
}
