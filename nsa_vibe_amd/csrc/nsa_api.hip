// C ABI of libnsa_sel_hip.so (see include/nsa_sel_hip.h).  Host-side argument checking,
// error reporting and kernel dispatch; no torch types, no allocation, no synchronisation.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <stdlib.h>
#include <strings.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "nsa_host.hpp"
#include "nsa_internal.hpp"
#include "sel_select_row.hpp"

namespace nsa {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char *what) {
    set_error("HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
    return NSA_ERR_HIP;
}

// ---- tuning switches -------------------------------------------------------------------------
static std::atomic<int> g_tune[TUNE_COUNT];
static std::once_flag g_tune_once;

static void tune_init() {
    for (int i = 0; i < TUNE_COUNT; ++i) {
        char name[64];
        snprintf(name, sizeof(name), "NSA_HIP_%s", TUNE_TABLE[i].name);
        const char *e = getenv(name);
        int v = e ? atoi(e) : TUNE_TABLE[i].def;
#ifndef NSA_DEC_TS
        if (i == TUNE_DECODE_STOP) v = 0;  // TIMELINE build only (see nsa_hip_set_tuning)
#endif
        g_tune[i].store(v, std::memory_order_relaxed);
    }
}

int tuning(Tune t) {
    std::call_once(g_tune_once, tune_init);
    return g_tune[t].load(std::memory_order_relaxed);
}

static int tune_index(const char *name) {
    if (!name) return -1;
    if (strncmp(name, "NSA_HIP_", 8) == 0) name += 8;
    for (int i = 0; i < TUNE_COUNT; ++i)
        if (strcasecmp(name, TUNE_TABLE[i].name) == 0) return i;
    return -1;
}

}  // namespace nsa

using namespace nsa;

extern "C" {

int nsa_hip_abi_version(void) { return NSA_HIP_ABI_VERSION; }

const char *nsa_hip_last_error(void) { return g_err; }

int nsa_hip_set_tuning(const char *name, int value) {
    const int i = tune_index(name);
    NSA_CHECK_ARG(i >= 0, "unknown tuning switch '%s'", name ? name : "(null)");
#ifndef NSA_DEC_TS
    // the phase stops of the fused decode kernel leave O and the ranges unwritten: they exist in the TIMELINE build only
    NSA_CHECK_ARG(i != TUNE_DECODE_STOP || value == 0, "DECODE_STOP is a measurement aid of the TIMELINE build (make TIMELINE=1)");
#endif
    std::call_once(g_tune_once, tune_init);
    g_tune[i].store(value, std::memory_order_relaxed);
    return NSA_OK;
}

int nsa_hip_get_tuning(const char *name, int *value) {
    const int i = tune_index(name);
    NSA_CHECK_ARG(i >= 0 && value, "unknown tuning switch '%s'", name ? name : "(null)");
    *value = tuning((Tune)i);
    return NSA_OK;
}

int nsa_hip_device_check(int dev, int *cu_count, size_t *hbm_bytes) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= dev || dev < 0) {
        set_error("no HIP device %d (count %d)", dev, n);
        return NSA_ERR_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    NSA_HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s, this library is built for gfx950 only", dev, prop.gcnArchName);
        return NSA_ERR_NO_DEVICE;
    }
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
    return NSA_OK;
}

// ------------------------------------------------------------------------------ attention
size_t nsa_sel_attn_fwd_workspace_kv(int B, int S, int G, int h, int Dk, int Dv, int S_kv, int n_ranges, int dtype) {
    AttnCall c{};  // the shape alone: no tensors, the route of variant 0
    c.B = B; c.S = S; c.G = G; c.h = h; c.Dk = Dk; c.Dv = Dv; c.S_kv = S_kv; c.n = n_ranges; c.dtype = dtype;
    if (!sel_attn_route(c).fast_ok) return 0;
    const size_t split_kv = sel_attn_mfma_workspace(c.rows(), h, Dv, nullptr);
    // key-split form of the block kernel (long contexts): its zones follow the rows' positions S_kv - S + row
    const size_t key_split = sel_attn_ksplit_workspace(dtype, h, Dk, Dv, S, S_kv > S ? S_kv : S, n_ranges, c.rows());
    return split_kv > key_split ? split_kv : key_split;
}

size_t nsa_sel_attn_fwd_workspace(int B, int S, int G, int h, int Dk, int Dv, int n_ranges, int dtype) {
    return nsa_sel_attn_fwd_workspace_kv(B, S, G, h, Dk, Dv, S, n_ranges, dtype);  // the prefill case S_kv = S
}

}  // extern "C"

AttnRoute nsa::sel_attn_route(const AttnCall &c) {
    AttnRoute r{AttnRoute::GENERIC, AttnRoute::WS_NONE, attn_mfma_shape_ok(c.dtype, c.h, c.Dk, c.Dv) && qkv_aligned(c), 1};
    const size_t need = r.fast_ok ? sel_attn_mfma_workspace(c.rows(), c.h, c.Dv, &r.nsplit) : 0;
    if (c.S_kv == 0 || c.n == 0) {
        r.kind = AttnRoute::ZERO_FILL;
    } else if (c.variant == 0 && c.S == 1 && !c.lse && sel_attn_decode_wg_supported(c) && (int64_t)c.S_kv * 2 * c.Dv < ((int64_t)1 << 31)) {
        r.kind = AttnRoute::DECODE_WG;  // decode: one workgroup per row, partials merged through LDS, no combine launch
    } else if (c.variant == 2 || (c.variant == 0 && r.fast_ok)) {
        r.kind = AttnRoute::MFMA;
        if (c.ws && ((uintptr_t)c.ws % 16 == 0) && (r.nsplit == 1 || c.ws_bytes >= need)) r.ws = r.nsplit > 1 ? AttnRoute::WS_SPLIT : AttnRoute::WS_KSPLIT;
    }
    return r;
}

// the block of a call on the MFMA route
static SelAttnParams sel_attn_mfma_params(const AttnCall &c, const AttnRoute &r, int defer) {
    SelAttnParams P = sel_attn_params(c);
    P.nsplit = 1;
    if (r.ws == AttnRoute::WS_SPLIT) {
        P.part = (float *)c.ws;
        P.nsplit = r.nsplit;
        P.defer_combine = defer;
    } else if (r.ws == AttnRoute::WS_KSPLIT) {
        P.ks_ws = c.ws;
        P.ks_bytes = c.ws_bytes;
    }
    return P;
}

int nsa::sel_attn_fwd_impl(const AttnCall &c, int defer, int *ns_used) {
    if (ns_used) *ns_used = 1;
    NSA_CHECK_ARG(dtype_ok(c.dtype), "sel_attn_fwd: unknown dtype %d", c.dtype);
    NSA_CHECK_ARG(c.B >= 0 && c.S >= 0 && c.G >= 1 && c.h >= 1 && c.Dk >= 1 && c.Dv >= 1 && c.S_kv >= 0 && c.n >= 0, "sel_attn_fwd: negative size");
    NSA_CHECK_ARG(c.n <= 64, "sel_attn_fwd: at most 64 ranges per row are supported (got %d)", c.n);
    NSA_CHECK_ARG(c.Dk <= 256 && c.Dv <= 256, "sel_attn_fwd: Dk/Dv up to 256 supported (got %d/%d)", c.Dk, c.Dv);
    const int64_t R = c.rows();
    if (R == 0) return NSA_OK;
    NSA_CHECK_ARG(c.Q && c.O && c.ranges || c.n == 0, "sel_attn_fwd: null pointer");
    NSA_CHECK_ARG((c.K && c.V) || c.S_kv == 0, "sel_attn_fwd: null K/V");
    const AttnRoute r = sel_attn_route(c);
    if (r.kind == AttnRoute::ZERO_FILL) {
        if (int rc = zero_rows(c.O, R, c.h, c.Dv, c.dtype, c.st)) return rc;
        if (c.lse) NSA_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)c.lse, (int)0xff800000, (size_t)R * c.h, c.st));  // lse = -inf (its bit pattern)
        return NSA_OK;
    }
    if (c.variant == 2) NSA_CHECK_ARG(r.fast_ok, "sel_attn_fwd: MFMA variant requested but shape/dtype/alignment unsupported");
    NSA_CHECK_ARG(c.variant >= 0 && c.variant <= 2, "sel_attn_fwd: unknown variant %d", c.variant);
    const SelAttnParams P = sel_attn_mfma_params(c, r, defer);
    if (ns_used && defer) *ns_used = P.nsplit;
    if (r.kind == AttnRoute::DECODE_WG) return launch_sel_attn_decode_wg(P, c.dtype, c.st);
    if (r.kind == AttnRoute::MFMA) return launch_sel_attn_fwd_mfma(P, c.dtype, c.st);
    return launch_sel_attn_fwd_generic(P, c.dtype, c.st);
}

// the two parity modes: their checks, the rows that select nothing, their one launch (qk: the mode reads Q and K too)
static int parity_mode(const char *who, bool qk, int (*launch)(const SelAttnParams &, int, hipStream_t), const AttnCall &c) {
    NSA_CHECK_ARG(dtype_ok(c.dtype), "%s: unknown dtype %d", who, c.dtype);
    NSA_CHECK_ARG(c.B >= 0 && c.S >= 0 && c.G >= 1 && c.h >= 1 && c.Dk >= 1 && c.Dv >= 1 && c.S_kv >= 0 && c.n >= 0, "%s: negative size", who);
    NSA_CHECK_ARG(c.n <= 64, "%s: at most 64 ranges per row are supported (got %d)", who, c.n);
    if (c.rows() == 0) return NSA_OK;
    NSA_CHECK_ARG((c.Q || !qk) && c.O && (c.ranges || c.n == 0) && (((c.K || !qk) && c.V) || c.S_kv == 0), "%s: null pointer", who);
    if (c.S_kv == 0 || c.n == 0) return zero_rows(c.O, c.rows(), c.h, c.Dv, c.dtype, c.st);
    return launch(sel_attn_params(c), c.dtype, c.st);
}

extern "C" {

int nsa_sel_attn_fwd(const void *Q, const void *K, const void *V, const int32_t *ranges, void *O, float *lse, int B,
                     int S, int G, int h, int Dk, int Dv, int S_kv, int n_ranges, int64_t ksb, int64_t ksg,
                     int64_t kss, int64_t vsb, int64_t vsg, int64_t vss, int dtype, float scale, int variant,
                     void *workspace, size_t workspace_bytes, void *stream) {
    return sel_attn_fwd_impl(AttnCall{Q, K, V, ranges, O, lse, B, S, G, h, Dk, Dv, S_kv, n_ranges, ksb, ksg, kss, vsb, vsg, vss, dtype, scale, variant,
                                      workspace, workspace_bytes, (hipStream_t)stream},
                             0, nullptr);
}

int nsa_sel_attn_first_key_parity(const void *V, const int32_t *ranges, void *O, int B, int S, int G, int h, int Dv, int S_kv, int n_ranges,
                                  int64_t vsb, int64_t vsg, int64_t vss, int dtype, void *stream) {
    // (no Q, no K: the mode copies rows of V; Dk and the scale are not read)
    return parity_mode("sel_attn_first_key_parity", false, launch_sel_first_key,
                       AttnCall{nullptr, nullptr, V, ranges, O, nullptr, B, S, G, h, Dv, Dv, S_kv, n_ranges, 0, 0, 0, vsb, vsg, vss, dtype, 1.f, 0, nullptr, 0, (hipStream_t)stream});
}

int nsa_sel_attn_head_causal_parity(const void *Q, const void *K, const void *V, const int32_t *ranges, void *O, int B, int S, int G, int h,
                                    int Dk, int Dv, int S_kv, int n_ranges, int64_t ksb, int64_t ksg, int64_t kss, int64_t vsb, int64_t vsg,
                                    int64_t vss, int dtype, float scale, void *stream) {
    return parity_mode("sel_attn_head_causal_parity", true, launch_sel_head_causal,
                       AttnCall{Q, K, V, ranges, O, nullptr, B, S, G, h, Dk, Dv, S_kv, n_ranges, ksb, ksg, kss, vsb, vsg, vss, dtype, scale, 0, nullptr, 0, (hipStream_t)stream});
}

size_t nsa_sel_attn_bwd_workspace(int B, int S, int G, int h, int Dk, int Dv, int S_kv, int dtype, int variant) {
    if (variant == 1 || !attn_mfma_shape_ok(dtype, h, Dk, Dv)) return 0;
    return sel_attn_bwd_mfma_workspace((int64_t)B * S * G, h, S, (int64_t)B * G, S_kv, Dk);
}

}  // extern "C"

// what both MFMA backwards ask beyond the route of their forward: the shape, aligned operands, O and dO read in 16-byte pieces, one launch
static bool bwd_mfma_ok(const AttnCall &c, const AttnGrads &g) {
    return attn_mfma_shape_ok(c.dtype, c.h, c.Dk, c.Dv) && qkv_aligned(c) && ((uintptr_t)g.dO % 16 == 0) && ((uintptr_t)c.O % 16 == 0) &&
           (int64_t)c.B * c.G <= 65535;
}

int nsa::sel_attn_bwd_impl(const AttnCall &c, const AttnGrads &g) {
    NSA_CHECK_ARG(dtype_ok(c.dtype), "sel_attn_bwd: unknown dtype %d", c.dtype);
    NSA_CHECK_ARG(c.B >= 0 && c.S >= 0 && c.G >= 1 && c.h >= 1 && c.Dk >= 1 && c.Dv >= 1 && c.S_kv >= 0 && c.n >= 0, "sel_attn_bwd: negative size");
    NSA_CHECK_ARG(c.n <= 64, "sel_attn_bwd: at most 64 ranges per row");
    NSA_CHECK_ARG(c.Dk <= 256 && c.Dv <= 256, "sel_attn_bwd: Dk/Dv up to 256 supported");
    NSA_CHECK_ARG(c.variant >= 0 && c.variant <= 2, "sel_attn_bwd: unknown variant %d", c.variant);
    const int64_t R = c.rows(), nbg = (int64_t)c.B * c.G;
    const bool empty = R == 0 || c.S_kv == 0 || c.n == 0;
    const bool fast_ok = !empty && bwd_mfma_ok(c, g) && c.ws && c.ws_bytes >= sel_attn_bwd_mfma_workspace(R, c.h, c.S, nbg, c.S_kv, c.Dk) &&
                         ((uintptr_t)c.ws % 16 == 0);
    if (c.variant == 2) NSA_CHECK_ARG(fast_ok, "sel_attn_bwd: MFMA variant requested but shape/dtype/alignment/workspace unsupported");
    const bool fast = fast_ok && c.variant != 1;
    if (!fast && nbg * c.S_kv > 0) {  // the generic kernel accumulates with atomics; the MFMA route writes every element
        NSA_HIP_TRY(hipMemsetAsync(g.dK, 0, sizeof(float) * (size_t)nbg * c.S_kv * c.Dk, c.st));
        NSA_HIP_TRY(hipMemsetAsync(g.dV, 0, sizeof(float) * (size_t)nbg * c.S_kv * c.Dv, c.st));
    }
    if (R == 0) return NSA_OK;
    if (c.S_kv == 0 || c.n == 0) {
        NSA_HIP_TRY(hipMemsetAsync(g.dQ, 0, (size_t)R * c.h * c.Dk * esize(c.dtype), c.st));
        return NSA_OK;
    }
    NSA_CHECK_ARG(c.Q && c.K && c.V && c.ranges && c.O && c.lse && g.dO && g.dQ && g.dK && g.dV, "sel_attn_bwd: null pointer");
    const SelAttnBwdParams P = sel_attn_bwd_params(c, g);
    if (fast) return launch_sel_attn_bwd_mfma(P, c.dtype, (float *)c.ws, c.st);
    return launch_sel_attn_bwd_generic(P, c.dtype, c.st);
}

AttnRoute nsa::band_attn_route(const AttnCall &c, const Band &band) {
    AttnRoute r{AttnRoute::GENERIC, AttnRoute::WS_NONE,
                c.S_kv > 0 && band.w > 0 && attn_mfma_shape_ok(c.dtype, c.h, c.Dk, c.Dv) && qkv_aligned(c) && out_aligned(c) && slabs_under_2gib(c), 1};
    const size_t need = band_attn_workspace(c.B, c.S, c.G, c.h, c.Dk, c.Dv, c.dtype, &r.nsplit);
    if (r.fast_ok && c.variant != 1) r.kind = AttnRoute::MFMA;
    if (r.kind == AttnRoute::MFMA && r.nsplit > 1 && c.ws && ((uintptr_t)c.ws % 16 == 0) && c.ws_bytes >= need) r.ws = AttnRoute::WS_SPLIT;
    return r;
}

int nsa::band_attn_fwd_impl(const AttnCall &c, const Band &band, int defer, int *ns_used) {
    if (ns_used) *ns_used = 1;
    NSA_CHECK_ARG(dtype_ok(c.dtype), "band_attn_fwd: unknown dtype %d", c.dtype);
    NSA_CHECK_ARG(c.B >= 0 && c.S >= 0 && c.G >= 1 && c.h >= 1 && c.Dk >= 1 && c.Dv >= 1 && c.S_kv >= 0, "band_attn_fwd: negative size");
    NSA_CHECK_ARG(band.t0 >= 0 && band.dd >= 1 && band.w >= 0, "band_attn_fwd: need t0 >= 0, dd >= 1, w >= 0");
    NSA_CHECK_ARG(c.variant >= 0 && c.variant <= 2, "band_attn_fwd: unknown variant %d", c.variant);
    if (c.rows() == 0) return NSA_OK;
    // S_kv == 0 or w == 0: every interval is empty; the generic kernel writes the zeros / -inf rows
    NSA_CHECK_ARG(c.Q && c.O && ((c.K && c.V) || c.S_kv == 0), "band_attn_fwd: null pointer");
    BandAttnParams P = band_attn_params(c, band);
    const AttnRoute r = band_attn_route(c, band);
    if (c.variant == 2) NSA_CHECK_ARG(r.fast_ok, "band_attn_fwd: MFMA variant requested but shape/dtype/alignment unsupported");
    if (r.kind != AttnRoute::MFMA) return launch_band_attn_fwd_generic(P, c.dtype, c.st);
    if (r.ws == AttnRoute::WS_SPLIT) {
        P.part = (float *)c.ws;
        P.nsplit = r.nsplit;
        P.defer_combine = defer;
        if (ns_used && defer) *ns_used = r.nsplit;
    }
    return launch_band_attn_fwd_mfma(P, c.dtype, c.st);
}

extern "C" {

int nsa_sel_attn_bwd(const void *Q, const void *K, const void *V, const int32_t *ranges, const void *O,
                     const float *lse, const void *dO, void *dQ, float *dK, float *dV, int B, int S, int G, int h,
                     int Dk, int Dv, int S_kv, int n_ranges, int64_t ksb, int64_t ksg, int64_t kss, int64_t vsb,
                     int64_t vsg, int64_t vss, int dtype, float scale, int variant, void *workspace, size_t workspace_bytes,
                     void *stream) {
    return sel_attn_bwd_impl(AttnCall{Q, K, V, ranges, (void *)O, (float *)lse, B, S, G, h, Dk, Dv, S_kv, n_ranges, ksb, ksg, kss, vsb, vsg, vss, dtype, scale,
                                      variant, workspace, workspace_bytes, (hipStream_t)stream},
                             AttnGrads{dO, dQ, dK, dV});
}

// ------------------------------------------------------------------------------ band attention
size_t nsa_band_attn_fwd_workspace(int B, int S, int G, int h, int Dk, int Dv, int dtype) {
    return band_attn_workspace(B, S, G, h, Dk, Dv, dtype, nullptr);
}

int nsa_band_attn_fwd(const void *Q, const void *K, const void *V, void *O, float *lse, int B, int S, int G, int h, int Dk,
                      int Dv, int S_kv, int64_t ksb, int64_t ksg, int64_t kss, int64_t vsb, int64_t vsg, int64_t vss, int t0,
                      int a, int dd, int c, int w, int dtype, float scale, int variant, void *workspace, size_t workspace_bytes,
                      void *stream) {
    return band_attn_fwd_impl(AttnCall{Q, K, V, nullptr, O, lse, B, S, G, h, Dk, Dv, S_kv, 0, ksb, ksg, kss, vsb, vsg, vss, dtype, scale, variant, workspace,
                                       workspace_bytes, (hipStream_t)stream},
                              Band{t0, a, dd, c, w}, 0, nullptr);
}

// Band attention backward.  dQ: dense 48-slot kernel (MFMA route); dK/dV: the key-block-major selection backward kernels fed
// with the band as one range per row.  workspace = selection-backward workspace (its delta area is shared) + the ranges.
static size_t band_bwd_ranges_off(int B, int S, int G, int h, int Dk, int Dv, int S_kv, int dtype, int variant) {
    return (nsa_sel_attn_bwd_workspace(B, S, G, h, Dk, Dv, S_kv, dtype, variant) + 255) & ~(size_t)255;
}

size_t nsa_band_attn_bwd_workspace(int B, int S, int G, int h, int Dk, int Dv, int S_kv, int dtype, int variant) {
    return band_bwd_ranges_off(B, S, G, h, Dk, Dv, S_kv, dtype, variant) + sizeof(int32_t) * 2 * (size_t)B * S * G;
}

int nsa_band_attn_bwd(const void *Q, const void *K, const void *V, const void *O, const float *lse, const void *dO, void *dQ, float *dK,
                      float *dV, int B, int S, int G, int h, int Dk, int Dv, int S_kv, int64_t ksb, int64_t ksg, int64_t kss, int64_t vsb,
                      int64_t vsg, int64_t vss, int t0, int a, int dd, int c, int w, int dtype, float scale, int variant, void *workspace,
                      size_t workspace_bytes, void *stream) {
    NSA_CHECK_ARG(dtype_ok(dtype), "band_attn_bwd: unknown dtype %d", dtype);
    NSA_CHECK_ARG(B >= 0 && S >= 0 && G >= 1 && h >= 1 && Dk >= 1 && Dv >= 1 && S_kv >= 0, "band_attn_bwd: negative size");
    NSA_CHECK_ARG(t0 >= 0 && dd >= 1 && w >= 0, "band_attn_bwd: need t0 >= 0, dd >= 1, w >= 0");
    NSA_CHECK_ARG(variant >= 0 && variant <= 2, "band_attn_bwd: unknown variant %d", variant);
    const int64_t R = (int64_t)B * S * G;
    if (R == 0) return NSA_OK;
    const size_t roff = band_bwd_ranges_off(B, S, G, h, Dk, Dv, S_kv, dtype, variant);
    if (int rc = check_workspace("band_attn_bwd", workspace, workspace_bytes, roff + sizeof(int32_t) * 2 * (size_t)R)) return rc;
    int32_t *ranges = (int32_t *)((unsigned char *)workspace + roff);
    // the band as one range per row: what the selection backward (either route) reads; its workspace ends where the ranges begin
    const AttnCall call{Q, K, V, ranges, (void *)O, (float *)lse, B, S, G, h, Dk, Dv, S_kv, 1, ksb, ksg, kss, vsb, vsg, vss, dtype, scale, variant == 2 ? 0 : variant,
                        workspace, roff, (hipStream_t)stream};
    const Band band{t0, a, dd, c, w};
    const AttnGrads grads{dO, dQ, dK, dV};
    BandAttnParams BP = band_attn_params(call, band);
    BP.O = nullptr;  // (the dQ kernel takes lse, delta and dO as its own arguments)
    BP.lse = nullptr;
    if (int rc = launch_band_ranges(ranges, BP, call.st)) return rc;
    const bool fast_ok = band_attn_route(call, band).fast_ok && roff > 0 && bwd_mfma_ok(call, grads);
    if (variant == 2) NSA_CHECK_ARG(fast_ok, "band_attn_bwd: MFMA variant requested but shape/dtype/alignment unsupported");
    if (!fast_ok || variant == 1) return sel_attn_bwd_impl(call, grads);
    NSA_CHECK_ARG(Q && K && V && O && lse && dO && dQ && dK && dV, "band_attn_bwd: null pointer");
    float *delta = (float *)workspace;
    if (int rc = launch_bwd_delta(O, dO, delta, R * h, Dv, dtype, call.st)) return rc;
    if (int rc = launch_band_attn_bwd_dq(BP, dO, lse, delta, dQ, dtype, call.st)) return rc;
    SelAttnBwdParams P = sel_attn_bwd_params(call, grads);
    P.skip_delta_dq = 1;
    return launch_sel_attn_bwd_mfma(P, dtype, delta, call.st);
}

// ------------------------------------------------------------------------------ block meta (host)
int nsa_block_counts(int seq_len, int l, int d, int l_sel, int *S_cmp, int *S_sel, int *nnz) {
    NSA_CHECK_ARG(l > 0 && d > 0 && l_sel > 0, "Block parameters must be positive");
    NSA_CHECK_ARG(l % d == 0 && l_sel % d == 0, "Require d|l and d|l_sel in M0");  // block_index.py:75-77
    const int sc = ncmp_of(seq_len, l, d);
    const int ss = seq_len <= 0 ? 0 : (seq_len + l_sel - 1) / l_sel;
    if (S_cmp) *S_cmp = sc;
    if (S_sel) *S_sel = ss;
    if (nnz) {
        // cmp block i = [i d, i d + l) overlaps selection blocks floor(i d / l') .. floor((i d + l - 1) / l'), capped
        int64_t cnt = 0;
        for (int i = 0; i < sc; ++i) {
            const int j0 = (i * d) / l_sel;
            int j1 = (i * d + l - 1) / l_sel;
            if (j1 > ss - 1) j1 = ss - 1;
            if (j1 >= j0) cnt += j1 - j0 + 1;
        }
        *nnz = (int)cnt;
    }
    return NSA_OK;
}

// Closed form of build_M_csl_csr (block_index.py:43-71): O(nnz) instead of the reference's
// O(S_cmp * S_sel) double loop.  Weight = overlap / total overlap, evaluated in double and
// rounded once to fp32 exactly as torch.tensor(python floats, dtype=float32) does.
int nsa_build_block_meta_host(int seq_len, int l, int d, int l_sel, int32_t *csr_indptr, int32_t *csr_indices,
                              float *csr_values, int32_t *csc_ptr, int32_t *csc_rows, float *csc_vals) {
    int sc, ss, nnz;
    int rc = nsa_block_counts(seq_len, l, d, l_sel, &sc, &ss, &nnz);
    if (rc) return rc;
    std::vector<int32_t> ind((size_t)nnz), rows((size_t)nnz);
    std::vector<float> val((size_t)nnz);
    std::vector<int32_t> iptr((size_t)sc + 1, 0);
    int k = 0;
    for (int i = 0; i < sc; ++i) {
        const int a0 = i * d, a1 = i * d + l;
        const int j0 = a0 / l_sel;
        int j1 = (a1 - 1) / l_sel;
        if (j1 > ss - 1) j1 = ss - 1;
        int total = 0;
        for (int j = j0; j <= j1; ++j) {
            const int lo = a0 > j * l_sel ? a0 : j * l_sel;
            const int hi = a1 < (j + 1) * l_sel ? a1 : (j + 1) * l_sel;
            total += hi - lo;
        }
        for (int j = j0; j <= j1; ++j) {
            const int lo = a0 > j * l_sel ? a0 : j * l_sel;
            const int hi = a1 < (j + 1) * l_sel ? a1 : (j + 1) * l_sel;
            ind[k] = j;
            rows[k] = i;
            val[k] = (float)((double)(hi - lo) / (double)total);
            ++k;
        }
        iptr[(size_t)i + 1] = k;
    }
    if (csr_indptr) memcpy(csr_indptr, iptr.data(), sizeof(int32_t) * ((size_t)sc + 1));
    if (csr_indices && nnz) memcpy(csr_indices, ind.data(), sizeof(int32_t) * (size_t)nnz);
    if (csr_values && nnz) memcpy(csr_values, val.data(), sizeof(float) * (size_t)nnz);
    if (csc_ptr) {
        // counting sort by column; stable in the row index => ascending cmp row inside each column
        std::vector<int32_t> cnt((size_t)ss + 1, 0);
        for (int e = 0; e < nnz; ++e) cnt[(size_t)ind[e] + 1]++;
        for (int j = 0; j < ss; ++j) cnt[(size_t)j + 1] += cnt[j];
        memcpy(csc_ptr, cnt.data(), sizeof(int32_t) * ((size_t)ss + 1));
        if (csc_rows && csc_vals) {
            std::vector<int32_t> pos(cnt.begin(), cnt.end() - 1);
            for (int e = 0; e < nnz; ++e) {
                const int p = pos[ind[e]]++;
                csc_rows[p] = rows[e];
                csc_vals[p] = val[e];
            }
        }
    }
    return NSA_OK;
}

// ------------------------------------------------------------------------------ scores
int nsa_map_pcmp_to_pgrp(const float *p_cmp, int64_t R, int h, int S_cmp_cur, const int32_t *csc_ptr,
                         const int32_t *csc_rows, const float *csc_vals, int S_sel, float *p_slc, float *p_grp,
                         void *stream) {
    NSA_CHECK_ARG(p_grp && csc_ptr, "map_pcmp_to_pgrp: null pointer");
    return launch_map_pcmp(p_cmp, R, h, S_cmp_cur, csc_ptr, csc_rows, csc_vals, S_sel, p_slc, p_grp, (hipStream_t)stream);
}

// (the scorers hand a NaN scale on, the attention fills replace it)
static float scorer_scale(float scale, int Dk) { return scale <= 0.f ? default_scale(0.f, Dk) : scale; }

int nsa_pcmp_all(const void *Q, const void *K_cmp, float *p_cmp, int B, int S, int G, int h, int Dk, int S_cmp,
                 int64_t csb, int64_t csg, int64_t css, int dtype, float scale, void *stream) {
    NSA_CHECK_ARG(dtype_ok(dtype), "pcmp_all: unknown dtype %d", dtype);
    NSA_CHECK_ARG(B >= 0 && S >= 0 && G >= 1, "pcmp_all: bad sizes");
    ScoresCall c{};  // all rows in one chunk, written to p_cmp; normalised over all S_cmp columns
    c.Q = Q; c.K_cmp = K_cmp; c.B = B; c.S = S; c.G = G; c.h = h; c.Dk = Dk; c.S_cmp = S_cmp; c.csb = csb; c.csg = csg; c.css = css;
    c.l = 1; c.d = 1; c.dtype = dtype; c.scale = scorer_scale(scale, Dk); c.ws = p_cmp; c.st = (hipStream_t)stream;
    return launch_pcmp(c, 0, c.rows());
}

size_t nsa_sel_scores_rows_workspace(int B, int S, int G, int h, int Dk, int S_cmp, int S_sel, int l, int d, int l_sel, int dtype,
                                     int variant, int norm) {
    const int64_t R = (int64_t)B * S * G;
    switch (scores_route(scores_shape_call(B, S, G, h, Dk, S_cmp, S_sel, l, d, l_sel, dtype, norm), variant).route) {
        case 2: return 0;
        case 3: return decode_scores_workspace(R, h, S_cmp);
        default: return S_cmp > 0 ? scores_workspace(R, h, S_cmp) : 0;
    }
}

size_t nsa_sel_scores_workspace(int B, int S, int G, int h, int Dk, int S_cmp, int S_sel, int l, int d, int l_sel, int dtype,
                                int variant) {
    return nsa_sel_scores_rows_workspace(B, S, G, h, Dk, S_cmp, S_sel, l, d, l_sel, dtype, variant, 0);
}

int nsa_sel_scores_rows(const void *Q, const void *K_cmp, float *p_grp, int B, int S, int G, int h, int Dk, int S_cmp,
                        int64_t csb, int64_t csg, int64_t css, const int32_t *csc_ptr, const int32_t *csc_rows,
                        const float *csc_vals, int S_sel, int l, int d, int l_sel, int causal_skip, int variant, int dtype,
                        float scale, int q0, int norm, void *workspace, size_t workspace_bytes, void *stream) {
    return sel_scores_impl(ScoresCall{Q, K_cmp, p_grp, csc_ptr, csc_rows, csc_vals, B, S, G, h, Dk, S_cmp, S_sel, csb, csg, css, l, d, l_sel, causal_skip,
                                      dtype, scale, q0, norm, workspace, workspace_bytes, (hipStream_t)stream},
                           variant);
}

int nsa_sel_scores(const void *Q, const void *K_cmp, float *p_grp, int B, int S, int G, int h, int Dk, int S_cmp,
                   int64_t csb, int64_t csg, int64_t css, const int32_t *csc_ptr, const int32_t *csc_rows,
                   const float *csc_vals, int S_sel, int l, int d, int l_sel, int causal_skip, int variant, int dtype,
                   float scale, void *workspace, size_t workspace_bytes, void *stream) {
    return sel_scores_impl(ScoresCall{Q, K_cmp, p_grp, csc_ptr, csc_rows, csc_vals, B, S, G, h, Dk, S_cmp, S_sel, csb, csg, css, l, d, l_sel, causal_skip,
                                      dtype, scale, 0, 0, workspace, workspace_bytes, (hipStream_t)stream},
                           variant);
}

int nsa_sel_scores_select_rows(const void *Q, const void *K_cmp, float *p_grp, int B, int S, int G, int h, int Dk, int S_cmp, int64_t csb,
                               int64_t csg, int64_t css, const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel, int l,
                               int d, int l_sel, int causal_skip, int dtype, float scale, int t0, int n_top, int force_init, int force_local,
                               int mode, int S_total, int32_t *ranges_out, int out_width, int q0, int norm, void *workspace,
                               size_t workspace_bytes, void *stream) {
    return sel_scores_select_impl(ScoresCall{Q, K_cmp, p_grp, csc_ptr, csc_rows, csc_vals, B, S, G, h, Dk, S_cmp, S_sel, csb, csg, css, l, d, l_sel,
                                             causal_skip, dtype, scale, q0, norm, workspace, workspace_bytes, (hipStream_t)stream},
                                  SelectCall{t0, nullptr, n_top, force_init, force_local, mode, S_total, ranges_out, out_width});
}

int nsa_sel_scores_select(const void *Q, const void *K_cmp, float *p_grp, int B, int S, int G, int h, int Dk, int S_cmp, int64_t csb, int64_t csg,
                          int64_t css, const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel, int l, int d,
                          int l_sel, int causal_skip, int dtype, float scale, int t0, int n_top, int force_init, int force_local, int mode,
                          int S_total, int32_t *ranges_out, int out_width, void *workspace, size_t workspace_bytes, void *stream) {
    return sel_scores_select_impl(ScoresCall{Q, K_cmp, p_grp, csc_ptr, csc_rows, csc_vals, B, S, G, h, Dk, S_cmp, S_sel, csb, csg, css, l, d, l_sel,
                                             causal_skip, dtype, scale, 0, 0, workspace, workspace_bytes, (hipStream_t)stream},
                                  SelectCall{t0, nullptr, n_top, force_init, force_local, mode, S_total, ranges_out, out_width});
}

// ------------------------------------------------------------------------------ selection
int nsa_batched_ranges_width(int S, int S_sel, int l_sel, int n_top, int force_init, int force_local) {
    return batched_width(S, S_sel, l_sel, n_top, force_init, force_local);
}

int nsa_select_topn_ranges(const float *p_grp, int64_t R, int S, int G, int t0, const int32_t *t_rows, int S_sel,
                           int l_sel, int n_top, int force_init, int force_local, int mode, int S_total,
                           int32_t *ranges_out, int out_width, void *stream) {
    return select_topn_impl(p_grp, R, S, G, S_sel, l_sel, SelectCall{t0, t_rows, n_top, force_init, force_local, mode, S_total, ranges_out, out_width},
                            (hipStream_t)stream);
}

int nsa_sel_select_attn_fwd(const float *p_grp, int t0, const int32_t *t_rows, int S_sel, int l_sel, int n_top, int force_init,
                            int force_local, int mode, int S_total, int32_t *ranges_out, int out_width, const void *Q, const void *K,
                            const void *V, void *O, float *lse, int B, int S, int G, int h, int Dk, int Dv, int S_kv, int64_t ksb,
                            int64_t ksg, int64_t kss, int64_t vsb, int64_t vsg, int64_t vss, int dtype, float scale, void *workspace,
                            size_t workspace_bytes, void *stream) {
    return sel_select_attn_impl(p_grp, S_sel, l_sel, SelectCall{t0, t_rows, n_top, force_init, force_local, mode, S_total, ranges_out, out_width},
                                AttnCall{Q, K, V, ranges_out, O, lse, B, S, G, h, Dk, Dv, S_kv, out_width, ksb, ksg, kss, vsb, vsg, vss, dtype, scale, 0, workspace,
                                         workspace_bytes, (hipStream_t)stream});
}

// ------------------------------------------------------------------------------ fused decode step
static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// decode-step workspace: scorer scratch (a bytes) | p_grp (p bytes) | attention scratch (c bytes), each a multiple of 16 bytes
struct SelDecodeWs {
    size_t a, p, c;
    SelDecodeWs(int B, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int n_top, int dtype)
        : a(align16(nsa_sel_scores_workspace(B, 1, G, h, Dk, S_cmp, S_sel, 0, 0, 0, dtype, 3))),
          p(align16(sizeof(float) * (size_t)B * G * (size_t)(S_sel > 0 ? S_sel : 1))),
          c(align16(nsa_sel_attn_fwd_workspace(B, 1, G, h, Dk, Dv, n_top, dtype))) {}
    size_t total() const { return a + p + c; }
};

size_t nsa_sel_decode_step_workspace(int B, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int n_top, int dtype) {
    return SelDecodeWs(B, G, h, Dk, Dv, S_cmp, S_sel, n_top, dtype).total();
}

// nsa_sel_decode_rows: scorer scratch (a) | p_grp (p) | attention scratch (c) of the separate launches; the one-launch form needs none
struct SelDecodeRowsWs {
    size_t a, p, c;
    SelDecodeRowsWs(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int n_top, int dtype)
        : a(align16(std::max(nsa_sel_scores_rows_workspace(B, S, G, h, Dk, S_cmp, S_sel, 0, 0, 0, dtype, 1, 1),
                             S_cmp >= 1 ? nsa_sel_scores_rows_workspace(B, S, G, h, Dk, S_cmp, S_sel, 0, 0, 0, dtype, 3, 1) : (size_t)0))),
          p(align16(sizeof(float) * (size_t)B * S * G * (size_t)(S_sel > 0 ? S_sel : 1))),
          c(align16(nsa_sel_attn_fwd_workspace_kv(B, S, G, h, Dk, Dv, 64 * (S_sel > 0 ? S_sel : 1), n_top, dtype))) {}
    size_t total() const { return a + p + c; }
};

size_t nsa_sel_decode_rows_workspace(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int n_top, int dtype) {
    if (B < 1 || S < 1 || G < 1 || h < 1) return 0;
    return SelDecodeRowsWs(B, S, G, h, Dk, Dv, S_cmp, S_sel, n_top, dtype).total();
}

}  // extern "C"

// ---- the scorer and selector family on its argument blocks (what the entry points above fill)
ScoresRoute nsa::scores_route(const ScoresCall &c, int variant) {
    const int64_t R = c.rows();
    const bool some = R > 0 && c.S_cmp >= 1 && c.S_sel > 0;  // something to score
    const bool tiled = some && scores_mfma_supported(c) && (int64_t)c.B * c.G <= 65535;
    ScoresRoute r;
    r.decode_fits = c.h <= 64 && (size_t)c.h * c.Dk * 4 <= 64 * 1024;
    r.route = variant != 0 ? variant : some && R <= DECODE_MAX_ROWS && r.decode_fits && !(c.norm && c.S >= 64) ? 3 : tiled ? 2 : 1;
    const bool logits_mfma = (c.dtype == NSA_DT_BF16 || c.dtype == NSA_DT_F16) && (c.Dk == 64 || c.Dk == 128) && c.h <= 16;
    r.mfma = (r.route == 3 ? logits_mfma : tiled) && kcmp_aligned(c.Q, c.K_cmp, c.csb, c.csg, c.css);
    return r;
}

int nsa::sel_scores_impl(ScoresCall c, int variant) {
    NSA_CHECK_ARG(dtype_ok(c.dtype), "sel_scores: unknown dtype %d", c.dtype);
    NSA_CHECK_ARG(c.B >= 0 && c.S >= 0 && c.G >= 1 && c.h >= 1, "sel_scores: bad sizes");
    NSA_CHECK_ARG(variant >= 0 && variant <= 3, "sel_scores: unknown variant %d", variant);
    NSA_CHECK_ARG(c.q0 >= 0 && (c.norm == 0 || c.norm == 1), "sel_scores: bad q0 / norm");
    NSA_CHECK_ARG(c.norm == 0 || (c.l >= 1 && c.d >= 1), "sel_scores: norm = 1 needs the block geometry l, d");
    c.scale = scorer_scale(c.scale, c.Dk);
    const ScoresRoute r = scores_route(c, variant);
    if (r.route == 3 && c.S_cmp >= 1 && c.rows() > 0 && c.S_sel > 0) return launch_decode_scores(c);
    if (r.route == 2) {
        NSA_CHECK_ARG(r.mfma, "sel_scores: MFMA route needs bf16/f16, Dk in {64,128}, h <= 16, l = 2d, l' = 4d and 16-byte aligned rows "
                              "(pass variant 1 for the generic route)");
        return launch_sel_scores_mfma(c, nullptr, nullptr);
    }
    return launch_sel_scores(c);
}

int nsa::select_topn_impl(const float *p_grp, int64_t R, int S, int G, int S_sel, int l_sel, const SelectCall &s, hipStream_t st) {
    NSA_CHECK_ARG(p_grp && s.ranges_out || R == 0, "select_topn_ranges: null pointer");
    NSA_CHECK_ARG(R >= 0 && S >= 1 && G >= 1 && S_sel >= 1 && l_sel >= 1 && s.n_top >= 0, "select: bad sizes");
    NSA_CHECK_ARG(S_sel <= 64 * 64, "select: S_sel=%d exceeds 4096 selection blocks", S_sel);
    NSA_CHECK_ARG(s.force_local >= 0 && s.force_local <= 30, "select: force_local out of range");
    SelectParams P{};
    if (int rc = select_params_fill(&P, p_grp, R, S, G, S_sel, l_sel, s)) return rc;
    return launch_select_topn(P, st);
}

int nsa::sel_select_attn_impl(const float *p_grp, int S_sel, int l_sel, const SelectCall &sel, const AttnCall &c) {
    NSA_CHECK_ARG(dtype_ok(c.dtype), "sel_select_attn_fwd: unknown dtype %d", c.dtype);
    NSA_CHECK_ARG(c.B >= 0 && c.S >= 1 && c.G >= 1 && c.h >= 1 && c.Dk >= 1 && c.Dv >= 1 && c.S_kv >= 0 && c.n >= 0, "sel_select_attn_fwd: bad sizes");
    const int64_t R = c.rows();
    if (R == 0) return NSA_OK;
    NSA_CHECK_ARG(p_grp && sel.ranges_out, "sel_select_attn_fwd: null pointer");
    const AttnRoute r = sel_attn_route(c);
    const bool fast_ok = r.fast_ok && c.S_kv > 0 && c.n >= 1 && c.n <= 64 && S_sel >= 1 && S_sel <= 1024 && r.nsplit == 1;
    // One launch (the selector inside the attention kernel) or two.  The fused selector runs 8 rows one after the other in a wave of a
    // kernel held to 2 waves per SIMD by its 253 VGPRs: its scalar chains run at latency and it adds 36 / 120 / 424 us at 4k x 8 / 16k x 2 /
    // 64k x 1, where the select kernel on its own (a row per wave, 6+ waves per SIMD) takes 28 / 57 / 243 us (profiles/r02
    // i_selector_share.txt): two launches are the default.
    // (never fused where the attention launch of the two calls would split the keys over two XCD groups: that form takes its ranges from
    // memory, and both ways of calling must give the same bits)
    const bool fuse = fast_ok && tuning(TUNE_SEL_FUSE) > 0 && !sel_attn_mfma_form(sel_attn_mfma_params(c, r, 0), c.dtype).ksplit;
    if (!fuse) {  // two launches
        if (int rc = select_topn_impl(p_grp, R, c.S, c.G, S_sel, l_sel, sel, c.st)) return rc;
        return sel_attn_fwd_impl(c, 0, nullptr);
    }
    NSA_CHECK_ARG(c.Q && c.K && c.V && c.O, "sel_select_attn_fwd: null pointer");
    SelectParams SP{};
    if (int rc = select_params_fill(&SP, p_grp, R, c.S, c.G, S_sel, l_sel, sel)) return rc;
    SelAttnParams P = sel_attn_params(c);
    P.nsplit = 1;
    P.fuse_select = 1;
    P.select = &SP;
    return launch_sel_attn_fwd_mfma(P, c.dtype, c.st);
}

// scores + top-n ranges of every row (prefill): on the 32x32x16 scorer route the selection of a query tile runs inside the scorer launch,
// everywhere else the scorer and the select kernel are launched back to back -- the same ranges bit for bit either way
int nsa::sel_scores_select_impl(ScoresCall c, const SelectCall &s) {
    NSA_CHECK_ARG(dtype_ok(c.dtype), "sel_scores_select: unknown dtype %d", c.dtype);
    NSA_CHECK_ARG(c.B >= 0 && c.S >= 0 && c.G >= 1 && c.h >= 1 && s.out_width >= 0, "sel_scores_select: bad sizes");
    NSA_CHECK_ARG(c.q0 >= 0 && (c.norm == 0 || c.norm == 1), "sel_scores_select: bad q0 / norm");
    const int64_t R = c.rows();
    if (R == 0 || s.out_width == 0) return NSA_OK;
    NSA_CHECK_ARG(c.p_grp && s.ranges_out, "sel_scores_select: null pointer");
    c.scale = scorer_scale(c.scale, c.Dk);
    const ScoresRoute r = scores_route(c, 0);
    if (r.route == 2 && r.mfma) {
        SelectParams SP{};
        if (int rc = select_params_fill(&SP, c.p_grp, R, c.S, c.G, c.S_sel, c.l_sel, s)) return rc;
        int done = 0;
        if (int rc = launch_sel_scores_mfma(c, &SP, &done)) return rc;
        return done ? NSA_OK : launch_select_topn(SP, c.st);
    }
    if (int rc = sel_scores_impl(c, r.route == 2 ? 1 : r.route /* rows the MFMA route cannot take: the generic one */)) return rc;
    return select_topn_impl(c.p_grp, R, c.S, c.G, c.S_sel, c.l_sel, s, c.st);
}

int nsa::sel_decode_step_impl(const SelDecodeCall &c, void *workspace, size_t workspace_bytes, void *stream, int defer, int *ns_used,
                              float **part_used, const DecBandPair *band, int *band_taken) {
    if (band_taken) *band_taken = 0;
    const SelDecodeWs W(c.B, c.G, c.h, c.Dk, c.Dv, c.S_cmp, c.S_sel, c.n_top, c.dtype);
    NSA_CHECK_ARG(workspace && ((uintptr_t)workspace % 16 == 0) && workspace_bytes >= W.total(), "decode_step: workspace missing, misaligned or too small");
    NSA_CHECK_ARG(c.n_top >= 1 && c.n_top <= 64, "decode_step: n_top must be in [1,64]");
    unsigned char *w = (unsigned char *)workspace;
    const size_t a = W.a, p = W.p;
    float *p_grp = (float *)(w + a);
    const int stencil = (c.l == 2 * c.d && c.l_sel == 4 * c.d) ? 1 : 0;  // Eq.9 in closed form (the fused kernel then reads no CSC arrays)
    if (decode_step_supported(c)) {  // scores -> statistics -> Eq.9/10 -> sequential top-n -> selection attention: ONE launch, O is final
        if (ns_used) *ns_used = 1;
        if (band && band_taken) *band_taken = 1;
        return launch_decode_step(c, w, a, (hipStream_t)stream, band_taken ? band : nullptr);
    }
    const ScoresCall sc = scores_call(c, p_grp, 1, 0, w, a, stream);  // the step's one row per (b, g), scored over all S_cmp columns
    const SelectCall sel = decode_select_call(c);
    if (decode_score_select_supported(sc)) {
        // scores -> statistics -> Eq.9/10 -> sequential top-n in one launch (bit-identical to the route below)
        if (int rc = launch_decode_score_select(sc, sel, stencil)) return rc;
    } else {
        if (int rc = sel_scores_impl(sc, c.S_cmp >= 1 ? 3 : 1)) return rc;
        if (int rc = select_topn_impl(p_grp, c.rows(), 1, c.G, c.S_sel, c.l_sel, sel, sc.st)) return rc;
    }
    if (part_used) *part_used = (float *)(w + a + p);
    return sel_attn_fwd_impl(attn_call(c, w + a + p, workspace_bytes - a - p, stream), defer, ns_used);
}

int nsa::sel_decode_rows_impl(const SelDecodeCall &c, void *workspace, size_t workspace_bytes, void *stream) {
    NSA_CHECK_ARG(dtype_ok(c.dtype), "decode_rows: unknown dtype %d", c.dtype);
    NSA_CHECK_ARG(c.B >= 0 && c.S >= 0 && c.G >= 1 && c.h >= 1 && c.Dk >= 1 && c.Dv >= 1 && c.S_cmp >= 0 && c.S_sel >= 1 && c.S_kv >= 1, "decode_rows: bad sizes");
    NSA_CHECK_ARG(c.n_top >= 1 && c.n_top <= 64, "decode_rows: n_top must be in [1,64]");
    NSA_CHECK_ARG(c.t0 >= 0 && c.S_kv >= c.t0 + c.S, "decode_rows: the cache must hold the S tokens t0 .. t0 + S - 1");
    if (c.rows() == 0) return NSA_OK;
    NSA_CHECK_ARG(c.Q && c.K && c.V && c.O && c.ranges_out, "decode_rows: null pointer");
    if (decode_rows_supported(c))  // every row's scores -> top-n at its own token -> selection attention over K/V[:t + 1]: ONE launch
        return launch_decode_rows(c, (hipStream_t)stream);
    // the separate launches: decode-normalised scores + sequential top-n at t0 + s, then the attention (what an extend of S tokens runs)
    const SelDecodeRowsWs W(c.B, c.S, c.G, c.h, c.Dk, c.Dv, c.S_cmp, c.S_sel, c.n_top, c.dtype);
    NSA_CHECK_ARG(workspace && ((uintptr_t)workspace % 16 == 0) && workspace_bytes >= W.total(), "decode_rows: workspace missing, misaligned or too small");
    unsigned char *w = (unsigned char *)workspace;
    if (int rc = sel_scores_select_impl(scores_call(c, (float *)(w + W.a), 2 /* skipped blocks stay unwritten: only the selector reads p_grp */, 1, w, W.a, stream),
                                        decode_select_call(c)))
        return rc;
    return sel_attn_fwd_impl(attn_call(c, w + W.a + W.p, workspace_bytes - W.a - W.p, stream), 0, nullptr);
}

int nsa::sel_decode_ragged_impl(const SelDecodeCall &c, const int32_t *t_pos, int t_max, void *stream) {
    NSA_CHECK_ARG(dtype_ok(c.dtype), "decode_ragged: unknown dtype %d", c.dtype);
    NSA_CHECK_ARG(c.B >= 0 && c.S >= 0 && c.G >= 1 && c.h >= 1 && c.Dk >= 1 && c.Dv >= 1 && c.S_cmp >= 0 && c.S_sel >= 1 && c.S_kv >= 1, "decode_ragged: bad sizes");
    NSA_CHECK_ARG(c.n_top >= 1 && c.n_top <= 64, "decode_ragged: n_top must be in [1,64]");
    NSA_CHECK_ARG(t_max >= 0, "decode_ragged: t_max (the host bound of t_pos[b] + S - 1) must not be negative");
    // the caches' capacity bound: no live row sits beyond te, and the metadata must cover te + 1 tokens
    const int te = std::min(t_max, c.S_kv - 1);
    NSA_CHECK_ARG(c.S_cmp >= decode_ncmp(te) && (int64_t)c.S_sel * 64 >= (int64_t)te + 1,
                  "decode_ragged: S_cmp / S_sel must describe at least min(t_max, S_kv - 1) + 1 = %d tokens (got S_cmp = %d, S_sel = %d)", te + 1, c.S_cmp, c.S_sel);
    if (c.rows() == 0) return NSA_OK;
    NSA_CHECK_ARG(c.Q && c.K && c.V && c.O && c.ranges_out && t_pos && (c.K_cmp || c.S_cmp == 0), "decode_ragged: null pointer");
    NSA_CHECK_ARG((uintptr_t)t_pos % 4 == 0, "decode_ragged: t_pos must be 4-byte aligned");
    const char *why = nullptr;
    NSA_CHECK_ARG(decode_ragged_shape_plan(c, t_max, nullptr, nullptr, &why), "decode_ragged: %s (B = %d, S = %d, D = %d, t_max = %d)", why, c.B, c.S, c.Dk, t_max);
    NSA_CHECK_ARG(c.d == 16 && c.l == 32 && c.l_sel == 64, "decode_ragged: the default block geometry only (l = 32, d = 16, l' = 64)");
    NSA_CHECK_ARG(decode_step_operands_ok(c), "decode_ragged: Q, K_cmp, K and V must be 16-byte aligned with strides in multiples of 8 elements, "
                                                "V rows contiguous and O 8-byte aligned");
    return launch_decode_rows(c, (hipStream_t)stream, t_pos, t_max);
}

// The ragged step over paged caches.  c: K_cmp / K / V are the pools, kcb / ksb / vsb their PAGE strides, S_kv is filled here with the
// capacity max_pages * 1024; S_cmp / S_sel are the metadata bounds of min(t_max, capacity - 1) + 1 tokens as in the ragged call.
int nsa::sel_decode_paged_impl(const SelDecodeCall &c0, const DecPageTable &pt, int max_pages, int page_tokens, const int32_t *t_pos, int t_max, void *stream) {
    NSA_CHECK_ARG(page_tokens == DEC_PAGE_TOKENS, "decode_paged: page_tokens = %d is not built: pages of 1024 tokens only (one scorer chunk of 64 compressed rows, "
                                                  "16 selection blocks)", page_tokens);
    NSA_CHECK_ARG(dtype_ok(c0.dtype), "decode_paged: unknown dtype %d", c0.dtype);
    NSA_CHECK_ARG(max_pages >= 1 && max_pages <= (1 << 20), "decode_paged: max_pages = %d, must be in [1, 2^20]", max_pages);
    NSA_CHECK_ARG(pt.n_pages >= 1, "decode_paged: n_pages = %d, the pools must hold at least one page", pt.n_pages);
    SelDecodeCall c = c0;
    c.S_kv = max_pages * DEC_PAGE_TOKENS;
    NSA_CHECK_ARG(c.B >= 0 && c.S >= 0 && c.G >= 1 && c.h >= 1 && c.Dk >= 1 && c.Dv >= 1 && c.S_cmp >= 0 && c.S_sel >= 1, "decode_paged: bad sizes");
    NSA_CHECK_ARG(c.n_top >= 1 && c.n_top <= 64, "decode_paged: n_top must be in [1,64]");
    NSA_CHECK_ARG(t_max >= 0, "decode_paged: t_max (the host bound of t_pos[b] + S - 1) must not be negative");
    const int te = std::min(t_max, c.S_kv - 1);
    NSA_CHECK_ARG(c.S_cmp >= decode_ncmp(te) && (int64_t)c.S_sel * 64 >= (int64_t)te + 1,
                  "decode_paged: S_cmp / S_sel must describe at least min(t_max, max_pages * 1024 - 1) + 1 = %d tokens (got S_cmp = %d, S_sel = %d)", te + 1, c.S_cmp,
                  c.S_sel);
    if (c.rows() == 0) return NSA_OK;
    NSA_CHECK_ARG(pt.table != nullptr, "decode_paged: null block table");
    NSA_CHECK_ARG((uintptr_t)pt.table % 4 == 0 && pt.stride >= max_pages, "decode_paged: the block table must be 4-byte aligned with a row stride of at least max_pages = %d "
                                                                          "(got %lld)", max_pages, (long long)pt.stride);
    NSA_CHECK_ARG(c.Q && c.K && c.V && c.O && c.ranges_out && t_pos && (c.K_cmp || c.S_cmp == 0), "decode_paged: null pointer");
    NSA_CHECK_ARG((uintptr_t)t_pos % 4 == 0, "decode_paged: t_pos must be 4-byte aligned");
    const char *why = nullptr;
    NSA_CHECK_ARG(decode_paged_shape_plan(c, t_max, nullptr, nullptr, &why), "decode_paged: %s (B = %d, S = %d, D = %d, t_max = %d)", why, c.B, c.S, c.Dk, t_max);
    NSA_CHECK_ARG(c.d == 16 && c.l == 32 && c.l_sel == 64, "decode_paged: the default block geometry only (l = 32, d = 16, l' = 64)");
    NSA_CHECK_ARG(decode_step_operands_ok(c), "decode_paged: Q and the three pools must be 16-byte aligned with page, group and row strides in multiples of 8 elements, "
                                                "V rows contiguous and O 8-byte aligned");
    // the kernel's only 32-bit byte offsets are those of a row inside one (page, group) plane: 1024 K / V rows, 64 compressed rows
    const int64_t lim = (int64_t)1 << 31;
    NSA_CHECK_ARG(c.kss >= 1 && c.vss >= 1 && c.kcs >= 1 && (int64_t)DEC_PAGE_TOKENS * c.kss * 2 < lim && (int64_t)DEC_PAGE_TOKENS * c.vss * 2 < lim &&
                      (int64_t)(DEC_PAGE_TOKENS / 16) * c.kcs * 2 < lim,
                  "decode_paged: the row strides put a page's rows outside the 32-bit offsets of one (page, group) plane (1024 rows of K / V, 64 of K_cmp: under 2 GiB each)");
    return launch_decode_rows(c, (hipStream_t)stream, t_pos, t_max, &pt);
}

int nsa::band_attn_fwd_ragged_impl(const AttnCall &c, const Band &band, const int32_t *t_pos, int t_max) {
    NSA_CHECK_ARG(dtype_ok(c.dtype), "band_attn_fwd_ragged: unknown dtype %d", c.dtype);
    NSA_CHECK_ARG(c.B >= 0 && c.S >= 0 && c.G >= 1 && c.h >= 1 && c.Dk >= 1 && c.Dv >= 1 && c.S_kv >= 0, "band_attn_fwd_ragged: negative size");
    NSA_CHECK_ARG(band.dd >= 1 && band.w >= 0 && t_max >= 0, "band_attn_fwd_ragged: need dd >= 1, w >= 0, t_max >= 0");
    NSA_CHECK_ARG(c.variant >= 0 && c.variant <= 2, "band_attn_fwd_ragged: unknown variant %d", c.variant);
    if (c.rows() == 0) return NSA_OK;
    NSA_CHECK_ARG(c.Q && c.O && t_pos && ((c.K && c.V) || c.S_kv == 0), "band_attn_fwd_ragged: null pointer");
    NSA_CHECK_ARG((uintptr_t)t_pos % 4 == 0, "band_attn_fwd_ragged: t_pos must be 4-byte aligned");
    // the route, the split count and the workspace do not depend on the positions: they are the scalar call's (planned from B, S, G, h, D)
    BandAttnParams P = band_attn_params(c, Band{0, band.a, band.dd, band.c, band.w});
    P.t_pos = t_pos;
    P.t_max = t_max;
    const AttnRoute r = band_attn_route(c, band);
    if (c.variant == 2) NSA_CHECK_ARG(r.fast_ok, "band_attn_fwd_ragged: MFMA variant requested but shape/dtype/alignment unsupported");
    if (r.kind != AttnRoute::MFMA) return launch_band_attn_fwd_generic(P, c.dtype, c.st);
    if (r.ws == AttnRoute::WS_SPLIT) {
        P.part = (float *)c.ws;
        P.nsplit = r.nsplit;
    }
    return launch_band_attn_fwd_mfma(P, c.dtype, c.st);
}

// The ragged band forward over paged caches.  c: K / V are the pools, ksb / vsb their PAGE strides; S_kv is filled here with the capacity
// max_pages * page_rows.  One route -- the MFMA kernels' PAGED form -- with the plan (form, split count, workspace) of the scalar and the
// ragged call; everything else is declined, there is no generic kernel over pools.
int nsa::band_attn_fwd_paged_impl(const AttnCall &c0, const Band &band, const BandPageTable &pt0, int max_pages, int page_rows, const int32_t *t_pos, int t_max) {
    NSA_CHECK_ARG(dtype_ok(c0.dtype), "band_attn_fwd_paged: unknown dtype %d", c0.dtype);
    NSA_CHECK_ARG(c0.B >= 0 && c0.S >= 0 && c0.G >= 1 && c0.h >= 1 && c0.Dk >= 1 && c0.Dv >= 1, "band_attn_fwd_paged: negative size");
    NSA_CHECK_ARG(band.dd >= 1 && t_max >= 0, "band_attn_fwd_paged: need dd >= 1, t_max >= 0");
    NSA_CHECK_ARG(attn_mfma_shape_ok(c0.dtype, c0.h, c0.Dk, c0.Dv),
                  "band_attn_fwd_paged: the MFMA kernels only -- bf16 / f16, Dk = Dv in {64, 128}, h <= 16 (got dtype %d, Dk = %d, Dv = %d, h = %d); no kernel reads "
                  "pools of pages for other shapes", c0.dtype, c0.Dk, c0.Dv, c0.h);
    NSA_CHECK_ARG(band.w >= 1, "band_attn_fwd_paged: w = %d, the window must hold at least one key (w >= 1)", band.w);
    NSA_CHECK_ARG(page_rows >= 32 && page_rows <= 65536 && (page_rows & (page_rows - 1)) == 0,
                  "band_attn_fwd_paged: page_rows = %d is not built: a power of two in [32, 65536] (a 32-key tile then touches at most two pages)", page_rows);
    NSA_CHECK_ARG(max_pages >= 1 && max_pages <= (1 << 20), "band_attn_fwd_paged: max_pages = %d, must be in [1, 2^20]", max_pages);
    NSA_CHECK_ARG(pt0.n_pages >= 1, "band_attn_fwd_paged: n_pages = %d, the pools must hold at least one page", pt0.n_pages);
    AttnCall c = c0;
    // (positions are 32-bit: a capacity beyond INT32_MAX rows bounds nothing a position can reach)
    c.S_kv = (int)std::min<int64_t>((int64_t)max_pages * page_rows, INT32_MAX);
    if (c.rows() == 0) return NSA_OK;
    NSA_CHECK_ARG(pt0.table != nullptr, "band_attn_fwd_paged: null block table");
    NSA_CHECK_ARG((uintptr_t)pt0.table % 4 == 0 && pt0.stride >= max_pages, "band_attn_fwd_paged: the block table must be 4-byte aligned with a row stride of at least "
                                                                           "max_pages = %d (got %lld)", max_pages, (long long)pt0.stride);
    NSA_CHECK_ARG(c.Q && c.K && c.V && c.O && t_pos, "band_attn_fwd_paged: null pointer");
    NSA_CHECK_ARG((uintptr_t)t_pos % 4 == 0, "band_attn_fwd_paged: t_pos must be 4-byte aligned");
    NSA_CHECK_ARG(qkv_aligned(c) && out_aligned(c), "band_attn_fwd_paged: Q and the two pools must be 16-byte aligned with page, group and row strides in multiples of "
                                                    "8 elements, and O 8-byte aligned");
    // the kernel's only 32-bit byte offsets are those of a row inside one (page, group) plane of page_rows rows
    const int64_t lim = (int64_t)1 << 31;
    NSA_CHECK_ARG(c.kss >= 1 && c.vss >= 1 && (int64_t)page_rows * c.kss * 2 < lim && (int64_t)page_rows * c.vss * 2 < lim,
                  "band_attn_fwd_paged: the row strides put a page's rows outside the 32-bit offsets of one (page, group) plane (page_rows = %d rows: under 2 GiB)",
                  page_rows);
    BandAttnParams P = band_attn_params(c, Band{0, band.a, band.dd, band.c, band.w});
    P.t_pos = t_pos;
    P.t_max = t_max;
    // the split count and the workspace do not depend on the positions or the pages: the scalar call's; without the workspace, the unsplit form
    int ns = 1;
    const size_t need = band_attn_workspace(c.B, c.S, c.G, c.h, c.Dk, c.Dv, c.dtype, &ns);
    if (ns > 1 && c.ws && ((uintptr_t)c.ws % 16 == 0) && c.ws_bytes >= need) {
        P.part = (float *)c.ws;
        P.nsplit = ns;
    }
    BandPageTable pt = pt0;
    pt.shift = __builtin_ctz((unsigned)page_rows);
    return launch_band_attn_fwd_mfma(P, c.dtype, c.st, &pt);
}

extern "C" {

size_t nsa_band_attn_fwd_paged_workspace(int B, int S, int G, int h, int Dk, int Dv, int dtype) {
    return band_attn_workspace(B, S, G, h, Dk, Dv, dtype, nullptr);  // planned from (B, S, G, h, D) alone: the scalar and the ragged call's
}

int nsa_band_attn_fwd_paged(const void *Q, const void *K_pool, const void *V_pool, const int32_t *block_table, int64_t table_stride, int n_pages, int max_pages,
                            int page_rows, void *O, float *lse, const int32_t *t_pos, int t_max, int B, int S, int G, int h, int Dk, int Dv, int64_t ksp, int64_t ksg,
                            int64_t kss, int64_t vsp, int64_t vsg, int64_t vss, int a, int dd, int c, int w, int dtype, float scale, void *workspace,
                            size_t workspace_bytes, void *stream) {
    return band_attn_fwd_paged_impl(AttnCall{Q, K_pool, V_pool, nullptr, O, lse, B, S, G, h, Dk, Dv, 0, 0, ksp, ksg, kss, vsp, vsg, vss, dtype, scale, 0, workspace,
                                             workspace_bytes, (hipStream_t)stream},
                                    Band{0, a, dd, c, w}, BandPageTable{block_table, table_stride, n_pages, 0}, max_pages, page_rows, t_pos, t_max);
}

int nsa_sel_decode_ragged(const void *Q, const void *K_cmp, const void *K, const void *V, const int32_t *csc_ptr, const int32_t *csc_rows,
                          const float *csc_vals, int32_t *ranges_out, void *O, const int32_t *t_pos, int t_max, int B, int S, int G, int h, int Dk,
                          int Dv, int S_cmp, int S_sel, int S_kv, int l, int d, int l_sel, int n_top, int64_t kcb, int64_t kcg, int64_t kcs,
                          int64_t ksb, int64_t ksg, int64_t kss, int64_t vsb, int64_t vsg, int64_t vss, int dtype, float scale, void *workspace,
                          size_t workspace_bytes, void *stream) {
    (void)workspace, (void)workspace_bytes;  // (the one launch needs no scratch)
    const SelDecodeCall c{Q, K_cmp, K, V, csc_ptr, csc_rows, csc_vals, ranges_out, O, B, S, G, h, Dk, Dv, S_cmp, S_sel, S_kv, l, d, l_sel, n_top, 0,
                          kcb, kcg, kcs, ksb, ksg, kss, vsb, vsg, vss, dtype, scale};
    return sel_decode_ragged_impl(c, t_pos, t_max, stream);
}

int nsa_sel_decode_paged(const void *Q, const void *Kc_pool, const void *K_pool, const void *V_pool, const int32_t *block_table, int64_t table_stride,
                         int n_pages, int max_pages, int page_tokens, const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals,
                         int32_t *ranges_out, void *O, const int32_t *t_pos, int t_max, int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int l,
                         int d, int l_sel, int n_top, int64_t kcp, int64_t kcg, int64_t kcs, int64_t ksp, int64_t ksg, int64_t kss, int64_t vsp, int64_t vsg,
                         int64_t vss, int dtype, float scale, void *workspace, size_t workspace_bytes, void *stream) {
    (void)workspace, (void)workspace_bytes;  // (the one launch needs no scratch)
    const SelDecodeCall c{Q, Kc_pool, K_pool, V_pool, csc_ptr, csc_rows, csc_vals, ranges_out, O, B, S, G, h, Dk, Dv, S_cmp, S_sel, 0, l, d, l_sel, n_top, 0,
                          kcp, kcg, kcs, ksp, ksg, kss, vsp, vsg, vss, dtype, scale};
    return sel_decode_paged_impl(c, DecPageTable{block_table, table_stride, n_pages}, max_pages, page_tokens, t_pos, t_max, stream);
}

size_t nsa_sel_decode_paged_workspace(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int n_top, int dtype) {
    (void)B, (void)S, (void)G, (void)h, (void)Dk, (void)Dv, (void)S_cmp, (void)S_sel, (void)n_top, (void)dtype;
    return 0;  // one launch, everything on chip (the ragged call's answer)
}

int nsa_sel_decode_paged_plan(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int max_pages, int page_tokens, int n_top, int dtype,
                              int t_max, int *launches, int *form) {
    NSA_CHECK_ARG(launches && form, "decode_paged_plan: null pointer");
    NSA_CHECK_ARG(dtype_ok(dtype), "decode_paged_plan: unknown dtype %d", dtype);
    NSA_CHECK_ARG(B >= 1 && S >= 1 && G >= 1 && h >= 1 && Dk >= 1 && Dv >= 1 && S_cmp >= 0 && S_sel >= 1 && max_pages >= 1 && max_pages <= (1 << 20) &&
                      page_tokens >= 1 && n_top >= 1 && n_top <= 64 && t_max >= 0,
                  "decode_paged_plan: bad sizes");
    *launches = 0;
    *form = -1;
    if (page_tokens == DEC_PAGE_TOKENS &&
        decode_paged_shape_plan(sel_decode_plan_call(B, S, G, h, Dk, Dv, S_cmp, S_sel, max_pages * DEC_PAGE_TOKENS, n_top, dtype), t_max, form, nullptr, nullptr))
        *launches = 1;
    return NSA_OK;
}

size_t nsa_sel_decode_ragged_workspace(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int n_top, int dtype) {
    (void)B, (void)S, (void)G, (void)h, (void)Dk, (void)Dv, (void)S_cmp, (void)S_sel, (void)n_top, (void)dtype;
    return 0;  // one launch, everything on chip: the query exists so that a later form may ask for scratch without a change of the callers
}

int nsa_sel_decode_ragged_plan(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int S_kv, int n_top, int dtype, int t_max,
                               int *launches, int *form) {
    NSA_CHECK_ARG(launches && form, "decode_ragged_plan: null pointer");
    NSA_CHECK_ARG(dtype_ok(dtype), "decode_ragged_plan: unknown dtype %d", dtype);
    NSA_CHECK_ARG(B >= 1 && S >= 1 && G >= 1 && h >= 1 && Dk >= 1 && Dv >= 1 && S_cmp >= 0 && S_sel >= 1 && S_kv >= 1 && n_top >= 1 && n_top <= 64 && t_max >= 0,
                  "decode_ragged_plan: bad sizes");
    // one launch or none: the separate launches take a scalar position only, so a declined shape has no route (launches 0, form -1)
    *launches = decode_ragged_shape_plan(sel_decode_plan_call(B, S, G, h, Dk, Dv, S_cmp, S_sel, S_kv, n_top, dtype), t_max, form, nullptr, nullptr) ? 1 : 0;
    return NSA_OK;
}

int nsa_band_attn_fwd_ragged(const void *Q, const void *K, const void *V, void *O, float *lse, const int32_t *t_pos, int t_max, int B, int S, int G,
                             int h, int Dk, int Dv, int S_kv, int64_t ksb, int64_t ksg, int64_t kss, int64_t vsb, int64_t vsg, int64_t vss, int a, int dd,
                             int c, int w, int dtype, float scale, int variant, void *workspace, size_t workspace_bytes, void *stream) {
    return band_attn_fwd_ragged_impl(AttnCall{Q, K, V, nullptr, O, lse, B, S, G, h, Dk, Dv, S_kv, 0, ksb, ksg, kss, vsb, vsg, vss, dtype, scale, variant,
                                              workspace, workspace_bytes, (hipStream_t)stream},
                                     Band{0, a, dd, c, w}, t_pos, t_max);
}

size_t nsa_band_attn_fwd_ragged_workspace(int B, int S, int G, int h, int Dk, int Dv, int dtype) {
    return band_attn_workspace(B, S, G, h, Dk, Dv, dtype, nullptr);  // the split count is planned from the row count alone: the scalar call's
}

int nsa_sel_decode_step(const void *Q, const void *K_cmp, const void *K, const void *V, const int32_t *csc_ptr,
                        const int32_t *csc_rows, const float *csc_vals, int32_t *ranges_out, void *O, int B, int G, int h, int Dk,
                        int Dv, int S_cmp, int S_sel, int S_kv, int l, int d, int l_sel, int n_top, int t_token, int64_t kcb,
                        int64_t kcg, int64_t kcs, int64_t ksb, int64_t ksg, int64_t kss, int64_t vsb, int64_t vsg, int64_t vss,
                        int dtype, float scale, void *workspace, size_t workspace_bytes, void *stream) {
    const SelDecodeCall c{Q, K_cmp, K, V, csc_ptr, csc_rows, csc_vals, ranges_out, O, B, 1, G, h, Dk, Dv, S_cmp, S_sel, S_kv, l, d, l_sel, n_top, t_token,
                          kcb, kcg, kcs, ksb, ksg, kss, vsb, vsg, vss, dtype, scale};
    return sel_decode_step_impl(c, workspace, workspace_bytes, stream, 0, nullptr, nullptr);
}

int nsa_sel_decode_rows(const void *Q, const void *K_cmp, const void *K, const void *V, const int32_t *csc_ptr, const int32_t *csc_rows,
                        const float *csc_vals, int32_t *ranges_out, void *O, int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel,
                        int S_kv, int l, int d, int l_sel, int n_top, int t0, int64_t kcb, int64_t kcg, int64_t kcs, int64_t ksb, int64_t ksg,
                        int64_t kss, int64_t vsb, int64_t vsg, int64_t vss, int dtype, float scale, void *workspace, size_t workspace_bytes,
                        void *stream) {
    const SelDecodeCall c{Q, K_cmp, K, V, csc_ptr, csc_rows, csc_vals, ranges_out, O, B, S, G, h, Dk, Dv, S_cmp, S_sel, S_kv, l, d, l_sel, n_top, t0,
                          kcb, kcg, kcs, ksb, ksg, kss, vsb, vsg, vss, dtype, scale};
    return sel_decode_rows_impl(c, workspace, workspace_bytes, stream);
}

int nsa_sel_decode_step_plan(int B, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int S_kv, int n_top, int dtype, int *launches, int *form,
                             int *nsplit) {
    NSA_CHECK_ARG(launches && form && nsplit, "decode_step_plan: null pointer");
    NSA_CHECK_ARG(dtype_ok(dtype), "decode_step_plan: unknown dtype %d", dtype);
    NSA_CHECK_ARG(B >= 1 && G >= 1 && h >= 1 && Dk >= 1 && Dv >= 1 && S_cmp >= 0 && S_sel >= 1 && S_kv >= 1 && n_top >= 1 && n_top <= 64,
                  "decode_step_plan: bad sizes");
    const int64_t R = (int64_t)B * G;
    if (decode_step_shape_plan(sel_decode_plan_call(B, 1, G, h, Dk, Dv, S_cmp, S_sel, S_kv, n_top, dtype), form, nsplit)) {
        *launches = 1;
        return NSA_OK;
    }
    // the route of sel_decode_step_impl for a declined shape, by the shape parts of the predicates it asks: scores + top-n in one launch or
    // three, then the attention (its decode form is one launch; the prefill kernel with the keys split adds a combine launch)
    int n = decode_score_select_shape_ok(scores_shape_call(B, 1, G, h, Dk, S_cmp, S_sel, 32, 16, 64, dtype, 0)) ? 1 : 3;
    if (sel_attn_decode_wg_shape_ok(dtype, h, Dk, Dv, n_top) && (int64_t)S_kv * 2 * Dv < ((int64_t)1 << 31)) {
        n += 1;
    } else {
        int ns = 1;
        if (attn_mfma_shape_ok(dtype, h, Dk, Dv)) sel_attn_mfma_workspace(R, h, Dv, &ns);
        n += ns > 1 ? 2 : 1;
    }
    *launches = n;
    return NSA_OK;
}

// the plan of nsa_sel_decode_rows for a cache that holds exactly the S new tokens behind t0 = S_kv - S (default block geometry, aligned inputs)
int nsa_sel_decode_rows_plan(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int S_kv, int n_top, int dtype, int *launches,
                             int *form) {
    NSA_CHECK_ARG(launches && form, "decode_rows_plan: null pointer");
    NSA_CHECK_ARG(dtype_ok(dtype), "decode_rows_plan: unknown dtype %d", dtype);
    NSA_CHECK_ARG(B >= 1 && S >= 1 && G >= 1 && h >= 1 && Dk >= 1 && Dv >= 1 && S_cmp >= 0 && S_sel >= 1 && S_kv >= S && n_top >= 1 && n_top <= 64,
                  "decode_rows_plan: bad sizes");
    if (decode_rows_shape_plan(sel_decode_plan_call(B, S, G, h, Dk, Dv, S_cmp, S_sel, S_kv, n_top, dtype), form, nullptr)) {
        *launches = 1;
        return NSA_OK;
    }
    // separate launches: the scorer (the decode-shaped pair, or one launch of the tiled / generic scorer), the select kernel, the attention
    // (a combine launch more where it splits the keys): an estimate, only "> 1" is contractual
    const int route = scores_route(scores_shape_call(B, S, G, h, Dk, S_cmp, S_sel, 32, 16, 64, dtype, 1), 0).route;
    *launches = (route == 3 ? 2 : 1) + 1 + 1;
    return NSA_OK;
}

int nsa_indices_to_ranges_v2(const int32_t *indices, int64_t R, int S, int G, int t0, int K, int S_sel, int l_sel,
                             int32_t *ranges_out, void *stream) {
    NSA_CHECK_ARG((indices && ranges_out) || R == 0 || K == 0, "indices_to_ranges_v2: null pointer");
    NSA_CHECK_ARG(S >= 1 && G >= 1, "indices_to_ranges_v2: bad sizes");
    return launch_indices_to_ranges(indices, R, S, G, t0, K, S_sel, l_sel, ranges_out, (hipStream_t)stream);
}

}  // extern "C"
