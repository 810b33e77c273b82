"""Helper of test_dispatch_host.py (not a test): asks the library's host dispatch layer for its tuning defaults, a table of workspace
sizes and the answers to a few refused calls, and prints them as one JSON object.  It makes no HIP call, so it runs without a GPU; it is
run in a fresh process so that no earlier test has touched a tuning switch.  `python tests/dispatch_probe.py` with NSA_HIP_LIB pointing at
a build of an older commit regenerates tests/golden/dispatch_host_sizes.json (the "sizes" and "tuning" parts)."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsa_vibe_amd import _lib  # noqa: E402

TUNING_NAMES = ["SEL_ROWS", "ATTN_MAP", "ATTN_STAGE", "BAND_STAGE", "DECODE_UNFUSED", "SEL_BLOCKS", "DECODE_WG", "SEL_ROWSUM", "DECODE_STENCIL",
                "SEL_FUSE", "SCORES_FORM", "SEL_FLAT", "SEL_KSPLIT", "DECODE_STOP", "DECODE_WAVES", "DECODE_SPLIT", "DECODE_STEP",
                "DECODE_TEAM_SPIN", "DECODE_WIDE", "SEL_KSPLIT_T1", "SEL_KSPLIT_T2", "SCORES_SELECT", "DECODE_BAND"]

# name -> (dim, G, h, D, l, d, l_sel, n_sel, w, dtype): the m7c layer, the same at D = 128 and in fp32, and the g20 geometry (D = 32)
LAYERS = {
    "m7c_bf16": (768, 2, 6, 64, 32, 16, 64, 16, 512, _lib.NSA_DT_BF16),
    "m7c_d128_bf16": (768, 2, 6, 128, 32, 16, 64, 16, 512, _lib.NSA_DT_BF16),
    "m7c_f32": (768, 2, 6, 64, 32, 16, 64, 16, 512, _lib.NSA_DT_F32),
    "g20_f32": (256, 2, 4, 32, 32, 16, 64, 16, 512, _lib.NSA_DT_F32),
    "g20_f16": (256, 2, 4, 32, 32, 16, 64, 16, 512, _lib.NSA_DT_F16),
}
BATCHES = (1, 8)
ROWS = (1, 63, 64, 100, 4096)   # 1 and below l = 32: no compressed token; 63 / 64 / 100 with B S G <= 1024 straddle the norm && S >= 64 route
STARTS = (0, 100, 4096)
CAPACITIES = (16, 100, 4096, 65536)  # 16 < l: n_cmp = 0


def layer_desc(cfg):
    dim, G, h, D, l, d, l_sel, n_sel, w, dt = cfg
    return _lib.NsaLayerDesc(dim=dim, G=G, h=h, Dk=D, Dv=D, l=l, d=d, l_sel=l_sel, n_sel=n_sel, w=w, gate_hidden=D // 2, dtype=dt,
                             rope_base=10000.0, rope_scale=1.0, gate_tau=1.0)


def ncmp(S, l, d):
    return 0 if S < l else (S - l) // d + 1


def sizes(L):
    out = {}
    for name, cfg in LAYERS.items():
        dim, G, h, D, l, d, l_sel, n_sel, w, dt = cfg
        desc = layer_desc(cfg)
        blk = _lib.NsaBlockDesc(attn=desc, mlp_hidden=4 * dim, norm_eps=1e-6)
        for B in BATCHES:
            for S in ROWS:
                out[f"prefill/{name}/B{B}/S{S}"] = L.nsa_layer_prefill_workspace(C.byref(desc), B, S, -(-S // l_sel))
                for t0 in STARTS:
                    S_sel, n_cmp = -(-(t0 + S) // l_sel), ncmp(t0 + S, l, d)
                    out[f"extend/{name}/B{B}/S{S}/t{t0}"] = L.nsa_layer_extend_workspace(C.byref(desc), B, S, t0, S_sel)
                    for norm in (0, 1):
                        for variant in (0, 1):
                            out[f"scores_rows/{name}/B{B}/S{S}/t{t0}/norm{norm}/v{variant}"] = L.nsa_sel_scores_rows_workspace(
                                B, S, G, h, D, n_cmp, S_sel, l, d, l_sel, dt, variant, norm)
            for S_max in CAPACITIES:
                out[f"layer_decode/{name}/B{B}/S{S_max}"] = L.nsa_layer_decode_step_workspace(C.byref(desc), B, S_max)
                out[f"block_decode/{name}/B{B}/S{S_max}"] = L.nsa_block_decode_step_workspace(C.byref(blk), B, S_max)
                out[f"sel_decode/{name}/B{B}/S{S_max}"] = L.nsa_sel_decode_step_workspace(B, G, h, D, D, ncmp(S_max, l, d), -(-S_max // l_sel) + 1,
                                                                                          n_sel, dt)
    return out


def refused(L):
    """(status, message) of calls that the dispatch layer refuses before its first HIP call.  The pointers are host memory that nothing reads."""
    out = {}
    mem = C.create_string_buffer(4096 + 256)
    p = (C.addressof(mem) + 255) & ~255  # 256-byte aligned, non-null
    desc = layer_desc(LAYERS["m7c_bf16"])
    kv = _lib.NsaKvDesc(K_sel=p, V_sel=p, K_win=p, V_win=p, K_raw=p, V_raw=p, K_cmp=p, V_cmp=p, B=1, S_max=128, n_cmp_max=7)
    pl, pk = C.byref(desc), C.byref(kv)

    def call(label, fn, *args):
        rc = fn(*args)
        out[label] = [rc, _lib.last_error()]

    def prefill(L_, kv_, S, S_sel, ws, ws_bytes, selector=_lib.NSA_SEL_BATCHED):
        return L.nsa_layer_prefill(L_, kv_, p, S, selector, p, p, p, S_sel, p, 16, p, None, ws, ws_bytes, None)

    def extend(L_, kv_, t0, S, S_sel, ws, ws_bytes):
        return L.nsa_layer_extend(L_, kv_, p, t0, S, p, p, p, S_sel, p, p, None, ws, ws_bytes, None)

    call("prefill/null_desc", prefill, None, pk, 64, 1, None, 0)
    call("extend/null_desc", extend, None, pk, 0, 64, 1, None, 0)
    zero = _lib.NsaLayerDesc()
    call("prefill/zero_desc", prefill, C.byref(zero), pk, 64, 1, None, 0)
    call("extend/zero_desc", extend, C.byref(zero), pk, 0, 64, 1, None, 0)
    call("prefill/null_cache", prefill, pl, C.byref(_lib.NsaKvDesc()), 64, 1, None, 0)
    call("extend/null_cache", extend, pl, C.byref(_lib.NsaKvDesc()), 0, 64, 1, None, 0)
    call("prefill/capacity", prefill, pl, pk, 129, 3, None, 0)
    call("extend/capacity", extend, pl, pk, 100, 29, 3, None, 0)
    call("extend/negative_t0", extend, pl, pk, -1, 29, 3, None, 0)
    call("prefill/bad_S_sel", prefill, pl, pk, 100, 1, None, 0)
    call("extend/bad_S_sel", extend, pl, pk, 64, 36, 1, None, 0)
    call("prefill/bad_selector", prefill, pl, pk, 100, 2, None, 0, 7)
    call("prefill/no_workspace", prefill, pl, pk, 100, 2, None, 0)
    call("extend/no_workspace", extend, pl, pk, 64, 36, 2, None, 0)
    need_p = L.nsa_layer_prefill_workspace(pl, 1, 100, 2)
    need_e = L.nsa_layer_extend_workspace(pl, 1, 36, 64, 2)
    call("prefill/small_workspace", prefill, pl, pk, 100, 2, p, need_p - 1)
    call("extend/small_workspace", extend, pl, pk, 64, 36, 2, p, need_e - 1)
    call("prefill/misaligned_workspace", prefill, pl, pk, 100, 2, p + 16, need_p)
    small = _lib.NsaKvDesc(K_sel=p, V_sel=p, K_win=p, V_win=p, K_raw=p, V_raw=p, K_cmp=p, V_cmp=p, B=1, S_max=128, n_cmp_max=5)
    call("prefill/cmp_cache_small", prefill, pl, C.byref(small), 128, 2, p, 1 << 40)
    call("extend/cmp_cache_small", extend, pl, C.byref(small), 64, 64, 2, p, 1 << 40)

    def decode(t, S_sel, ws, ws_bytes):
        d2 = layer_desc(LAYERS["m7c_bf16"])
        d2.W_qkv, d2.W_out = p, p
        return L.nsa_layer_decode_step(C.byref(d2), pk, p, p, t, p, p, p, S_sel, None, None, ws, ws_bytes, None)

    call("decode/position", decode, 128, 3, None, 0)
    call("decode/bad_S_sel", decode, 100, 1, None, 0)
    call("decode/no_workspace", decode, 100, 2, None, 0)
    call("decode/small_workspace", decode, 100, 2, p, L.nsa_layer_decode_step_workspace(pl, 1, 128) - 1)
    # MFMA variant on fp32: refused by the routing predicate
    call("sel_attn_fwd/mfma_f32", L.nsa_sel_attn_fwd, p, p, p, p, p, None, 1, 16, 2, 6, 64, 64, 16, 1, 2 * 16 * 64, 16 * 64, 64, 2 * 16 * 64, 16 * 64, 64,
         _lib.NSA_DT_F32, 0.0, 2, None, 0, None)
    call("band_attn_fwd/mfma_f32", L.nsa_band_attn_fwd, p, p, p, p, None, 1, 16, 2, 6, 64, 64, 16, 2 * 16 * 64, 16 * 64, 64, 2 * 16 * 64, 16 * 64, 64, 0, 0, 1, 0,
         8, _lib.NSA_DT_F32, 0.0, 2, None, 0, None)
    call("sel_attn_fwd/mfma_unaligned", L.nsa_sel_attn_fwd, p, p + 2, p, p, p, None, 1, 16, 2, 6, 64, 64, 16, 1, 2 * 16 * 64, 16 * 64, 64, 2 * 16 * 64, 16 * 64, 64,
         _lib.NSA_DT_BF16, 0.0, 2, None, 0, None)
    call("band_attn_bwd/no_workspace", L.nsa_band_attn_bwd, p, p, p, p, p, p, p, p, p, 1, 16, 2, 6, 64, 64, 16, 2 * 16 * 64, 16 * 64, 64, 2 * 16 * 64,
         16 * 64, 64, 0, 0, 1, 0, 8, _lib.NSA_DT_BF16, 0.0, 0, None, 0, None)
    call("tuning/unknown", L.nsa_hip_set_tuning, b"nope", 0)
    call("tuning/decode_stop", L.nsa_hip_set_tuning, b"DECODE_STOP", 1)
    call("tuning/decode_stop_zero", L.nsa_hip_set_tuning, b"NSA_HIP_decode_stop", 0)
    return out


def main():
    L = _lib.lib()
    tuning = {n: _lib.get_tuning(n) for n in TUNING_NAMES}  # first: nothing has set a switch yet
    print(json.dumps({"tuning": tuning, "sizes": sizes(L), "refused": refused(L)}, indent=0, sort_keys=True))


if __name__ == "__main__":
    main()
