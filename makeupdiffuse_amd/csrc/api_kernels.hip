// libmkd single-kernel entry points (unit tests, tuners, tools): each runs one launcher on the caller's buffers and uses no mkd_ctx.
// The GEMM family shares one zero page, one split-K workspace and one path from arguments to launch.
#include "mkd_common.h"
#include "tfm_fold.h"
#include "../../include/mkd.h"

#include <cstring>
#include <string>
#include <vector>

static bf16_t* g_zero = nullptr;
static float* g_ws = nullptr; static size_t g_ws_bytes = 0;
static float* g_gn = nullptr; static size_t g_gn_bytes = 0;

static int scratch(float** p, size_t* have, size_t need) {
    if (*have >= need && *p) return 0;
    if (*p) { hipDeviceSynchronize(); hipFree(*p); *p = nullptr; }
    MKD_HIP_CHECK(hipMalloc((void**)p, need ? need : 256));
    *have = need;
    return 0;
}
static int zero_page() {
    if (g_zero) return 0;
    MKD_HIP_CHECK(hipMalloc((void**)&g_zero, 4096));
    MKD_HIP_CHECK(hipMemset(g_zero, 0, 4096));
    return 0;
}
// what every GEMM entry sets: operands, bias, output, shape, scale 1 and the zero page (zero_page() comes first)
static GemmArgs gemm_args(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, void* C, int ldc, int M, int N, int K) {
    GemmArgs a; memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.bias = bias; a.scale = 1.0f; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
    a.zero = g_zero;
    return a;
}
static void conv_geometry(GemmArgs& a, int Hin, int Win, int Cin, int Hout, int Wout, int stride, int up, int pad_tl, int splitk) {
    a.conv = 1; a.Hin = Hin; a.Win = Win; a.Cin = Cin; a.Hout = Hout; a.Wout = Wout; a.stride = stride; a.up = up; a.pad_tl = pad_tl;
    a.splitk = splitk > 0 ? splitk : 0;
}
// the parameters that the mkd_gemm_* family shares in the ABI (include/mkd.h), as launch arguments
static GemmArgs gemm_abi_args(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, const float* rowbias, int ldrb,
                              int rows_per_batch, const uint16_t* R, int ldr, float scale, int act, void* C, int ldc, int out_f32, int M,
                              int N, int K, int conv3x3, int Hin, int Win, int Cin, int Hout, int Wout, int stride, int up, int splitk) {
    GemmArgs a = gemm_args(A, lda, W, ldw, bias, C, ldc, M, N, K);
    a.rowbias = rowbias; a.ldrb = ldrb; a.rows_per_batch = rows_per_batch; a.R = R; a.ldr = ldr; a.scale = scale; a.act = act; a.out_f32 = out_f32;
    conv_geometry(a, Hin, Win, Cin, Hout, Wout, stride, up, 1, splitk);
    a.conv = conv3x3 ? 1 : 0;
    return a;
}
// the decision launch_gemm will take (fallbacks included), the split-K workspace grown for it and bound, the launch
static int gemm_run(GemmArgs& a, void* stream) {
    int cfg_i = 0, s = 1;
    int rc = gemm_resolve(a, &cfg_i, &s);
    if (rc) return rc;
    rc = scratch(&g_ws, &g_ws_bytes, gemm_ws_bytes(a.M, a.N, s > 1 ? s : 2));
    if (rc) return rc;
    a.ws = g_ws; a.ws_bytes = g_ws_bytes;
    return launch_gemm(a, (hipStream_t)stream);
}

static int gemm_entry(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, const float* rowbias, int ldrb,
                      int rows_per_batch, const uint16_t* R, int ldr, float scale, int act, void* C, int ldc, int out_f32, int M,
                      int N, int K, int conv3x3, int batch, int Hin, int Win, int Cin, int Hout, int Wout, int stride, int up,
                      int splitk, long long* gn_stat, int gn_cg, int gn_coff, int gn_hw, void* stream) {
    if (!A || !W || !C) return mkd_fail(MKD_ERR_ARG, "mkd_gemm_bf16: null pointer");
    if (int rc = zero_page()) return rc;
    if (conv3x3 && M != batch * Hout * Wout) return mkd_fail(MKD_ERR_ARG, "mkd_gemm_bf16: M != batch*Hout*Wout");
    GemmArgs a = gemm_abi_args(A, lda, W, ldw, bias, rowbias, ldrb, rows_per_batch, R, ldr, scale, act, C, ldc, out_f32, M, N, K, conv3x3,
                               Hin, Win, Cin, Hout, Wout, stride, up, splitk);
    a.gn_stat = gn_stat; a.gn_cg = gn_cg; a.gn_coff = gn_coff; a.gn_hw = gn_hw;
    return gemm_run(a, stream);
}

extern "C" {

int mkd_gemm_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, const float* rowbias, int ldrb,
                  int rows_per_batch, const uint16_t* R, int ldr, float scale, int act, void* C, int ldc, int out_f32, int M,
                  int N, int K, int conv3x3, int batch, int Hin, int Win, int Cin, int Hout, int Wout, int stride, int up,
                  int splitk, void* stream) {
    return gemm_entry(A, lda, W, ldw, bias, rowbias, ldrb, rows_per_batch, R, ldr, scale, act, C, ldc, out_f32, M, N, K, conv3x3, batch,
                      Hin, Win, Cin, Hout, Wout, stride, up, splitk, nullptr, 0, 0, 0, stream);
}
int mkd_conv3x3_down_bf16(const uint16_t* x, int ldx, const uint16_t* w_packed, const float* bias, uint16_t* y, int ldy, int batch, int H, int W,
                          int Cin, int Cout, int splitk, void* stream) {
    if (!x || !w_packed || !y) return mkd_fail(MKD_ERR_ARG, "mkd_conv3x3_down_bf16: null pointer");
    if (batch <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2) return mkd_fail(MKD_ERR_ARG, "mkd_conv3x3_down_bf16: H, W must be even");
    if (int rc = zero_page()) return rc;
    GemmArgs a = gemm_args(x, ldx, w_packed, 9 * Cin, bias, y, ldy, batch * (H / 2) * (W / 2), Cout, 9 * Cin);
    conv_geometry(a, H, W, Cin, H / 2, W / 2, 2, 0, /*pad_tl=*/0, splitk);
    return gemm_run(a, stream);
}
int mkd_conv3x3_fold_bf16(const uint16_t* x, int ldx, const uint16_t* w_fold, const float* bias, const uint16_t* x2, int ldx2, int K2, uint16_t* y,
                          int ldy, int batch, int H, int W, int Cin, int N, int splitk, void* stream) {
    if (!x || !w_fold || !x2 || !y) return mkd_fail(MKD_ERR_ARG, "mkd_conv3x3_fold_bf16: null pointer");
    if (int rc = zero_page()) return rc;
    GemmArgs a = gemm_args(x, ldx, w_fold, 9 * Cin + K2, bias, y, ldy, batch * H * W, N, 9 * Cin + K2);
    conv_geometry(a, H, W, Cin, H, W, 1, 0, 1, splitk);
    a.A2 = x2; a.lda2 = ldx2; a.K2 = K2;
    return gemm_run(a, stream);
}
int mkd_gemm_gnstat_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, const float* rowbias, int ldrb,
                         int rows_per_batch, const uint16_t* R, int ldr, float scale, int act, void* C, int ldc, int out_f32, int M,
                         int N, int K, int conv3x3, int batch, int Hin, int Win, int Cin, int Hout, int Wout, int stride, int up,
                         int splitk, int64_t* gn_stat, int gn_cg, int gn_coff, int gn_hw, void* stream) {
    if (!gn_stat) return mkd_fail(MKD_ERR_ARG, "mkd_gemm_gnstat_bf16: null statistics buffer");
    return gemm_entry(A, lda, W, ldw, bias, rowbias, ldrb, rows_per_batch, R, ldr, scale, act, C, ldc, out_f32, M, N, K, conv3x3, batch,
                      Hin, Win, Cin, Hout, Wout, stride, up, splitk, (long long*)gn_stat, gn_cg, gn_coff, gn_hw, stream);
}
int mkd_gemm_groupnorm_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, const float* rowbias, int ldrb,
                            int rows_per_batch, const uint16_t* R, int ldr, float scale, void* C, int ldc, int write_raw, int M, int N,
                            int K, int conv3x3, int batch, int Hin, int Win, int Cin, int Hout, int Wout, int stride, int up, int splitk,
                            int rows_per_sample, const float* gamma, const float* beta, float eps, int silu, uint16_t* y, int ld_y,
                            void* stream) {
    if (!A || !W || (!C && write_raw) || !gamma || !beta || !y) return mkd_fail(MKD_ERR_ARG, "mkd_gemm_groupnorm_bf16: null pointer");
    if (rows_per_sample <= 0 || M % rows_per_sample) return mkd_fail(MKD_ERR_ARG, "mkd_gemm_groupnorm_bf16: M must be a multiple of rows_per_sample");
    if (int rc = zero_page()) return rc;
    if (conv3x3 && M != batch * Hout * Wout) return mkd_fail(MKD_ERR_ARG, "mkd_gemm_groupnorm_bf16: M != batch*Hout*Wout");
    const int nb = M / rows_per_sample;
    if (!gn_from_slabs_supported(nb, rows_per_sample, N)) return mkd_fail(MKD_ERR_UNSUPPORTED, "mkd_gemm_groupnorm_bf16: GroupNorm geometry does not fit the single-pass kernel");
    GemmArgs a = gemm_abi_args(A, lda, W, ldw, bias, rowbias, ldrb, rows_per_batch, R, ldr, scale, /*act=*/0, C, ldc, /*out_f32=*/0, M, N, K, conv3x3,
                               Hin, Win, Cin, Hout, Wout, stride, up, splitk);
    int cfg_i = 0, s = 1;
    int rc = gemm_resolve(a, &cfg_i, &s);
    if (rc) return rc;
    if (s < 2) return mkd_fail(MKD_ERR_UNSUPPORTED, "mkd_gemm_groupnorm_bf16: this shape is not split over K");
    a.defer_epilogue = 1;          // the partial slabs stay in the workspace: the GroupNorm kernel below reduces them
    rc = gemm_run(a, stream);
    if (rc) return rc;
    a.splitk = s;
    if (!write_raw) a.C = nullptr;
    return launch_gn_from_slabs(a, gamma, beta, eps, silu, y, ld_y, nb, rows_per_sample, (hipStream_t)stream);
}
int mkd_gn_colstats(const uint16_t* x, int ld, int batch, int hw, int ncols, int cg, int coff, int64_t* gstat, void* stream) {
    if (!x || !gstat) return mkd_fail(MKD_ERR_ARG, "mkd_gn_colstats: null pointer");
    return launch_gn_colstats(x, ld, batch, hw, ncols, cg, coff, (long long*)gstat, (hipStream_t)stream);
}
int mkd_gn_apply_stats(const uint16_t* x, int ld_in, const float* gamma, const float* beta, float eps, int silu, uint16_t* y,
                       int ld_out, int batch, int hw, int C, const int64_t* gstat, void* stream) {
    if (!x || !y || !gamma || !beta || !gstat) return mkd_fail(MKD_ERR_ARG, "mkd_gn_apply_stats: null pointer");
    return launch_gn_apply_stats(x, ld_in, gamma, beta, eps, silu, y, ld_out, batch, hw, C, (const long long*)gstat, (hipStream_t)stream);
}
int mkd_fold_layernorm(const float* w, const float* gamma, const float* beta, const float* bias, int N, int K, uint16_t* w_out,
                       int dst_row0, int dst_row_mul, float* s_out, float* b_out, void* stream) {
    if (!w || !gamma || !beta || !w_out || !s_out || !b_out) return mkd_fail(MKD_ERR_ARG, "mkd_fold_layernorm: null pointer");
    return launch_fold_layernorm(w, gamma, beta, bias, N, K, w_out, dst_row0, dst_row_mul, s_out, b_out, (hipStream_t)stream);
}
int mkd_gemm_ln_bf16(const uint16_t* A, int lda, const uint16_t* Wfold, int ldw, const float* bias_fold, const float* ln_s,
                     const float* row_stats, int stat_slots, float eps, int act, void* C, int ldc, int M, int N, int K, void* stream) {
    if (!A || !Wfold || !C || !ln_s) return mkd_fail(MKD_ERR_ARG, "mkd_gemm_ln_bf16: null pointer");          // row_stats null: on the fly
    if (int rc = zero_page()) return rc;
    GemmArgs a = gemm_args(A, lda, Wfold, ldw, bias_fold, C, ldc, M, N, K);
    a.act = act; a.rows_per_batch = 1; a.ln_s = ln_s; a.ln_eps = eps; a.stat_in = row_stats; a.stat_in_slots = stat_slots;
    return launch_gemm(a, (hipStream_t)stream);          // (row statistics over the whole row: never split over K, no workspace)
}
int mkd_gemm_rowstats_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, const uint16_t* R, int ldr,
                           uint16_t* C, int ldc, int M, int N, int K, float* stat_out, int stat_capacity_slots, int* slots_out,
                           void* stream) {
    if (!A || !W || !C || !stat_out || !slots_out) return mkd_fail(MKD_ERR_ARG, "mkd_gemm_rowstats_bf16: null pointer");
    if (int rc = zero_page()) return rc;
    const int slots = gemm_stat_slots(M, N, K);
    if (slots > stat_capacity_slots) return mkd_fail(MKD_ERR_ARG, "mkd_gemm_rowstats_bf16: statistics buffer too small");
    *slots_out = slots;
    GemmArgs a = gemm_args(A, lda, W, ldw, bias, C, ldc, M, N, K);
    a.R = R; a.ldr = ldr; a.rows_per_batch = 1; a.stat_out = stat_out;
    return gemm_run(a, stream);
}
int mkd_groupnorm(const uint16_t* x, int ld_in, const float* gamma, const float* beta, float eps, int silu, uint16_t* y,
                  int ld_out, int batch, int hw, int C, int groups, void* stream) {
    int rc = scratch(&g_gn, &g_gn_bytes, groupnorm_partials_bytes(batch, hw, groups));
    if (rc) return rc;
    return launch_groupnorm(x, ld_in, gamma, beta, eps, silu, y, ld_out, batch, hw, C, groups, g_gn, (hipStream_t)stream);
}
int mkd_layernorm(const uint16_t* x, const float* gamma, const float* beta, float eps, uint16_t* y, int rows, int d, void* stream) {
    return launch_layernorm(x, gamma, beta, eps, y, rows, d, (hipStream_t)stream);
}
int mkd_layernorm_ld(const uint16_t* x, int ldx, const float* gamma, const float* beta, float eps, uint16_t* y, int rows, int d, void* stream) {
    return launch_layernorm(x, gamma, beta, eps, y, rows, d, (hipStream_t)stream, ldx);
}
int mkd_attention(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv, uint16_t* o, int ldo,
                  int batch, int Tq, int Tk, int heads, int dh, float scale, void* stream) {
    return launch_attention(q, ldq, k, ldk, v, ldv, o, ldo, batch, Tq, Tk, heads, dh, scale, (hipStream_t)stream);
}
int mkd_attention_causal(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv, uint16_t* o, int ldo,
                         int batch, int Tq, int Tk, int heads, int dh, float scale, void* stream) {
    return launch_attention(q, ldq, k, ldk, v, ldv, o, ldo, batch, Tq, Tk, heads, dh, scale, (hipStream_t)stream, 1);
}
int mkd_geglu(const uint16_t* x, uint16_t* y, int rows, int inner, void* stream) {
    return launch_geglu(x, y, rows, inner, (hipStream_t)stream);
}
int mkd_softmax_rows(const float* x, uint16_t* y, int rows, int cols, void* stream) {
    return launch_softmax_rows(x, y, rows, cols, (hipStream_t)stream);
}
int mkd_vae_enc_tail(const uint16_t* x, const uint16_t* w, const float* bias, const uint16_t* wq, const float* bq, const float* noise,
                     float scale, float* z_out, float* moments_out, int batch, int H, int W, int Cin, int z_channels, void* stream) {
    return launch_vae_enc_tail(x, w, bias, wq, bq, noise, scale, z_out, moments_out, batch, H, W, Cin, z_channels, (hipStream_t)stream);
}
int mkd_post_quant(const float* z, const uint16_t* w, const float* bias, float inv_scale, float* out, int batch, int C, int hw, void* stream) {
    return launch_post_quant(z, w, bias, inv_scale, out, batch, C, hw, (hipStream_t)stream);
}
int mkd_timestep_embedding(const int64_t* t, uint16_t* out, int batch, int dim, void* stream) {
    return launch_timestep_embedding(t, out, batch, dim, (hipStream_t)stream);
}
int mkd_clip_embed(const int32_t* tokens, const uint16_t* tok_emb, const uint16_t* pos_emb, uint16_t* out, int batch, int T, int width,
                   int vocab, void* stream) {
    return launch_clip_embed(tokens, tok_emb, pos_emb, out, batch, T, width, vocab, (hipStream_t)stream);
}
int mkd_blend_bf16(const uint16_t* a, const uint16_t* b, const float* alpha, uint16_t* y, int64_t per_sample, int batch, void* stream) {
    return launch_blend(a, b, alpha, y, per_sample, batch, (hipStream_t)stream);
}
int mkd_conv3x3_direct(const void* x, int in_nchw_f32, const uint16_t* w, const float* bias, void* y, int out_nchw_f32, int act,
                       const uint16_t* add, int batch, int Hin, int Win, int Cin, int Cout, int stride, void* stream) {
    return launch_conv3x3_direct(x, in_nchw_f32, w, bias, y, out_nchw_f32, act, add, batch, Hin, Win, Cin, Cout, stride,
                                 (hipStream_t)stream);
}
int mkd_pack_conv_weight(const float* w, uint16_t* out, int Cout, int Cin, int kh, int kw, void* stream) {
    return launch_pack_conv_weight(w, out, Cout, Cin, kh, kw, (hipStream_t)stream);
}

// ---- fused transformer tail, stand-alone (unit parity test, tools/bench_tfm_tail.py) ------------------------------------------
struct mkd_tfm_tail { int d = 0; bf16_t* wpk = nullptr; float* vec = nullptr; bf16_t* kvp = nullptr; int kv_batch = 0, Tk = 0; std::vector<void*> owned; };
void mkd_tfm_tail_destroy(mkd_tfm_tail* h) {
    if (!h) return;
    for (void* p : h->owned) hipFree(p);
    delete h;
}
int mkd_tfm_tail_create(int d, const float* to_out1_w, const float* to_out1_b, const float* norm2_g, const float* norm2_b,
                        const float* to_q2_w, const float* to_out2_w, const float* to_out2_b, const float* norm3_g, const float* norm3_b,
                        const float* ff0_w, const float* ff0_b, const float* ff2_w, const float* ff2_b, const float* proj_out_w,
                        const float* proj_out_b, mkd_tfm_tail** out) {
    if (!out) return mkd_fail(MKD_ERR_ARG, "null out");
    if (!tfm_tail_weight_bytes(d)) return mkd_fail(MKD_ERR_UNSUPPORTED, "tfm_tail: only d = 320 is built");
    mkd_tfm_tail* h = new mkd_tfm_tail; h->d = d;
    const AllocFn dal = [h](void** o, size_t bytes) -> int { MKD_HIP_CHECK(hipMalloc(o, bytes)); h->owned.push_back(*o); return 0; };
    void *wo1 = nullptr, *wo2 = nullptr;
    Folded q2, ffg; bf16_t* wm = nullptr; float* bm = nullptr;
    const size_t dd = (size_t)d * d;
    int rc = dal(&wo1, dd * 2);
    if (!rc) rc = dal(&wo2, dd * 2);
    if (!rc) rc = dal((void**)&h->wpk, tfm_tail_weight_bytes(d));
    if (!rc) rc = dal((void**)&h->vec, tfm_tail_vec_bytes(d));
    if (!rc) rc = launch_f32_to_bf16(to_out1_w, (bf16_t*)wo1, (int64_t)dd, 0);
    if (!rc) rc = launch_f32_to_bf16(to_out2_w, (bf16_t*)wo2, (int64_t)dd, 0);
    if (!rc) rc = fold_ln2_q(to_q2_w, norm2_g, norm2_b, d, dal, &q2);
    if (!rc) rc = fold_ln3_geglu(ff0_w, ff0_b, norm3_g, norm3_b, d, dal, &ffg);
    if (!rc) rc = merge_ff_out(proj_out_w, ff2_w, ff2_b, proj_out_b, d, dal, &wm, &bm);
    if (!rc) {
        TfmTailWeights s{(const bf16_t*)wo1, to_out1_b, q2.w, q2.s, q2.b, (const bf16_t*)wo2, to_out2_b, ffg.w, ffg.s, ffg.b, wm, bm};
        rc = tfm_tail_pack_weights(d, s, h->wpk, h->vec, 0);
    }
    if (rc) { mkd_tfm_tail_destroy(h); return rc; }
    *out = h;
    return 0;
}
/* experiment builds (-DMKD_TFM_TRACE) only: device buffer [workgroups][8][32] of int64 time stamps; a no-op in the product build */
int mkd_debug_tfm_trace(long long* buf) { tfm_tail_set_trace(buf); return 0; }
int mkd_debug_attn_trace(long long* buf) { return attn_set_trace(buf); }
int mkd_tfm_tail_set_context(mkd_tfm_tail* h, const uint16_t* kv, int ldkv, int batch, int Tk, void* stream) {
    if (!h) return mkd_fail(MKD_ERR_ARG, "null handle");
    if (batch > h->kv_batch) {
        void* p = nullptr;
        MKD_HIP_CHECK(hipMalloc(&p, tfm_tail_kv_bytes(h->d, batch)));
        h->owned.push_back(p); h->kvp = (bf16_t*)p; h->kv_batch = batch;
    }
    h->Tk = Tk;
    return launch_tfm_tail_pack_kv(h->d, kv, ldkv, batch, Tk, h->kvp, (hipStream_t)stream);
}
int mkd_tfm_tail_run(mkd_tfm_tail* h, const uint16_t* a1, int lda, const uint16_t* h0, int ldh, const uint16_t* xin, int ldx, uint16_t* out,
                     int ldo, int M, int T, void* stream) {
    if (!h || !h->kvp) return mkd_fail(MKD_ERR_STATE, "tfm_tail: set the context first");
    if (T <= 0 || M % T || M / T > h->kv_batch) return mkd_fail(MKD_ERR_ARG, "tfm_tail: M must be samples x T within the packed context");
    return launch_tfm_tail(h->d, h->wpk, h->vec, a1, lda, h0, ldh, xin, ldx, h->kvp, out, ldo, M, T, h->Tk, (hipStream_t)stream);
}

// ---- fused transformer head, stand-alone (unit parity test) ---------------------------------------------------------------------
struct mkd_tfm_head { int d = 0; bf16_t* wpk = nullptr; float* vec = nullptr; float* part = nullptr; size_t part_bytes = 0; std::vector<void*> owned; };
void mkd_tfm_head_destroy(mkd_tfm_head* h) {
    if (!h) return;
    for (void* p : h->owned) hipFree(p);
    delete h;
}
int mkd_tfm_head_create(int d, const float* gn_g, const float* gn_b, const float* proj_in_w, const float* proj_in_b, const float* norm1_g,
                        const float* norm1_b, const float* to_q_w, const float* to_k_w, const float* to_v_w, mkd_tfm_head** out) {
    if (!out) return mkd_fail(MKD_ERR_ARG, "null out");
    if (!tfm_head_weight_bytes(d)) return mkd_fail(MKD_ERR_UNSUPPORTED, "tfm_head: only d = 320 is built");
    mkd_tfm_head* h = new mkd_tfm_head; h->d = d;
    const AllocFn dal = [h](void** o, size_t bytes) -> int { MKD_HIP_CHECK(hipMalloc(o, bytes)); h->owned.push_back(*o); return 0; };
    void* wpi = nullptr; Folded qkv;
    const size_t dd = (size_t)d * d;
    int rc = dal(&wpi, dd * 2);
    if (!rc) rc = dal((void**)&h->wpk, tfm_head_weight_bytes(d));
    if (!rc) rc = dal((void**)&h->vec, tfm_head_vec_bytes(d));
    if (!rc) rc = launch_f32_to_bf16(proj_in_w, (bf16_t*)wpi, (int64_t)dd, 0);
    if (!rc) rc = fold_ln1_qkv(to_q_w, to_k_w, to_v_w, norm1_g, norm1_b, d, dal, &qkv);
    if (!rc) {
        TfmHeadWeights s{gn_g, gn_b, (const bf16_t*)wpi, proj_in_b, qkv.w, qkv.s, qkv.b};
        rc = tfm_head_pack_weights(d, s, h->wpk, h->vec, 0);
    }
    if (rc) { mkd_tfm_head_destroy(h); return rc; }
    *out = h;
    return 0;
}
int mkd_tfm_head_run(mkd_tfm_head* h, const uint16_t* x, int ldx, float gn_eps, uint16_t* h0, uint16_t* qkv, int batch, int T, void* stream) {
    if (!h) return mkd_fail(MKD_ERR_ARG, "null handle");
    const size_t need = groupnorm_partials_bytes(batch, T, 32);
    if (need > h->part_bytes) {
        void* p = nullptr;
        MKD_HIP_CHECK(hipMalloc(&p, need));
        h->owned.push_back(p); h->part = (float*)p; h->part_bytes = need;
    }
    int nch = 0;
    int rc = launch_gn_stats(x, ldx, batch, T, h->d, 32, h->part, (hipStream_t)stream, &nch);
    if (rc) return rc;
    return launch_tfm_head(h->d, h->wpk, h->vec, x, ldx, h->part, nch, gn_eps, h0, qkv, batch * T, T, (hipStream_t)stream);
}

}  // extern "C"
