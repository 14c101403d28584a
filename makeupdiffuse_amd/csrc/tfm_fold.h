// The fold recipe of a transformer block, on fp32 device pointers; mkd_ctx::finalize (engine.hip) and the stand-alone mkd_tfm_tail /
// mkd_tfm_head handles (api_kernels.hip) both build their weights here
#pragma once
#include "mkd_common.h"

#include <functional>

// LayerNorm folded into its consumer GEMM: W' = W*gamma (bf16), s = rowsum(W'), b' = b + W.beta
struct Folded { bf16_t* w = nullptr; float* s = nullptr; float* b = nullptr; };
typedef std::function<int(void**, size_t)> AllocFn;
static int alloc_folded(const AllocFn& al, size_t n, size_t k, Folded* f) {
    int rc = al((void**)&f->w, n * k * sizeof(bf16_t));
    if (!rc) rc = al((void**)&f->s, n * sizeof(float));
    if (!rc) rc = al((void**)&f->b, n * sizeof(float));
    return rc;
}
// attn1: [to_q; to_k; to_v] . LN1
static int fold_ln1_qkv(const float* to_q, const float* to_k, const float* to_v, const float* gamma, const float* beta, int d, const AllocFn& al, Folded* f) {
    int rc = alloc_folded(al, (size_t)3 * d, d, f);
    const float* parts[3] = {to_q, to_k, to_v};
    for (int j = 0; j < 3 && !rc; ++j) rc = launch_fold_layernorm(parts[j], gamma, beta, nullptr, d, d, f->w, j * d, 1, f->s, f->b, 0);
    return rc;
}
// attn2.to_q . LN2
static int fold_ln2_q(const float* to_q, const float* gamma, const float* beta, int d, const AllocFn& al, Folded* f) {
    int rc = alloc_folded(al, d, d, f);
    if (!rc) rc = launch_fold_layernorm(to_q, gamma, beta, nullptr, d, d, f->w, 0, 1, f->s, f->b, 0);
    return rc;
}
// ff.net.0.proj [8d][d] . LN3: rows [0,4d) = value, [4d,8d) = gate  ->  row 2j = value_j, row 2j+1 = gate_j
static int fold_ln3_geglu(const float* w, const float* bias, const float* gamma, const float* beta, int d, const AllocFn& al, Folded* f) {
    const int inner = 4 * d;
    int rc = alloc_folded(al, (size_t)2 * inner, d, f);
    for (int half = 0; half < 2 && !rc; ++half)
        rc = launch_fold_layernorm(w + (size_t)half * inner * d, gamma, beta, bias + half * inner, inner, d, f->w, half, 2, f->s, f->b, 0);
    return rc;
}
// FF2 and proj_out are both linear with nothing in between: one GEMM over [gg | h2] (K = 5d)
static int merge_ff_out(const float* proj_out_w, const float* ff2_w, const float* ff2_b, const float* proj_out_b, int d, const AllocFn& al,
                        bf16_t** wm, float** bm) {
    int rc = al((void**)wm, (size_t)d * 5 * d * sizeof(bf16_t));
    if (!rc) rc = al((void**)bm, (size_t)d * sizeof(float));
    if (!rc) rc = launch_merge_ff_out(proj_out_w, ff2_w, ff2_b, proj_out_b, *wm, *bm, d, 0);
    return rc;
}
