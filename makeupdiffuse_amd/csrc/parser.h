// Launchers of kernels_parser.hip (the face-parsing network's own kernels); each only enqueues on `stream`.
#pragma once
#include "mkd_common.h"

constexpr int PARSER_GATE_MAX = 2048;       // channels / mat-vec outputs a channel gate handles
constexpr int PARSER_STEM_MAX = 128;        // stem output channels (its bf16 weights live in LDS)

size_t parser_stem_lds_bytes(int C0);
// x fp32 NCHW [B,3,H,W] in [0,1] -> y bf16 NHWC [B,H/2,W/2,C0]; w bf16 [(ky*7+kx)*3+c][C0] and bias [C0] with the BN folded in
int launch_parser_stem_conv(const float* x, const bf16_t* w, const float* bias, bf16_t* y, int batch, int H, int W, int C0, const float* mean,
                            const float* stdv, hipStream_t stream);
int launch_parser_maxpool(const bf16_t* x, bf16_t* y, int batch, int Hin, int Win, int C, hipStream_t stream);      // 3x3 s2 p1, dense NHWC
int launch_parser_subsample(const bf16_t* x, int ldx, bf16_t* y, int batch, int Hin, int Win, int C, hipStream_t stream);
int launch_parser_gate(const bf16_t* x, int ldx, int batch, int pixels, int C, const float* w1, const float* b1, int n1, int act1, const float* w2,
                       const float* b2, int n2, int act2, float* out, hipStream_t stream);
int launch_parser_gate_apply(const bf16_t* x, int ldx, const float* a, int mode, const float* v, const bf16_t* r, int ldr, bf16_t* y, int ldy, int batch,
                             int h, int w, int C, int u, hipStream_t stream);
int launch_parser_head(const float* logits, int64_t s_class, int64_t s_row, int64_t s_col, int64_t s_batch, int batch, int n_classes, int h8, int w8,
                       int P_h, int P_w, int out_h, int out_w, const uint8_t* lut, uint8_t* labels, hipStream_t stream);
int launch_parser_logits_nchw(const float* x, int ld, float* y, int batch, int hw, int n_classes, hipStream_t stream);
