// The face-parsing network as a stand-alone handle (include/mkd.h: mkd_parser_*): parameter table, BatchNorm fold and weight packing
// on the host at finalize, and the launch sequence.  UPSTREAM: zllrunning/face-parsing.PyTorch model.py / resnet.py (BiSeNet with a
// ResNet-18 context path) as vendored by PSGAN / EleGANt faceutils/mask; the reference reaches it from diffdata/preprocessing.py:38.
// Every 3x3 and 1x1 convolution runs on launch_gemm (bf16 NHWC, fp32 accumulation, ReLU = epilogue code 4); the rest is kernels_parser.hip.
#include "mkd_common.h"
#include "parser.h"
#include "../../include/mkd.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

struct Param { std::vector<int64_t> shape; std::vector<float> data; bool loaded = false; };
struct PackItem { std::string key, conv, bn; int kind, pad_rows_to; };       // kind 0: bf16 GEMM weight; 1: fp32 gate weight; 2: the stem
struct ConvW { size_t w_off = 0, b_off = 0; int cout = 0, cin = 0, k = 0; bool has_bias = false; };       // offsets into the packed device block

uint16_t host_bf16(float f) {             // round to nearest even (finite inputs; NaN stays NaN)
    uint32_t u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

bool ignorable(const std::string& n) {    // training-only heads and BatchNorm's step counter
    static const char* tail = "num_batches_tracked";
    if (n.rfind("conv_out16.", 0) == 0 || n.rfind("conv_out32.", 0) == 0) return true;
    return n.size() >= strlen(tail) && n.compare(n.size() - strlen(tail), strlen(tail), tail) == 0;
}

}  // namespace

struct mkd_parser {
    mkd_parser_config cfg;
    std::map<std::string, Param> params;          // sorted by name
    bool finalized = false;
    std::vector<PackItem> items;                  // what finalize folds and packs, in order
    std::map<std::string, ConvW> packed;          // shapes from create on, offsets from finalize on
    char* wdev = nullptr;
    bf16_t* zero = nullptr;
    char* ws = nullptr; size_t ws_cap = 0;
    int launches = 0;

    int ncp() const { return (cfg.n_classes + 3) & ~3; }          // logit columns: classes padded to the GEMM's multiple of 4
    void add(const std::string& n, std::vector<int64_t> s) { params[n].shape = std::move(s); }
    void add_bn(const std::string& n, int c) { for (const char* f : {"weight", "bias", "running_mean", "running_var"}) add(n + "." + f, {c}); }
    void add_conv(const std::string& n, int co, int ci, int k) { add(n + ".weight", {co, ci, k, k}); }
    void build_table();
    int finalize();
    int run(const float* images, int batch, int H, int W, char* base, size_t* need, double* flops, int* launches_out, float** logits_out, hipStream_t stream) const;
    int forward(const float* images, int batch, int H, int W, float** logits_out, hipStream_t stream);
    ~mkd_parser() {
        if (wdev || ws || zero) hipDeviceSynchronize();
        if (wdev) hipFree(wdev);
        if (ws) hipFree(ws);
        if (zero) hipFree(zero);
    }
};

void mkd_parser::build_table() {
    const int* w = cfg.widths;
    const int cp = cfg.cp_channels, ff = cfg.ffm_channels;
    add_conv("cp.resnet.conv1", w[0], 3, 7);
    add_bn("cp.resnet.bn1", w[0]);
    int cin = w[0];
    for (int L = 0; L < 4; ++L)
        for (int i = 0; i < cfg.blocks[L]; ++i) {
            const std::string P = "cp.resnet.layer" + std::to_string(L + 1) + "." + std::to_string(i);
            const int stride = (i == 0 && L > 0) ? 2 : 1;
            add_conv(P + ".conv1", w[L], cin, 3); add_bn(P + ".bn1", w[L]);
            add_conv(P + ".conv2", w[L], w[L], 3); add_bn(P + ".bn2", w[L]);
            if (cin != w[L] || stride != 1) { add_conv(P + ".downsample.0", w[L], cin, 1); add_bn(P + ".downsample.1", w[L]); }
            cin = w[L];
        }
    for (int k = 0; k < 2; ++k) {
        const std::string A = k ? "cp.arm32" : "cp.arm16";
        add_conv(A + ".conv.conv", cp, k ? w[3] : w[2], 3); add_bn(A + ".conv.bn", cp);
        add_conv(A + ".conv_atten", cp, cp, 1); add_bn(A + ".bn_atten", cp);
        const std::string Hd = k ? "cp.conv_head32" : "cp.conv_head16";
        add_conv(Hd + ".conv", cp, cp, 3); add_bn(Hd + ".bn", cp);
    }
    add_conv("cp.conv_avg.conv", cp, w[3], 1); add_bn("cp.conv_avg.bn", cp);
    add_conv("ffm.convblk.conv", ff, w[1] + cp, 1); add_bn("ffm.convblk.bn", ff);
    add_conv("ffm.conv1", ff / 4, ff, 1);
    add_conv("ffm.conv2", ff, ff / 4, 1);
    add_conv("conv_out.conv.conv", ff, ff, 3); add_bn("conv_out.conv.bn", ff);
    add_conv("conv_out.conv_out", cfg.n_classes, ff, 1);

    auto item = [&](const std::string& key, const std::string& conv, const std::string& bn, int kind, int pad_rows_to) {
        items.push_back({key, conv, bn, kind, pad_rows_to});
        const Param& W = params[conv + ".weight"];
        ConvW c; c.cout = std::max((int)W.shape[0], pad_rows_to); c.cin = (int)W.shape[1]; c.k = (int)W.shape[2]; c.has_bias = !bn.empty();
        packed[key] = c;
    };
    item("stem", "cp.resnet.conv1", "cp.resnet.bn1", 2, 0);
    for (int L = 0; L < 4; ++L)
        for (int i = 0; i < cfg.blocks[L]; ++i) {
            const std::string P = "cp.resnet.layer" + std::to_string(L + 1) + "." + std::to_string(i);
            item(P + ".conv1", P + ".conv1", P + ".bn1", 0, 0);
            item(P + ".conv2", P + ".conv2", P + ".bn2", 0, 0);
            if (params.count(P + ".downsample.0.weight")) item(P + ".down", P + ".downsample.0", P + ".downsample.1", 0, 0);
        }
    for (const char* A : {"cp.arm16", "cp.arm32"}) {
        item(std::string(A) + ".conv", std::string(A) + ".conv.conv", std::string(A) + ".conv.bn", 0, 0);
        item(std::string(A) + ".atten", std::string(A) + ".conv_atten", std::string(A) + ".bn_atten", 1, 0);
    }
    item("cp.conv_head16", "cp.conv_head16.conv", "cp.conv_head16.bn", 0, 0);
    item("cp.conv_head32", "cp.conv_head32.conv", "cp.conv_head32.bn", 0, 0);
    item("cp.conv_avg", "cp.conv_avg.conv", "cp.conv_avg.bn", 1, 0);
    item("ffm.convblk", "ffm.convblk.conv", "ffm.convblk.bn", 0, 0);
    item("ffm.conv1", "ffm.conv1", "", 1, 0);
    item("ffm.conv2", "ffm.conv2", "", 1, 0);
    item("conv_out.conv", "conv_out.conv.conv", "conv_out.conv.bn", 0, 0);
    item("conv_out.conv_out", "conv_out.conv_out", "", 0, ncp());
}

// Fold + pack on the host, one upload.  W' = W * g / sqrt(var + eps), b' = beta - mean * g / sqrt(var + eps), all fp32; GEMM weights are
// then rounded to bf16 in [Cout][ky][kx][Cin] order, gate weights stay fp32 [Cout][Cin].
int mkd_parser::finalize() {
    for (const auto& kv : params)
        if (!kv.second.loaded) return mkd_fail(MKD_ERR_MISSING, "mkd_parser_finalize: missing tensor " + kv.first);
    std::vector<char> stage;
    auto bump = [&](size_t bytes) { const size_t o = stage.size(); stage.resize(o + ((bytes + 255) & ~(size_t)255), 0); return o; };
    // kind 0: bf16 GEMM weight; 1: fp32 gate weight; 2: the stem ([tap][C0] bf16)
    auto pack = [&](const std::string& key, const std::string& conv, const std::string& bn, int kind, int pad_rows_to) {
        const Param& W = params[conv + ".weight"];
        const int co = (int)W.shape[0], ci = (int)W.shape[1], k = (int)W.shape[2];
        const int rows = pad_rows_to > co ? pad_rows_to : co;
        std::vector<float> scale(co, 1.0f), bias(co, 0.0f);
        if (!bn.empty()) {
            const float* g = params[bn + ".weight"].data.data(); const float* be = params[bn + ".bias"].data.data();
            const float* mu = params[bn + ".running_mean"].data.data(); const float* var = params[bn + ".running_var"].data.data();
            for (int o = 0; o < co; ++o) { scale[o] = g[o] / sqrtf(var[o] + cfg.bn_eps); bias[o] = be[o] - mu[o] * scale[o]; }
        }
        ConvW& c = packed[key];
        const size_t per = (size_t)ci * k * k;
        c.w_off = bump((size_t)rows * per * (kind == 1 ? 4 : 2));
        for (int o = 0; o < co; ++o)
            for (int i = 0; i < ci; ++i)
                for (int t = 0; t < k * k; ++t) {
                    const float v = W.data[((size_t)o * ci + i) * k * k + t] * scale[o];
                    if (kind == 1) ((float*)(stage.data() + c.w_off))[(size_t)o * per + (size_t)t * ci + i] = v;
                    else if (kind == 0) ((uint16_t*)(stage.data() + c.w_off))[(size_t)o * per + (size_t)t * ci + i] = host_bf16(v);
                    else ((uint16_t*)(stage.data() + c.w_off))[((size_t)t * ci + i) * co + o] = host_bf16(v);
                }
        c.b_off = bump((size_t)rows * 4);
        memcpy(stage.data() + c.b_off, bias.data(), (size_t)co * 4);
    };
    for (const PackItem& it : items) pack(it.key, it.conv, it.bn, it.kind, it.pad_rows_to);
    if (wdev) { hipDeviceSynchronize(); hipFree(wdev); wdev = nullptr; }
    MKD_HIP_CHECK(hipMalloc((void**)&wdev, stage.size()));
    MKD_HIP_CHECK(hipMemcpy(wdev, stage.data(), stage.size(), hipMemcpyHostToDevice));
    if (!zero) {
        MKD_HIP_CHECK(hipMalloc((void**)&zero, 4096));
        MKD_HIP_CHECK(hipMemset(zero, 0, 4096));
    }
    finalized = true;
    return 0;
}

// The launch sequence.  base = the workspace; null: a DRY pass that enqueues nothing, forms no pointer and only adds up what a real
// pass needs (need[0] = the shared split-K workspace, need[1] = the whole workspace, which a real pass is handed back).  *flops = 2 x
// the multiply-accumulates, *launches_out = the kernels of the pass.  Every activation gets its own slice of the workspace (bump
// allocation, 256-byte aligned); the handle itself is not changed.
int mkd_parser::run(const float* images, int batch, int H, int W, char* base, size_t* need, double* flops, int* launches_out, float** logits_out,
                    hipStream_t stream) const {
    const bool dry = base == nullptr;
    size_t off = 0;
    double fl = 0.0;
    int nl = 0;
    auto alloc = [&](size_t n) { char* p = dry ? nullptr : base + off; off += (n + 255) & ~(size_t)255; return p; };
    auto dev = [&](size_t o) -> const char* { return wdev ? wdev + o : nullptr; };          // (a dry pass may come before finalize)
    auto act = [&](size_t pixels, int C) { return (bf16_t*)alloc(pixels * C * sizeof(bf16_t)); };
    size_t ws_need = 0;
    float* splitk_ws = nullptr; size_t splitk_bytes = 0;
    auto wgt = [&](const std::string& k) -> const ConvW& { return packed.at(k); };
    // one GEMM: conv3x3 (k == 3; input [B,Hin,Win,Cin] at pixel stride lda, nearest-upsampled by 2^up, stride s) or linear (k == 1)
    auto gemm = [&](const std::string& key, const bf16_t* A, int lda, int Hin, int Win, int stride, int up, const bf16_t* R, int ldr, int actc,
                    void* Cout, int ldc, int out_f32) -> int {
        const ConvW& c = wgt(key);
        GemmArgs a; memset(&a, 0, sizeof(a));
        const int Ho = c.k == 3 ? (Hin << up) / stride : Hin, Wo = c.k == 3 ? (Win << up) / stride : Win;
        a.A = A; a.lda = lda; a.W = (const bf16_t*)dev(c.w_off); a.ldw = c.cin * c.k * c.k;
        a.bias = c.has_bias ? (const float*)dev(c.b_off) : nullptr;
        a.rows_per_batch = 1; a.R = R; a.ldr = ldr; a.scale = 1.0f; a.act = actc; a.C = Cout; a.ldc = ldc; a.out_f32 = out_f32;
        a.M = batch * Ho * Wo; a.N = c.cout; a.K = c.cin * c.k * c.k;
        if (c.k == 3) { a.conv = 1; a.Hin = Hin; a.Win = Win; a.Cin = c.cin; a.Hout = Ho; a.Wout = Wo; a.stride = stride; a.up = up; a.pad_tl = 1; }
        a.zero = zero;
        int cfg_i = 0, s = 1;
        const int rc = gemm_resolve(a, &cfg_i, &s);
        if (rc) return rc;
        fl += 2.0 * a.M * a.N * a.K;
        nl += s > 1 ? 2 : 1;
        ws_need = std::max(ws_need, gemm_ws_bytes(a.M, a.N, s));          // nothing for a GEMM that does not split
        if (dry) return 0;
        a.ws = splitk_ws; a.ws_bytes = splitk_bytes;
        return launch_gemm(a, stream);
    };
#define PARSER_DO(expr) do { const int _rc = (expr); if (_rc) return _rc; } while (0)
#define PARSER_K(expr) do { ++nl; if (!dry) { const int _rc = (expr); if (_rc) return _rc; } } while (0)
    const int* w = cfg.widths;
    const int cp = cfg.cp_channels, ff = cfg.ffm_channels, catC = w[1] + cp;
    const int h8 = H / 8, w8 = W / 8, h16 = H / 16, w16 = W / 16, h32 = H / 32, w32 = W / 32;
    if (!dry) { splitk_ws = (float*)alloc(need[0]); splitk_bytes = need[0]; }
    // stem
    bf16_t* s0 = act((size_t)batch * (H / 2) * (W / 2), w[0]);
    bf16_t* x0 = act((size_t)batch * (H / 4) * (W / 4), w[0]);
    {
        const ConvW& c = wgt("stem");
        PARSER_K(launch_parser_stem_conv(images, (const bf16_t*)dev(c.w_off), (const float*)dev(c.b_off), s0, batch, H, W, w[0], cfg.mean, cfg.std, stream));
        fl += 2.0 * batch * (H / 2) * (W / 2) * w[0] * 147;
        PARSER_K(launch_parser_maxpool(s0, x0, batch, H / 2, W / 2, w[0], stream));
    }
    bf16_t* cat = act((size_t)batch * h8 * w8, catC);       // [feat8 | feat_cp8]
    const bf16_t* cur = x0; int curC = w[0], curLd = w[0], h = H / 4, wd = W / 4;
    const bf16_t* feat16 = nullptr; const bf16_t* feat32 = nullptr;
    for (int L = 0; L < 4; ++L) {
        for (int i = 0; i < cfg.blocks[L]; ++i) {
            const std::string P = "cp.resnet.layer" + std::to_string(L + 1) + "." + std::to_string(i);
            const int stride = (i == 0 && L > 0) ? 2 : 1, co = w[L];
            const int ho = h / stride, wo = wd / stride;
            const size_t px = (size_t)batch * ho * wo;
            bf16_t* t = act(px, co);
            PARSER_DO(gemm(P + ".conv1", cur, curLd, h, wd, stride, 0, nullptr, 0, 4, t, co, 0));
            const bf16_t* R = cur; int ldr = curLd;
            if (packed.count(P + ".down")) {
                const bf16_t* A = cur; int lda = curLd;
                if (stride == 2) {
                    bf16_t* g = act(px, curC);
                    PARSER_K(launch_parser_subsample(cur, curLd, g, batch, h, wd, curC, stream));
                    A = g; lda = curC;
                }
                bf16_t* sc = act(px, co);
                PARSER_DO(gemm(P + ".down", A, lda, ho, wo, 1, 0, nullptr, 0, 0, sc, co, 0));
                R = sc; ldr = co;
            }
            const bool to_cat = L == 1 && i == cfg.blocks[L] - 1;
            bf16_t* out = to_cat ? cat : act(px, co);
            const int ldo = to_cat ? catC : co;
            PARSER_DO(gemm(P + ".conv2", t, co, ho, wo, 1, 0, R, ldr, 4, out, ldo, 0));
            cur = out; curC = co; curLd = ldo; h = ho; wd = wo;
        }
        if (L == 2) feat16 = cur;
        if (L == 3) feat32 = cur;
    }
    // context path
    auto gate1 = [&](const std::string& key, const bf16_t* x, int ldx, int pixels, int C, int actc, float* out) -> int {
        const ConvW& c = wgt(key);
        return launch_parser_gate(x, ldx, batch, pixels, C, (const float*)dev(c.w_off), (const float*)dev(c.b_off), c.cout, actc, nullptr, nullptr,
                                  0, 0, out, stream);
    };
    float* avg = (float*)alloc((size_t)batch * cp * 4);
    PARSER_K(gate1("cp.conv_avg", feat32, w[3], h32 * w32, w[3], 1, avg));
    bf16_t* f32t = act((size_t)batch * h32 * w32, cp);
    PARSER_DO(gemm("cp.arm32.conv", feat32, w[3], h32, w32, 1, 0, nullptr, 0, 4, f32t, cp, 0));
    float* a32 = (float*)alloc((size_t)batch * cp * 4);
    PARSER_K(gate1("cp.arm32.atten", f32t, cp, h32 * w32, cp, 2, a32));
    bf16_t* s32 = act((size_t)batch * h32 * w32, cp);
    PARSER_K(launch_parser_gate_apply(f32t, cp, a32, 0, avg, nullptr, 0, s32, cp, batch, h32, w32, cp, 0, stream));
    bf16_t* cp16 = act((size_t)batch * h16 * w16, cp);
    PARSER_DO(gemm("cp.conv_head32", s32, cp, h32, w32, 1, 1, nullptr, 0, 4, cp16, cp, 0));            // nearest x2 inside the conv's gather
    bf16_t* f16t = act((size_t)batch * h16 * w16, cp);
    PARSER_DO(gemm("cp.arm16.conv", feat16, w[2], h16, w16, 1, 0, nullptr, 0, 4, f16t, cp, 0));
    float* a16 = (float*)alloc((size_t)batch * cp * 4);
    PARSER_K(gate1("cp.arm16.atten", f16t, cp, h16 * w16, cp, 2, a16));
    bf16_t* s16 = act((size_t)batch * h16 * w16, cp);
    PARSER_K(launch_parser_gate_apply(f16t, cp, a16, 1, nullptr, cp16, cp, s16, cp, batch, h16, w16, cp, 0, stream));
    PARSER_DO(gemm("cp.conv_head16", s16, cp, h16, w16, 1, 1, nullptr, 0, 4, dry ? nullptr : cat + w[1], catC, 0));    // feat_cp8 beside feat8
    // feature fusion
    bf16_t* f = act((size_t)batch * h8 * w8, ff);
    PARSER_DO(gemm("ffm.convblk", cat, catC, h8, w8, 1, 0, nullptr, 0, 4, f, ff, 0));
    float* af = (float*)alloc((size_t)batch * ff * 4);
    {
        const ConvW& c1 = wgt("ffm.conv1"); const ConvW& c2 = wgt("ffm.conv2");
        PARSER_K(launch_parser_gate(f, ff, batch, h8 * w8, ff, (const float*)dev(c1.w_off), nullptr, c1.cout, 1, (const float*)dev(c2.w_off), nullptr,
                                    c2.cout, 2, af, stream));
    }
    bf16_t* fo = act((size_t)batch * h8 * w8, ff);
    PARSER_K(launch_parser_gate_apply(f, ff, af, 2, nullptr, nullptr, 0, fo, ff, batch, h8, w8, ff, 0, stream));
    // output head
    bf16_t* co = act((size_t)batch * h8 * w8, ff);
    PARSER_DO(gemm("conv_out.conv", fo, ff, h8, w8, 1, 0, nullptr, 0, 4, co, ff, 0));
    float* logits = (float*)alloc((size_t)batch * h8 * w8 * ncp() * 4);
    PARSER_DO(gemm("conv_out.conv_out", co, ff, h8, w8, 1, 0, nullptr, 0, 0, logits, ncp(), 1));
#undef PARSER_DO
#undef PARSER_K
    if (dry) { need[0] = ws_need; need[1] = off + ((ws_need + 255) & ~(size_t)255); }
    if (logits_out) *logits_out = logits;
    if (flops) *flops = fl;
    if (launches_out) *launches_out = nl;
    return 0;
}

int mkd_parser::forward(const float* images, int batch, int H, int W, float** logits_out, hipStream_t stream) {
    size_t need[2] = {0, 0};
    int rc = run(nullptr, batch, H, W, nullptr, need, nullptr, nullptr, nullptr, stream);
    if (rc) return rc;
    if (need[1] > ws_cap) {              // a new (batch, H, W): the handle's own workspace grows, as mkd_prepare's does
        if (ws) { hipDeviceSynchronize(); hipFree(ws); ws = nullptr; ws_cap = 0; }
        MKD_HIP_CHECK(hipMalloc((void**)&ws, need[1]));
        ws_cap = need[1];
    }
    return run(images, batch, H, W, ws, need, nullptr, &launches, logits_out, stream);
}

static int parser_check_cfg(const mkd_parser_config* c) {
    if (!c) return mkd_fail(MKD_ERR_ARG, "mkd_parser_create: null config");
    if (c->n_classes < 2 || c->n_classes > 32) return mkd_fail(MKD_ERR_ARG, "mkd_parser_create: n_classes must be 2..32");
    for (int i = 0; i < 4; ++i) {
        if (c->widths[i] < 8 || c->widths[i] % 8 || c->widths[i] > PARSER_GATE_MAX) return mkd_fail(MKD_ERR_ARG, "mkd_parser_create: every width must be a multiple of 8 in 8..2048");
        if (c->blocks[i] < 1 || c->blocks[i] > 64) return mkd_fail(MKD_ERR_ARG, "mkd_parser_create: blocks per layer must be 1..64");
    }
    if (c->widths[0] > PARSER_STEM_MAX) return mkd_fail(MKD_ERR_ARG, "mkd_parser_create: the stem width is at most 128 (its weights live in LDS)");
    if (c->cp_channels < 8 || c->cp_channels % 8 || c->cp_channels > PARSER_GATE_MAX) return mkd_fail(MKD_ERR_ARG, "mkd_parser_create: cp_channels must be a multiple of 8 in 8..2048");
    if (c->ffm_channels < 8 || c->ffm_channels % 8 || c->ffm_channels > PARSER_GATE_MAX) return mkd_fail(MKD_ERR_ARG, "mkd_parser_create: ffm_channels must be a multiple of 8 in 8..2048");
    if (!(c->bn_eps > 0.f)) return mkd_fail(MKD_ERR_ARG, "mkd_parser_create: bn_eps must be positive");
    for (int i = 0; i < 3; ++i)
        if (!(c->std[i] > 0.f) || !std::isfinite(c->mean[i])) return mkd_fail(MKD_ERR_ARG, "mkd_parser_create: std must be positive, mean finite");
    return 0;
}

static int parser_check_call(const char* what, const mkd_parser* p, const float* images, int batch, int H, int W) {
    if (!p || !images) return mkd_fail(MKD_ERR_ARG, std::string(what) + ": null pointer");
    if (batch < 1 || batch > 64) return mkd_fail(MKD_ERR_ARG, std::string(what) + ": batch must be 1..64");
    if (H < 64 || H > 1024 || H % 32 || W < 64 || W > 1024 || W % 32) return mkd_fail(MKD_ERR_ARG, std::string(what) + ": H and W must be multiples of 32 in 64..1024");
    return 0;
}

static int head_check(const float* logits, int batch, int n_classes, int h8, int w8, int P_h, int P_w, int out_h, int out_w, const uint8_t* labels) {
    if (!logits || !labels) return mkd_fail(MKD_ERR_ARG, "mkd_parse_labels: null pointer");
    if (batch < 1 || batch > 65535) return mkd_fail(MKD_ERR_ARG, "mkd_parse_labels: batch must be 1..65535");
    if (n_classes < 2 || n_classes > 32) return mkd_fail(MKD_ERR_ARG, "mkd_parse_labels: n_classes must be 2..32");
    if (h8 < 1 || w8 < 1 || P_h < 1 || P_w < 1 || h8 > 16384 || w8 > 16384 || P_h > 16384 || P_w > 16384)
        return mkd_fail(MKD_ERR_ARG, "mkd_parse_labels: logit and parse sizes must be 1..16384");
    if (out_h < 1 || out_w < 1 || out_h > 16384 || out_w > 16384) return mkd_fail(MKD_ERR_ARG, "mkd_parse_labels: out_h and out_w must be 1..16384");
    return 0;
}

extern "C" {

int mkd_parser_create(const mkd_parser_config* cfg, mkd_parser** out) {
    if (!out) return mkd_fail(MKD_ERR_ARG, "mkd_parser_create: null out");
    *out = nullptr;
    const int rc = parser_check_cfg(cfg);
    if (rc) return rc;
    mkd_parser* p = new mkd_parser();
    p->cfg = *cfg;
    p->build_table();
    *out = p;
    return 0;
}
void mkd_parser_destroy(mkd_parser* p) { delete p; }
int mkd_parser_param_total(const mkd_parser* p) { return p ? (int)p->params.size() : 0; }
const char* mkd_parser_param_name(const mkd_parser* p, int i) {
    if (!p || i < 0 || i >= (int)p->params.size()) return nullptr;
    auto it = p->params.begin(); std::advance(it, i);
    return it->first.c_str();
}
int mkd_parser_param_shape(const mkd_parser* p, int i, int64_t* shape4) {
    if (!p || !shape4 || i < 0 || i >= (int)p->params.size()) return -1;
    auto it = p->params.begin(); std::advance(it, i);
    for (size_t k = 0; k < it->second.shape.size(); ++k) shape4[k] = it->second.shape[k];
    return (int)it->second.shape.size();
}
int64_t mkd_parser_param_count(const mkd_parser* p) {
    int64_t n = 0;
    if (p) for (const auto& kv : p->params) { int64_t e = 1; for (int64_t d : kv.second.shape) e *= d; n += e; }
    return n;
}
int mkd_parser_load_weight(mkd_parser* p, const char* name, const float* data, int ndim, const int64_t* shape) {
    if (!p || !name || !data || (ndim > 0 && !shape) || ndim < 0) return mkd_fail(MKD_ERR_ARG, "mkd_parser_load_weight: null pointer");
    const std::string n(name);
    if (ignorable(n)) return 0;
    auto it = p->params.find(n);
    if (it == p->params.end()) return mkd_fail(MKD_ERR_ARG, "mkd_parser_load_weight: unknown tensor " + n);
    Param& q = it->second;
    bool ok = ndim == (int)q.shape.size();
    int64_t e = 1;
    for (int k = 0; ok && k < ndim; ++k) { ok = shape[k] == q.shape[k]; e *= q.shape[k]; }
    if (!ok) return mkd_fail(MKD_ERR_ARG, "mkd_parser_load_weight: wrong shape for " + n);
    q.data.assign(data, data + e);
    q.loaded = true;
    p->finalized = false;
    return 0;
}
int mkd_parser_finalize(mkd_parser* p) {
    if (!p) return mkd_fail(MKD_ERR_ARG, "mkd_parser_finalize: null handle");
    return p->finalize();
}
int mkd_parser_logits(mkd_parser* p, const float* images01, int batch, int H, int W, float* logits_nchw, void* stream) {
    const int rc = parser_check_call("mkd_parser_logits", p, images01, batch, H, W);
    if (rc) return rc;
    if (!logits_nchw) return mkd_fail(MKD_ERR_ARG, "mkd_parser_logits: null pointer");
    if (!p->finalized) return mkd_fail(MKD_ERR_STATE, "mkd_parser_logits: weights are not finalized");
    float* lg = nullptr;
    const int r2 = p->forward(images01, batch, H, W, &lg, (hipStream_t)stream);
    if (r2) return r2;
    ++p->launches;
    return launch_parser_logits_nchw(lg, p->ncp(), logits_nchw, batch, (H / 8) * (W / 8), p->cfg.n_classes, (hipStream_t)stream);
}
int mkd_parser_parse(mkd_parser* p, const float* images01, int batch, int H, int W, int out_h, int out_w, const uint8_t* lut, uint8_t* labels,
                     float* logits_nchw, void* stream) {
    const int rc = parser_check_call("mkd_parser_parse", p, images01, batch, H, W);
    if (rc) return rc;
    if (!labels) return mkd_fail(MKD_ERR_ARG, "mkd_parser_parse: null pointer");
    if (out_h < 1 || out_w < 1 || out_h > 16384 || out_w > 16384) return mkd_fail(MKD_ERR_ARG, "mkd_parser_parse: out_h and out_w must be 1..16384");
    if (!p->finalized) return mkd_fail(MKD_ERR_STATE, "mkd_parser_parse: weights are not finalized");
    float* lg = nullptr;
    const int r2 = p->forward(images01, batch, H, W, &lg, (hipStream_t)stream);
    if (r2) return r2;
    const int h8 = H / 8, w8 = W / 8, nc = p->ncp();
    if (logits_nchw) {
        ++p->launches;
        const int r3 = launch_parser_logits_nchw(lg, nc, logits_nchw, batch, h8 * w8, p->cfg.n_classes, (hipStream_t)stream);
        if (r3) return r3;
    }
    ++p->launches;
    return launch_parser_head(lg, 1, (int64_t)w8 * nc, nc, (int64_t)h8 * w8 * nc, batch, p->cfg.n_classes, h8, w8, H, W, out_h, out_w, lut, labels,
                              (hipStream_t)stream);
}
double mkd_parser_flops(const mkd_parser* p, int H, int W) {
    if (!p || H < 64 || H > 1024 || H % 32 || W < 64 || W > 1024 || W % 32) return 0.0;
    size_t need[2] = {0, 0};
    double fl = 0.0;
    return p->run(nullptr, 1, H, W, nullptr, need, &fl, nullptr, nullptr, nullptr) ? 0.0 : fl;
}
int mkd_parser_launches(const mkd_parser* p) { return p ? p->launches : 0; }

int mkd_parse_labels(const float* logits, int64_t s_class, int64_t s_row, int64_t s_col, int64_t s_batch, int batch, int n_classes, int h8, int w8,
                     int P_h, int P_w, int out_h, int out_w, const uint8_t* lut, uint8_t* labels, void* stream) {
    const int rc = head_check(logits, batch, n_classes, h8, w8, P_h, P_w, out_h, out_w, labels);
    if (rc) return rc;
    return launch_parser_head(logits, s_class, s_row, s_col, s_batch, batch, n_classes, h8, w8, P_h, P_w, out_h, out_w, lut, labels, (hipStream_t)stream);
}

int mkd_parser_stem(const float* images01, const uint16_t* w_packed, const float* bias, const float* mean3, const float* std3, uint16_t* half_res,
                    uint16_t* y, int batch, int H, int W, int C0, void* stream) {
    if (!images01 || !w_packed || !bias || !mean3 || !std3 || !half_res || !y) return mkd_fail(MKD_ERR_ARG, "mkd_parser_stem: null pointer");
    if (batch < 1 || batch > 65535 || H < 32 || W < 32 || H % 32 || W % 32 || H > 16384 || W > 16384) return mkd_fail(MKD_ERR_ARG, "mkd_parser_stem: H and W must be multiples of 32");
    if (C0 < 8 || C0 % 8 || C0 > PARSER_STEM_MAX) return mkd_fail(MKD_ERR_ARG, "mkd_parser_stem: C0 must be a multiple of 8 in 8..128");
    const int rc = launch_parser_stem_conv(images01, w_packed, bias, half_res, batch, H, W, C0, mean3, std3, (hipStream_t)stream);
    if (rc) return rc;
    return launch_parser_maxpool(half_res, y, batch, H / 2, W / 2, C0, (hipStream_t)stream);
}
int mkd_channel_gate(const uint16_t* x, int ldx, int batch, int pixels, int C, const float* w1, const float* b1, int n1, int act1, const float* w2,
                     const float* b2, int n2, int act2, float* out, void* stream) {
    if (!x || !w1 || !out) return mkd_fail(MKD_ERR_ARG, "mkd_channel_gate: null pointer");
    if (batch < 1 || batch > 65535 || pixels < 1 || C < 8 || C % 8 || C > PARSER_GATE_MAX || ldx < C || ldx % 8)
        return mkd_fail(MKD_ERR_ARG, "mkd_channel_gate: C must be a multiple of 8 in 8..2048, ldx a multiple of 8 >= C");
    if (n1 < 1 || n1 > PARSER_GATE_MAX || (w2 && (n2 < 1 || n2 > PARSER_GATE_MAX))) return mkd_fail(MKD_ERR_ARG, "mkd_channel_gate: 1..2048 outputs per mat-vec");
    if (act1 < 0 || act1 > 2 || act2 < 0 || act2 > 2) return mkd_fail(MKD_ERR_ARG, "mkd_channel_gate: activation codes are 0 none, 1 ReLU, 2 sigmoid");
    return launch_parser_gate(x, ldx, batch, pixels, C, w1, b1, n1, act1, w2, w2 ? b2 : nullptr, w2 ? n2 : 0, act2, out, (hipStream_t)stream);
}
int mkd_gate_apply_bf16(const uint16_t* x, int ldx, const float* a, int mode, const void* add, int ldadd, uint16_t* y, int ldy, int batch, int h, int w,
                        int C, int u, void* stream) {
    if (!x || !a || !y || (mode != 2 && !add)) return mkd_fail(MKD_ERR_ARG, "mkd_gate_apply_bf16: null pointer");
    if (mode < 0 || mode > 2 || u < 0 || u > 1) return mkd_fail(MKD_ERR_ARG, "mkd_gate_apply_bf16: mode is 0..2, u is 0 or 1");
    if (batch < 1 || h < 1 || w < 1 || h > 16384 || w > 16384 || C < 8 || C % 8 || ldx < C || ldx % 8 || ldy < C || ldy % 8 || (mode == 1 && (ldadd < C || ldadd % 8)))
        return mkd_fail(MKD_ERR_ARG, "mkd_gate_apply_bf16: C and the pixel strides must be multiples of 8, strides >= C");
    return launch_parser_gate_apply(x, ldx, a, mode, mode == 0 ? (const float*)add : nullptr, mode == 1 ? (const bf16_t*)add : nullptr, ldadd, y, ldy, batch,
                                    h, w, C, u, (hipStream_t)stream);
}

}  // extern "C"
