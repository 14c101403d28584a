// The GEMM / conv tile configurations: ONE row each, in index order.  Everything that addresses a kernel by number - the tuned table
// (gemm_tuned.inc), the run-time overrides, mkd_gemm_force_tile, the tuners (through mkd_gemm_tile_info) - means a row of this file;
// the metadata table, the is-patch / folds-second-input / plain-epilogue-only predicates, the CFG_<name> constants and both dispatch
// switches (launch_gemm, launch_conv_patch) are generated from it.  A new tile is a new row at the end; a row is never renumbered
// or renamed (profiles/tune/*.json and gemm_tuned.inc hold indices).
//
//   MKD_TILE(index, name, family, TM, TN, WM, WN, STAGES, KW, base)
//
//   name     bare token: "name" for reports, CFG_name as a constant
//   family   GEMM    gemm_kernel (gather / linear), every epilogue variant
//            KSPLIT  gemm_kernel with the in-block K split: KW groups of WM x WN waves; plain epilogue or on-the-fly LayerNorm only
//            LIGHT   gemm_kernel, plain epilogue only (two instantiations instead of eight)
//            PATCH   conv3x3_patch_kernel (kernels_conv.hip): LDS-staged 3x3 conv, geometry limits (conv_patch_supported)
//            RA      gemm_ra_kernel: WM waves split the rows only (WN = 1); plain epilogue only
//   TM x TN  block tile; WM x WN wave grid (m x n); STAGES LDS ring depth
//   base     the configuration a launch falls back to when it needs more than this row's epilogue (itself for GEMM / PATCH rows)
//
//                                                                          LDS      blocks/CU  FLOP per staged byte
MKD_TILE( 0, 256x128,          GEMM,   256, 128, 4, 2, 3, 1,  0)      // 144 KiB  1          85
MKD_TILE( 1, 128x128_s3,       GEMM,   128, 128, 2, 2, 3, 1,  1)      //  96 KiB  1          64
MKD_TILE( 2, 128x128_s2,       GEMM,   128, 128, 2, 2, 2, 1,  2)      //  64 KiB  2          64
MKD_TILE( 3, 128x64,           GEMM,   128,  64, 2, 2, 3, 1,  3)      //  72 KiB  2          43
MKD_TILE( 4, 64x128,           GEMM,    64, 128, 2, 2, 3, 1,  4)      //  72 KiB  2          43
MKD_TILE( 5, 64x64,            GEMM,    64,  64, 2, 2, 4, 1,  5)      //  64 KiB  2          32
// LDS-staged 3x3 conv tiles: 8 waves on the 256-pixel tiles, 4 on the others
MKD_TILE( 6, patch256x128,     PATCH,  256, 128, 4, 2, 3, 1,  6)
MKD_TILE( 7, patch256x64,      PATCH,  256,  64, 4, 2, 3, 1,  7)
MKD_TILE( 8, patch128x128,     PATCH,  128, 128, 2, 2, 3, 1,  8)
MKD_TILE( 9, patch128x64,      PATCH,  128,  64, 2, 2, 3, 1,  9)
MKD_TILE(10, patch64x128,      PATCH,   64, 128, 2, 2, 3, 1, 10)
MKD_TILE(11, patch64x64,       PATCH,   64,  64, 2, 2, 3, 1, 11)
// short-K layers, (nearly) every K-step in flight at once
MKD_TILE(12, 64x64_s6,         GEMM,    64,  64, 2, 2, 6, 1, 12)      //  96 KiB
MKD_TILE(13, 64x128_s5,        GEMM,    64, 128, 2, 2, 5, 1, 13)      // 120 KiB
// every channel count of the nets is a multiple of 320, so 160-wide column tiles never run a partly empty tile (N = 320 -> 2 x 160
// instead of 3 x 128 with 17 % of the MFMA work wasted)
MKD_TILE(14, 64x160,           GEMM,    64, 160, 2, 2, 3, 1, 14)      //  86 KiB
MKD_TILE(15, 128x160,          GEMM,   128, 160, 2, 2, 3, 1, 15)      // 110 KiB
MKD_TILE(16, 64x160_s2,        GEMM,    64, 160, 2, 2, 2, 1, 16)      //  57 KiB  2
// one CU streams at most ~55 GB/s (tools/micro/stream_rate.hip), so a GEMM with fewer blocks than CUs finishes sooner when each
// block pulls FEWER operand bytes ((TM + TN) * K * 2), not more
MKD_TILE(17, 32x64,            GEMM,    32,  64, 2, 2, 4, 1, 17)
MKD_TILE(18, 64x32,            GEMM,    64,  32, 2, 2, 4, 1, 18)
MKD_TILE(19, 32x32,            GEMM,    32,  32, 2, 2, 4, 1, 19)
// in-block K split (KW groups of 4 waves, see gemm_kernel)
MKD_TILE(20, 32x32_k2,         KSPLIT,  32,  32, 2, 2, 4, 2, 19)
MKD_TILE(21, 32x32_k4,         KSPLIT,  32,  32, 2, 2, 4, 4, 19)
MKD_TILE(22, 64x32_k2,         KSPLIT,  64,  32, 2, 2, 4, 2, 18)
MKD_TILE(23, 64x32_k4,         KSPLIT,  64,  32, 2, 2, 3, 4, 18)
MKD_TILE(24, 64x64_k2,         KSPLIT,  64,  64, 2, 2, 4, 2,  5)
MKD_TILE(25, 64x64_k4,         KSPLIT,  64,  64, 2, 2, 2, 4,  5)
MKD_TILE(26, 32x64_k2,         KSPLIT,  32,  64, 2, 2, 4, 2, 17)
MKD_TILE(27, 32x64_k4,         KSPLIT,  32,  64, 2, 2, 3, 4, 17)
MKD_TILE(28, 128x64_k2,        KSPLIT, 128,  64, 2, 2, 3, 2,  3)
MKD_TILE(29, 64x128_k2,        KSPLIT,  64, 128, 2, 2, 3, 2,  4)
// more waves per CU pulling operands.  A 4-wave workgroup streams ~48 GB/s whatever its ring depth (2, 4 or 8 stages), a CU with 8
// waves ~94 GB/s, with 16 waves ~122 GB/s (tools/micro/stream_rate2.hip): the limit is per WAVE.  So: the same tiles with 2-stage
// rings (half the LDS -> twice the resident workgroups) ...
MKD_TILE(30, 64x64_s2,         LIGHT,   64,  64, 2, 2, 2, 1,  5)
MKD_TILE(31, 128x64_s2,        LIGHT,  128,  64, 2, 2, 2, 1,  3)
MKD_TILE(32, 64x128_s2,        LIGHT,   64, 128, 2, 2, 2, 1,  4)
MKD_TILE(33, 64x32_s2,         LIGHT,   64,  32, 2, 2, 2, 1, 18)
// ... and 8-wave workgroups.  Plain epilogue only (anything else runs on the base configuration).
MKD_TILE(34, 128x128_w8,       LIGHT,  128, 128, 4, 2, 2, 1,  2)
MKD_TILE(35, 128x64_w8,        LIGHT,  128,  64, 4, 2, 3, 1,  3)
MKD_TILE(36, 64x128_w8,        LIGHT,   64, 128, 2, 4, 3, 1,  4)
MKD_TILE(37, 64x64_w8,         LIGHT,   64,  64, 2, 4, 4, 1,  5)
// LDS-staged 3x3 conv tiles with EIGHT waves (32x32 / 32x32 / 32x64 per wave): a wave's LDS-DMA transfers complete one after the
// other (~1 KiB per 200-300 cycles, tools/micro/stream_rate3.hip), and with four waves each tap asks 2.7 pieces of every wave for
// 16 MFMAs - the tap waits for the transfers, not for the matrix cores; eight waves halve the pieces per wave.  Inside the sampling
// loop the whole-loop tuner (tools/tune_wall.py) moves the heavy shapes onto the eight-wave tiles although they are not faster alone
// (DESIGN.md 4.4): half the LDS-DMA pieces per wave and K-step.
MKD_TILE(38, patch128x64_w8,   PATCH,  128,  64, 4, 2, 3, 1, 38)
MKD_TILE(39, patch64x128_w8,   PATCH,   64, 128, 2, 4, 3, 1, 39)
MKD_TILE(40, patch128x128_w8,  PATCH,  128, 128, 4, 2, 3, 1, 40)
MKD_TILE(41, 256x64_w8,        LIGHT,  256,  64, 4, 2, 3, 1,  3)      // gather / linear, plain epilogue only
// LDS-staged with SIXTEEN waves (32x64 / 32x32 per wave)
MKD_TILE(42, patch256x128_w16, PATCH,  256, 128, 8, 2, 3, 1, 42)
MKD_TILE(43, patch128x128_w16, PATCH,  128, 128, 4, 4, 3, 1, 43)
// register-A tiles (gemm_ra_kernel: activations straight into the MFMA's registers, only the weight tile through LDS): 8 waves of
// 32 rows each, 4 waves of 32 rows (128-row tiles) or 64 rows (ra256x64)
MKD_TILE(44, ra256x64_w8,      RA,     256,  64, 8, 1, 4, 1,  3)
MKD_TILE(45, ra256x128_w8,     RA,     256, 128, 8, 1, 3, 1,  1)
MKD_TILE(46, ra128x128,        RA,     128, 128, 4, 1, 3, 1,  1)
MKD_TILE(47, ra128x64,         RA,     128,  64, 4, 1, 4, 1,  3)
MKD_TILE(48, ra128x160,        RA,     128, 160, 4, 1, 3, 1, 14)
MKD_TILE(49, ra256x64,         RA,     256,  64, 4, 1, 3, 1,  3)
// SIXTEEN waves (64x64 each), 128 KiB LDS: 128 FLOP per byte pulled out of L2, for the few GEMMs whose M and N both allow it (the K
// loops of the gather / linear kernel run at three quarters of the L2 -> CU rate: DESIGN.md 4.5); plain epilogue only
MKD_TILE(50, 256x256_w16,      LIGHT,  256, 256, 4, 4, 2, 1,  0)
