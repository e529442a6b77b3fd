// Every implicit-GEMM kernel form that is compiled into the library, one X-macro row per form; the first argument of a row is the form's
// base id (CfgInfo::base in igemm.hip), the others are the kernel's template arguments.  The instantiation units, the launcher
// ladi_igemm_launch_base_<id>(IGemmArgs, int batch, hipStream_t) of each form, the dispatch switch, the symbol names and the per-base trait
// record (family, tile geometry) of igemm.hip are all generated from these rows.
//
// Ring-staged kernel: X(base id, WQ, WP, TQ, TP, BK, NST, OCC, ILV), see igemm_kernel.h for the meaning of the parameters.  Grouped by
// translation unit (igemm_inst_<group>.hip) so the build parallelises.
#pragma once

// ---- two workgroups (of 4 waves) or more per CU: the round-1/2 shapes
#define LADI_IGEMM_TILES_A(X) \
    X(1, 2, 2, 2, 4, 32, 3, 2, 0)  /* 128x256 */ \
    X(3, 2, 2, 2, 2, 32, 3, 2, 0)  /* 128x128 */ \
    X(4, 2, 2, 2, 1, 32, 3, 2, 0)  /* 128x64  */ \
    X(5, 2, 2, 1, 1, 32, 3, 2, 0)  /* 64x64   */
#define LADI_IGEMM_TILES_B(X) \
    X(2, 2, 2, 5, 2, 32, 2, 2, 0)  /* 320x128 (Cout = 320 layers, no padding waste) */ \
    X(6, 2, 2, 4, 2, 32, 3, 2, 0)  /* 256x128 */ \
    X(16, 2, 2, 1, 1, 32, 4, 2, 0) /* 64x64, deeper prefetch for shallow-K, latency-bound GEMMs */
#define LADI_IGEMM_TILES_C(X) \
    X(7, 2, 2, 2, 2, 64, 2, 2, 0)  /* 128x128 BK64 */ \
    X(8, 2, 2, 2, 4, 64, 2, 2, 0)  /* 128x256 BK64 */ \
    X(9, 2, 2, 2, 1, 64, 3, 2, 0)  /* 128x64  BK64 */
#define LADI_IGEMM_TILES_D(X) \
    X(10, 2, 2, 5, 2, 64, 2, 2, 0) /* 320x128 BK64 */ \
    X(17, 2, 2, 2, 1, 32, 4, 2, 0) \
    X(18, 2, 2, 2, 2, 32, 4, 2, 0)
#define LADI_IGEMM_TILES_E(X) \
    X(19, 2, 4, 2, 2, 32, 3, 2, 0) /* 128x256, 8 waves */ \
    X(20, 4, 2, 2, 2, 32, 3, 2, 0) /* 256x128, 8 waves */ \
    X(21, 2, 4, 4, 2, 32, 3, 2, 0) /* 256x256, 8 waves, 96 KB LDS */
#define LADI_IGEMM_TILES_F(X) \
    X(22, 2, 4, 5, 2, 64, 2, 2, 0) /* 320x256, 8 waves, 144 KB LDS */ \
    X(47, 2, 2, 2, 2, 64, 2, 2, 1) /* 128x128 BK64, DMA issue interleaved with the MFMA groups */ \
    X(48, 2, 2, 2, 1, 64, 3, 2, 1) /* 128x64  BK64, interleaved */
// ---- round 3: ONE workgroup of 4 waves per CU, one wave per SIMD with up to 240 accumulator registers: tiles whose grid fills the chip
//      at batch 8 (320x192: 256 tiles on the 49 152-pixel level) and deep rings (64-128 KB in flight per CU)
#define LADI_IGEMM_TILES_G(X) \
    X(39, 2, 2, 5, 3, 64, 2, 1, 1) /* 320x192, 128 KB ring, interleaved */ \
    X(40, 2, 2, 5, 3, 32, 4, 1, 1) /* 320x192, BK32 4-deep ring (128 KB): every stage is issued 3 K steps before it is awaited */
#define LADI_IGEMM_TILES_H(X) \
    X(41, 2, 2, 4, 4, 64, 2, 1, 1) /* 256x256, 128 KB ring */ \
    X(42, 2, 2, 2, 2, 64, 4, 1, 1) /* 128x128, 4-deep ring (128 KB) */
#define LADI_IGEMM_TILES_I(X) \
    X(43, 2, 2, 2, 4, 64, 3, 1, 1) /* 128x256, 3-deep ring (144 KB) */ \
    X(44, 2, 2, 2, 1, 64, 5, 1, 1) /* 128x64, 5-deep ring (120 KB) */ \
    X(45, 2, 2, 4, 3, 64, 2, 1, 1) /* 256x192, 112 KB ring */

#define LADI_IGEMM_TILES_ALL(X) \
    LADI_IGEMM_TILES_A(X) LADI_IGEMM_TILES_B(X) LADI_IGEMM_TILES_C(X) LADI_IGEMM_TILES_D(X) LADI_IGEMM_TILES_E(X) LADI_IGEMM_TILES_F(X) \
    LADI_IGEMM_TILES_G(X) LADI_IGEMM_TILES_H(X) LADI_IGEMM_TILES_I(X)

// ---- igemm8_kernel (igemm8.hip), the phase-staggered 8-wave pipeline: X(base id, TQ, TP), workgroup tile (64 TQ) x (128 TP), BK = 64
#define LADI_IGEMM8_TILES(X) \
    X(32, 5, 2) /* 320x256 (Cout = 320 / 640 / 960 / 1280 layers without padding waste) */ \
    X(33, 4, 2) /* 256x256 */ \
    X(54, 2, 2) /* 128x256 */ \
    X(55, 4, 1) /* 256x128 */ \
    X(56, 2, 1) /* 128x128 (64 KB of LDS: two workgroups = 16 waves per CU) */ \
    X(57, 5, 1) /* 320x128 */ \
    X(58, 3, 2) /* 192x256 */

// ---- igemm_lc_kernel (igemm_lc.hip), loader / consumer: X(base id, WQ, WP, TQ, TP, NL, NST): WQ x WP consumer waves of (32 TQ) x (32 TP),
//      NL loader waves, NST-deep ring, BK = 64
#define LADI_IGEMM_LC_TILES(X) \
    X(62, 2, 2, 2, 2, 2, 4) /* 128x128, 128 KB ring */ \
    X(63, 2, 2, 2, 2, 2, 5) /* 128x128, 160 KB ring */ \
    X(64, 2, 2, 4, 2, 2, 3) /* 256x128, 144 KB ring */ \
    X(65, 2, 2, 2, 4, 2, 3) /* 128x256, 144 KB ring */ \
    X(66, 2, 2, 2, 1, 2, 6) /* 128x64, 144 KB ring */ \
    X(67, 2, 2, 5, 2, 2, 2) /* 320x128, 112 KB ring */ \
    X(68, 2, 2, 3, 3, 2, 3) /* 192x192, 144 KB ring */

// ---- igemm_halo_kernel (igemm_halo_kernel.h), halo-resident 3x3 convolution: X(base id, TQ, TP, NXB, NSTW, WPN, WMAX, ONE, G2D, UPS), workgroup
//      tile (64 TQ) x (32 WPN TP) on 2 x WPN waves, BK = 64.  At most two forms per translation unit (igemm_halo_inst_<group>.hip): one form
//      takes ~30 s of hipcc
#define LADI_HALO_TILES_A(X) \
    X(74, 2, 2, 2, 3, 4, 48, 0, 0, 0)  /* 128x256, double halo buffer, 3 weight slots (144 KB) */ \
    X(78, 4, 1, 1, 3, 4, 48, 0, 0, 0)  /* 256x128, single halo buffer, 3 weight slots (128 KB) */
#define LADI_HALO_TILES_B(X) \
    X(75, 4, 2, 1, 3, 4, 48, 0, 0, 0)  /* 256x256, single halo buffer, 3 weight slots (144 KB) */ \
    X(84, 2, 2, 1, 2, 2, 48, 0, 0, 0)  /* 128x128, 4 waves, TWO workgroups per CU (64-72 KB each): one multiplies while the other waits */
#define LADI_HALO_TILES_C(X) \
    X(76, 5, 2, 1, 2, 4, 48, 0, 0, 0)  /* 320x256, single halo buffer, 2 weight slots (128 KB) */ \
    X(88, 2, 2, 1, 3, 2, 24, 0, 0, 0)  /* 128x128, 4 waves x 2 per CU, rows <= 24 pixels: 3 weight slots (72 KB) */
#define LADI_HALO_TILES_D(X) \
    X(77, 2, 1, 2, 4, 4, 48, 0, 0, 0)  /* 128x128, double halo buffer, 4 weight slots (128 KB) */ \
    X(85, 2, 3, 1, 2, 2, 48, 0, 0, 0)  /* 128x192, 4 waves x 2 per CU */
#define LADI_HALO_TILES_E(X) \
    X(89, 2, 3, 1, 3, 2, 24, 0, 0, 0)  /* 128x192, 4 waves x 2 per CU, rows <= 24 pixels */ \
    X(97, 2, 4, 1, 2, 2, 24, 0, 0, 0)  /* 128x256, 4 waves of 64 x 128 x 2 per CU, rows <= 24 pixels (72 KB) */
#define LADI_HALO_TILES_F(X) \
    X(92, 5, 1, 1, 2, 6, 48, 0, 0, 0)  /* 320x192, 12 waves (3 per SIMD), 144 KB */ \
    X(100, 2, 2, 1, 3, 4, 48, 0, 1, 0) /* 2-D blocked 128x256 (8 rows x 32), 8 waves, 96 KB */
#define LADI_HALO_TILES_G(X) \
    X(96, 5, 3, 1, 2, 2, 48, 1, 0, 0)  /* 320x192, 4 waves, ONE per SIMD (240 accumulators), 120 KB */ \
    X(103, 2, 2, 1, 2, 2, 48, 0, 1, 0) /* 2-D blocked 128x128 (4 rows x 32), 4 waves x 2 per CU, 60 KB */
#define LADI_HALO_TILES_H(X) \
    X(101, 4, 2, 1, 3, 4, 48, 0, 1, 0) /* 2-D blocked 256x256, 8 waves, 144 KB */ \
    X(102, 5, 2, 1, 2, 4, 48, 0, 1, 0) /* 2-D blocked 320x256, 8 waves, 128 KB */
#define LADI_HALO_TILES_I(X) \
    X(104, 2, 3, 1, 2, 2, 48, 0, 0, 1) /* folded upsample 128x192, 4 waves x 2 per CU */ \
    X(106, 2, 2, 1, 2, 2, 48, 0, 0, 1) /* folded upsample 128x128, 4 waves x 2 per CU */
#define LADI_HALO_TILES_J(X) \
    X(105, 5, 1, 1, 2, 6, 48, 0, 0, 1) /* folded upsample 320x192, 12 waves */

#define LADI_HALO_TILES_ALL(X) \
    LADI_HALO_TILES_A(X) LADI_HALO_TILES_B(X) LADI_HALO_TILES_C(X) LADI_HALO_TILES_D(X) LADI_HALO_TILES_E(X) LADI_HALO_TILES_F(X) \
    LADI_HALO_TILES_G(X) LADI_HALO_TILES_H(X) LADI_HALO_TILES_I(X) LADI_HALO_TILES_J(X)

// ---- linear_xs_kernel (linear_xs.hip), X-stationary 1x1 layers: X(base id, NST = weight-ring depth).  Its other template arguments depend on the
//      launch (K, epilogue mode, fused norm) and its pixel blocks per wave / channel slices on the configuration, so it has no generated launcher
#define LADI_LINEAR_XS_FORMS(X) \
    X(23, 3) /* two workgroups per CU */ \
    X(93, 2) /* two-slot ring: three workgroups per CU (K = 320) */

// every base id that has a generated launcher, as LADI_PER_BASE(id) (defined by the user before the expansion)
#define LADI_IGEMM_BASE_OF(base, ...) LADI_PER_BASE(base)
#define LADI_IGEMM_LAUNCHER_BASES \
    LADI_IGEMM_TILES_ALL(LADI_IGEMM_BASE_OF) LADI_IGEMM8_TILES(LADI_IGEMM_BASE_OF) LADI_IGEMM_LC_TILES(LADI_IGEMM_BASE_OF) \
    LADI_HALO_TILES_ALL(LADI_IGEMM_BASE_OF)
