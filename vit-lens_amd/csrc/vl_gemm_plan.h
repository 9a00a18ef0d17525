// The row split of the bf16 NT GEMM under cfg == VL_GEMM_AUTO, stated once: which rows of C[M,N] = A[M,K] W[N,K]^T go to the
// persistent kernels and which kernel takes the rows behind them (DESIGN.md 7.13 holds the table).  Pure integer functions of
// the shape and of G, the persistent grid: vl_gemm.hip's run_gemm, vl_gemm_main_rows and vl_gemm_rest_cfg ask them, and
// tests/native/gemm_plan_host.cpp prints them over a grid.  Host only and free of HIP headers, so a plain C++ program includes it.
#pragma once

// The cfg argument of vl_gemm_bf16 (include/vitlens_hip.h lists what each kernel is; 8 and 10 are VL_GEMM_PERSIST and
// VL_GEMM_PINGPONG there).  Any other value runs GEMM_CFG_T256 ... GEMM_CFG_T128_REG by its low two bits.
enum GemmCfg : int {
  GEMM_CFG_T256 = 0,          // one 256x256 LDS-DMA tile per workgroup
  GEMM_CFG_T128 = 1,          // one 128x128 LDS-DMA tile per workgroup
  GEMM_CFG_T256_REG = 2,      // 0 and 1 with register staging
  GEMM_CFG_T128_REG = 3,
  GEMM_CFG_PERSIST1_OLD = 4,  // historical alias of 5
  GEMM_CFG_PERSIST1 = 5,      // round-1 persistent kernel, any shape
  GEMM_CFG_PERSIST1_N128 = 6, // the same on 256x128 tiles (experiment)
  GEMM_CFG_PARK = 8,          // vl_gemm_park.hip
  GEMM_CFG_TAIL = 9,          // split-K tail kernel, one 32x32 tile per workgroup
  GEMM_CFG_PINGPONG = 10,     // vl_gemm_pp.hip
  GEMM_CFG_T64 = 11,          // one 64x64 LDS-DMA tile per workgroup
  GEMM_CFG_T128X64 = 12,
};

// Fewer 256x256 tiles than 3/4 of the grid: 128x128 tiles.  (Between 3/4 and one full round the persistent kernel's single uneven
// round wins: text tower out_proj / c_proj, 77 x 3 = 231 tiles, 30 / 86 us against 89 us on 128x128 tiles.)
constexpr int GEMM_MAIN_MIN_NUM = 3, GEMM_MAIN_MIN_DEN = 4;
// Rows behind the main part.  More than 512: 128x128 tiles.  Otherwise 64x64 LDS-DMA tiles when at least 192 of them fill most of
// the chip (N >= 3072 at 256 rows: 10-12 us against 15-20 us, profiles/r03b_tail_probe.log), else the split-K 32x32 tail kernel
// (long K, few columns: 17 us against 28-32 us).
constexpr int GEMM_REST_T128_ABOVE_ROWS = 512, GEMM_REST_T64_MIN_TILES = 192;

inline int gemm_plan_gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// Rows (a multiple of 256) that run_gemm hands to launch_best_persist; 0: the whole problem runs on GEMM_CFG_T128.  G = the
// persistent grid, num_cus() & ~7.  The largest row range whose tile count is a whole number of rounds of G workgroups (every CU gets
// the same number of tiles: no tail round); N % 256 == 128 runs 256x128 tiles on the ping-pong kernel, two workgroups per CU, hence
// 2 G.  Where no whole round fits (the text tower's 77 row tiles x 9 or 12 column tiles) every full row tile goes, with an uneven
// last round.  G < 8 is DEFINED as 0 rows: the round length G / gcd(G, tiles) would be 0 there.  No device this library runs on
// reports fewer than 8 CUs (MI355X: 256, also what num_cus() assumes when the query fails), so nothing changes on hardware.
inline int gemm_main_rows(int M, int N, int G) {
  if (G < 8) return 0;
  const int tiles_n = (N + 255) / 256, full_m = M / 256;
  if ((long)full_m * tiles_n < (G * GEMM_MAIN_MIN_NUM) / GEMM_MAIN_MIN_DEN) return 0;
  const int step = (N & 255) == 128 ? 2 * G / gemm_plan_gcd(2 * G, N >> 7) : G / gemm_plan_gcd(G, tiles_n);
  const int main_m = (full_m / step) * step;
  return (main_m ? main_m : full_m) * 256;      // (full_m >= 1 here: the 3/4 test has returned for 0)
}

// Kernel of the rows behind the main part of a row-split problem.
inline int gemm_rest_cfg(int rows, int N) {
  if (rows > GEMM_REST_T128_ABOVE_ROWS) return GEMM_CFG_T128;
  const long t64 = (long)((rows + 63) / 64) * ((N + 63) / 64);
  return t64 >= GEMM_REST_T64_MIN_TILES ? GEMM_CFG_T64 : GEMM_CFG_TAIL;
}
