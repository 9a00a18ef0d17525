// Prints the row-split plan of csrc/vl_gemm_plan.h over a grid, for tests/test_gemm_plan_host.py (which holds the oracle).
//   main G N rem : gemm_main_rows(t * 256 + rem, N, G) for t = 0 .. 1100
//   rest N       : gemm_rest_cfg(rows, N) for rows = 1 .. 600
#include <cstdio>
#include <vector>

#include "vl_gemm_plan.h"

int main() {
  std::vector<int> widths;
  for (int n = 64; n <= 8192; n += 64) widths.push_back(n);
  for (int n : {1000, 1664, 4992}) widths.push_back(n);
  for (int G : {0, 4, 8, 64, 104, 256, 304})
    for (int N : widths)
      for (int rem : {0, 40, 255}) {
        std::printf("main %d %d %d :", G, N, rem);
        for (int t = 0; t <= 1100; ++t) std::printf(" %d", gemm_main_rows(t * 256 + rem, N, G));
        std::printf("\n");
      }
  for (int N : widths) {
    std::printf("rest %d :", N);
    for (int rows = 1; rows <= 600; ++rows) std::printf(" %d", gemm_rest_cfg(rows, N));
    std::printf("\n");
  }
  return 0;
}
