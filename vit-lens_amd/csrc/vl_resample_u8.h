// What the 8-bit Pillow resampler kernels share (csrc/vl_preproc.hip: evaluation; csrc/vl_image_augment.hip: the crop boxes of
// the plain-image training transform): the 22-bit fixed point, the clip and the tap loop of one output pixel.
#pragma once
#include "vl_common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ unsigned char clip8(int acc) {
  const int v = acc >> PRECISION_BITS;
  return (unsigned char)min(max(v, 0), 255);
}

// Tap loop of one output pixel: acc[c] += k[j] * s[j * step + c] for the C channels.  With 3 or 4 channels the bytes of a
// pixel come from ONE unaligned 4-byte load (gfx950 runs with unaligned access enabled; hipcc itself lowers an align-1
// 4-byte copy to global_load_dword) instead of C byte loads - the loop is bound by load instructions, not by bytes.  The
// fourth byte of a 3-channel pixel belongs to the next pixel; `end` is one past the last readable byte, and a thread whose
// last tap would read beyond it (the final pixel of a buffer only) takes the byte loop.
template <int C>
__device__ __forceinline__ void tap_loop(const unsigned char* __restrict__ s, long step, const int* __restrict__ k, int n,
                                         const unsigned char* end, int (&acc)[C]) {
  if (C >= 3 && s + (long)(n - 1) * step + 4 <= end) {
    for (int j = 0; j < n; ++j) {
      unsigned v;
      __builtin_memcpy(&v, s + (long)j * step, 4);
      const int kj = k[j];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += (int)((v >> (8 * c)) & 0xffu) * kj;
    }
  } else {
    for (int j = 0; j < n; ++j) {
      const int kj = k[j];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += (int)s[(long)j * step + c] * kj;
    }
  }
}

template <int C>
__device__ __forceinline__ void h_pixel(const unsigned char* __restrict__ s, const int* __restrict__ k, int n, const unsigned char* end,
                                        unsigned char* __restrict__ dst) {
  int acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
  tap_loop<C>(s, C, k, n, end, acc);
#pragma unroll
  for (int c = 0; c < C; ++c) dst[c] = clip8(acc[c]);
}

}  // namespace
