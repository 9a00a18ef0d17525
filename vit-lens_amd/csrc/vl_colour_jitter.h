// ColorJitter on one float pixel, as torchvision's tensor path computes it, and the fixed-order reduction of the contrast
// term's grey mean: one definition for the colour pass of the depth recipe (csrc/vl_rgbd_augment.hip) and the float tail of
// the plain-image recipe (csrc/vl_image_augment.hip); `jitter` is a template on the record type.  A record type provides flags (the F_ bits below), b, b1, c, c1, s, s1
// (factor and 1 - factor, the difference formed in double on the host) and hue.
#pragma once
#include "vl_common.h"

namespace {

// `block_sum` adds the partial sums of a workgroup of exactly RA_THREADS threads: both colour kernels are launched with it
constexpr int RA_THREADS = 1024;
constexpr int RA_WAVES = RA_THREADS / 64;
// the bits of a record's `flags` that the chain reads (bit 32 is the depth recipe's own)
constexpr int F_FLIP = 1, F_BRIGHT = 2, F_CONTRAST = 4, F_SAT = 8, F_HUE = 16, F_ORDER_SHIFT = 8;

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float grey(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }

// torchvision's adjust_hue on one pixel: _rgb2hsv, h = (h + shift) mod 1 (floor-mod), _hsv2rgb
__device__ __forceinline__ void hue_shift(float& r, float& g, float& b, float shift) {
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.f : maxc);
  const float div = eqc ? 1.f : cr;
  const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
  const float hr = maxc == r ? bc - gc : 0.f;
  const float hg = (maxc == g && maxc != r) ? 2.f + rc - bc : 0.f;
  const float hb = (maxc != g && maxc != r) ? 4.f + gc - rc : 0.f;
  float h = (hr + hg + hb) / 6.f + 1.f;
  h -= floorf(h);                               // fmod(x, 1) of a positive x
  h += shift;
  h -= floorf(h);                               // the floor-mod of torch's %
  const float v = maxc;
  const float h6 = h * 6.f, fl = floorf(h6), f = h6 - fl;
  const int sector = ((int)fl) % 6;
  const float pp = clamp01(v * (1.f - s)), q = clamp01(v * (1.f - s * f)), t = clamp01(v * (1.f - s * (1.f - f)));
  switch (sector) {
    case 0: r = v; g = t; b = pp; break;
    case 1: r = q; g = v; b = pp; break;
    case 2: r = pp; g = v; b = t; break;
    case 3: r = pp; g = q; b = v; break;
    case 4: r = t; g = pp; b = v; break;
    default: r = v; g = pp; b = q; break;
  }
}

// The jitter terms in the drawn order.  STOP_AT_CONTRAST: only the terms in front of the contrast term (first sweep).
template <bool STOP_AT_CONTRAST, typename Rec>
__device__ __forceinline__ void jitter(float& r, float& g, float& b, const Rec& p, float mean) {
  const int order = p.flags >> F_ORDER_SHIFT;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int id = (order >> (2 * k)) & 3;
    if (STOP_AT_CONTRAST && id == 1) return;
    if (!(p.flags & (F_BRIGHT << id))) continue;
    if (id == 0) {
      r = clamp01(p.b * r); g = clamp01(p.b * g); b = clamp01(p.b * b);
    } else if (id == 1) {
      const float m = p.c1 * mean;
      r = clamp01(p.c * r + m); g = clamp01(p.c * g + m); b = clamp01(p.c * b + m);
    } else if (id == 2) {
      const float m = p.s1 * grey(r, g, b);
      r = clamp01(p.s * r + m); g = clamp01(p.s * g + m); b = clamp01(p.s * b + m);
    } else {
      hue_shift(r, g, b, p.hue);
    }
  }
}

// the butterfly leaves the same bits in every lane (a + b == b + a); the waves' partials are then added in wave order
__device__ __forceinline__ float block_sum(float v, float* s_red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = s_red[0];
#pragma unroll
  for (int w = 1; w < RA_WAVES; ++w) r += s_red[w];
  return r;
}

}  // namespace
