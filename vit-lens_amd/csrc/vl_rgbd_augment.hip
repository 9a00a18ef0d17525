// The training transform of the depth recipe on the GPU, one call per batch:
//
//   vl_rgbd_augment = ToTensor + DepthNorm + RandomResizedCrop(bilinear) + RandomHorizontalFlip + ColorJitter3d +
//                     RandomErasing + Normalize on an RGB-D sample (modal_depth/processors/vt_processor.py:94-207,
//                     transforms_rgbd.py; RandAugment3d is the identity on four channels).
//
// Every random scalar is the host's (RGBD_Processor_Train.draw): a sample arrives as one 136-byte record.  Three launches:
//   1. horizontal pass: for the source rows of the crop box that the vertical taps touch, the S output columns of all four
//      channels, taps relative to the box and clamped into it (F.interpolate sees only the slice).  RGB bytes are divided by
//      255 (ToTensor, an IEEE division) and depth is clamped and scaled (DepthNorm) as they are read; a flipped sample reads
//      the table row of S-1-x.  One float4 per (row, column) goes to the intermediate.
//   2. vertical pass: one float4 load per tap; depth is finished here (erase, normalise), RGB goes to its planes unnormalised.
//   3. colour pass, one workgroup per sample, in place on the RGB planes: a first sweep applies the jitter terms in front of
//      the contrast term and reduces the grey mean (per-thread sums in index order, wave butterfly, waves in order: the same
//      bits wherever the sample stands in the batch), a second sweep applies the whole chain, the erase and the normalisation.
//      Without an enabled contrast term the first sweep is skipped.
// The launches are split because the contrast mean needs every resampled pixel of the sample (588 KiB of planes at S = 224,
// more than a CU's LDS), and the two resampling passes because the intermediate rows are shared by all S output rows.
#include "vl_common.h"
#include "vitlens_hip.h"
#include "vl_colour_jitter.h"

extern "C" int vl_set_error(const char* msg);

namespace {

// one record per sample, as include/vitlens_hip.h spells it out (136 bytes)
struct RgbdAugRec {
  uint64_t rgb, depth;                        // device pointers: uint8 [H,W,3], float32 [H,W]
  int32_t rgb_stride, depth_stride;           // bytes per row of rgb, floats per row of depth
  int32_t H, W;
  int32_t top, left, bh, bw;                  // the crop box
  int32_t row0, nrows;                        // rows of the box (relative to top) the vertical taps touch
  int32_t hb, hw, hks, vb, vw, vks;           // word offsets of bounds / weights into `tables`, taps per row
  int64_t tmp;                                // offset of the sample's intermediate, in float4
  int32_t flags;
  float b, b1, c, c1, s, s1, hue;             // factor and 1 - factor (formed in double on the host), hue shift
  int32_t ei, ej, eh, ew;                     // erase rectangle in the output
};
static_assert(sizeof(RgbdAugRec) == 136, "vl_rgbd_augment: the parameter record is 34 words");

constexpr int F_ERASE = 32;                   // beside the flag bits of csrc/vl_colour_jitter.h

struct NormP { float mean[4], std[4]; };
struct DepthP { float lo, hi, div; };

__device__ __forceinline__ bool erased(const RgbdAugRec& p, int y, int x) {
  return (p.flags & F_ERASE) && y >= p.ei && y < p.ei + p.eh && x >= p.ej && x < p.ej + p.ew;
}

__global__ void __launch_bounds__(256) rgbd_h_kernel(const RgbdAugRec* __restrict__ recs, int S, const int* __restrict__ tables,
                                                     f32x4* __restrict__ tmp, const DepthP dp) {
  const RgbdAugRec& p = recs[blockIdx.z];
  const int nrows = p.nrows;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)nrows * S) return;
  const int r = (int)(i / S), x = (int)(i - (long)r * S);
  const int xo = (p.flags & F_FLIP) ? S - 1 - x : x;
  const int* bounds = tables + p.hb;
  const int xmin = bounds[2 * xo], n = min(bounds[2 * xo + 1], p.hks);
  const float* w = (const float*)(tables + p.hw) + (long)xo * p.hks;
  // a row or column outside the image is clamped into it: a bad record gives a wrong pixel, never a read outside the source
  const int row = min(max(p.top + p.row0 + r, 0), p.H - 1);
  const unsigned char* rgb = (const unsigned char*)p.rgb + (long)row * p.rgb_stride;
  const float* dep = (const float*)p.depth + (long)row * p.depth_stride;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < n; ++j) {
    const int col = min(max(p.left + min(max(xmin + j, 0), p.bw - 1), 0), p.W - 1);
    const unsigned char* px = rgb + (long)col * 3;
    const f32x4 v = {(float)px[0] / 255.0f, (float)px[1] / 255.0f, (float)px[2] / 255.0f,
                     fminf(fmaxf(dep[col], dp.lo), dp.hi) / dp.div};
    acc += w[j] * v;
  }
  tmp[p.tmp + (long)r * S + x] = acc;
}

__global__ void __launch_bounds__(256) rgbd_v_kernel(const RgbdAugRec* __restrict__ recs, int S, const int* __restrict__ tables,
                                                     const f32x4* __restrict__ tmp, float depth_mean, float depth_std,
                                                     float* __restrict__ out_rgb, float* __restrict__ out_depth) {
  const RgbdAugRec& p = recs[blockIdx.z];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= S * S) return;
  const int y = i / S, x = i - y * S;
  const int* bounds = tables + p.vb;
  const int ymin = bounds[2 * y], n = min(bounds[2 * y + 1], p.vks);
  const float* w = (const float*)(tables + p.vw) + (long)y * p.vks;
  const f32x4* t = tmp + p.tmp;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < n; ++j) {
    const int yy = min(max(min(max(ymin + j, 0), p.bh - 1) - p.row0, 0), p.nrows - 1);
    acc += w[j] * t[(long)yy * S + x];
  }
  const long plane = (long)S * S;
  float* o = out_rgb + (long)blockIdx.z * 3 * plane + i;
  o[0] = acc.x; o[plane] = acc.y; o[2 * plane] = acc.z;
  out_depth[(long)blockIdx.z * plane + i] = ((erased(p, y, x) ? 0.f : acc.w) - depth_mean) / depth_std;
}

__global__ void __launch_bounds__(RA_THREADS) rgbd_colour_kernel(const RgbdAugRec* __restrict__ recs, int S, const NormP np,
                                                                 float* __restrict__ out_rgb) {
  __shared__ float s_red[RA_WAVES];
  const RgbdAugRec p = recs[blockIdx.x];
  const int plane = S * S;
  float* o = out_rgb + (long)blockIdx.x * 3 * plane;
  float mean = 0.f;
  if (p.flags & F_CONTRAST) {
    float sum = 0.f;
    for (int i = threadIdx.x; i < plane; i += RA_THREADS) {
      float r = o[i], g = o[plane + i], b = o[2 * plane + i];
      jitter<true>(r, g, b, p, 0.f);
      sum += grey(r, g, b);
    }
    mean = block_sum(sum, s_red) / (float)plane;
  }
  for (int i = threadIdx.x; i < plane; i += RA_THREADS) {
    float r = o[i], g = o[plane + i], b = o[2 * plane + i];
    jitter<false>(r, g, b, p, mean);
    const int y = i / S;
    if (erased(p, y, i - y * S)) r = g = b = 0.f;
    o[i] = (r - np.mean[0]) / np.std[0];
    o[plane + i] = (g - np.mean[1]) / np.std[1];
    o[2 * plane + i] = (b - np.mean[2]) / np.std[2];
  }
}

}  // namespace

extern "C" int vl_rgbd_augment(const void* records, int n, int S, int max_nrows, const void* tables, float* tmp, const float* mean,
                               const float* stdv, float depth_lo, float depth_hi, float depth_div, float* out_rgb,
                               float* out_depth, hipStream_t stream) {
  if (n <= 0 || n > 65535 || S <= 0 || S > 4096 || max_nrows <= 0)
    return vl_set_error("vl_rgbd_augment: bad shape (1 <= n <= 65535, 1 <= S <= 4096, max_nrows >= 1)");
  if (!records || !tables || !tmp || !mean || !stdv || !out_rgb || !out_depth) return vl_set_error("vl_rgbd_augment: null operand");
  if ((((uintptr_t)records) & 7) != 0 || (((uintptr_t)tmp) & 15) != 0)
    return vl_set_error("vl_rgbd_augment: the records must be 8-byte aligned and the intermediate 16-byte aligned");
  NormP np;
  for (int c = 0; c < 4; ++c) { np.mean[c] = mean[c]; np.std[c] = stdv[c]; }
  if (np.std[0] == 0.f || np.std[1] == 0.f || np.std[2] == 0.f || np.std[3] == 0.f || depth_div == 0.f)
    return vl_set_error("vl_rgbd_augment: std and the depth divisor must be non-zero");
  const RgbdAugRec* recs = (const RgbdAugRec*)records;
  const DepthP dp{depth_lo, depth_hi, depth_div};
  const unsigned gh = (unsigned)(((long)max_nrows * S + 255) / 256), gv = (unsigned)(((long)S * S + 255) / 256);
  hipLaunchKernelGGL(rgbd_h_kernel, dim3(gh, 1, n), dim3(256), 0, stream, recs, S, (const int*)tables, (f32x4*)tmp, dp);
  hipLaunchKernelGGL(rgbd_v_kernel, dim3(gv, 1, n), dim3(256), 0, stream, recs, S, (const int*)tables, (const f32x4*)tmp, np.mean[3],
                     np.std[3], out_rgb, out_depth);
  hipLaunchKernelGGL(rgbd_colour_kernel, dim3(n), dim3(RA_THREADS), 0, stream, recs, S, np, out_rgb);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}
