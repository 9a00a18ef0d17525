// The plain-image training transform of the tactile and EEG recipes on the GPU, one call per batch:
//
//   vl_image_augment = RandomResizedCrop(S, bilinear) + RandomHorizontalFlip + RandAugment on the 8-bit image (every stage as
//                      the Pillow call it ends in, byte for byte), then ToTensor + ColorJitter + Normalize
//                      (modal_eeg/processors/eeg_processor.py:93-139 and modal_tactile/processors/tact_processor.py:92-138).
//
// Every random scalar is the host's (Image_Processor_Train.draw): a sample arrives as one 368-byte record.  Three launches,
// whatever the batch:
//   1. horizontal pass of Pillow's 8-bit resampler (csrc/vl_resample_u8.h) over the rows of the crop box that the vertical taps
//      touch; the taps never leave the box (Pillow crops first).
//   2. vertical pass, which writes the 8-bit S x S x 3 crop; a flipped sample's column x reads the intermediate's column S-1-x.
//   3. one workgroup per sample: the sample's RandAugment ops one after another, then the float tail.  An op reads the current
//      image and writes the other of the sample's two buffers (the geometric ops and Sharpness read anywhere around a pixel);
//      a workgroup barrier orders an op's global stores before the next op's loads.  Both buffers are 147 KiB at S = 224
//      and stay in L2.  Contrast needs the mean of L (an integer sum: LDS atomic), AutoContrast and Equalize the per-channel
//      256-bin histograms (LDS atomics, then three threads scan them); their results become a 3 x 256 LUT in LDS.
//      The tail is the colour chain of csrc/vl_colour_jitter.h (shared with vl_rgbd_augment): a first sweep for the contrast
//      term's grey mean, a second for the whole chain and the normalisation.
//
// Arithmetic of the 8-bit ops: the affine source position and the bilinear blend in doubles, the enhance blends
// and the SMOOTH filter in float32, every operation rounded on its own (fp contract off: nothing becomes an fma), then
// Pillow's truncation; the LUT ops are integer, AutoContrast's scale and offset doubles.
#include "vl_common.h"
#include "vitlens_hip.h"
#include "vl_colour_jitter.h"
#include "vl_resample_u8.h"

extern "C" int vl_set_error(const char* msg);

namespace {

enum { OP_IDENTITY = 0, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y, OP_ROTATE, OP_BRIGHTNESS, OP_COLOR, OP_CONTRAST,
       OP_SHARPNESS, OP_POSTERIZE, OP_SOLARIZE, OP_AUTOCONTRAST, OP_EQUALIZE };
constexpr int MAX_OPS = 4;

// one op slot of the record (64 bytes)
struct ImageOp {
  int32_t code;                               // OP_*
  int32_t ipay;                               // Posterize: the byte mask; Solarize: the threshold (bytes >= it are inverted)
  float fpay;                                 // the enhance ops: the factor 1 + m
  int32_t pad;
  double m[6];                                // the geometric ops: output pixel centre -> source position
};

// one record per sample, as include/vitlens_hip.h spells it out (368 bytes)
struct ImageAugRec {
  uint64_t src;                               // device pointer: uint8 [H,W,3]
  int32_t stride, H, W;                       // bytes per row of src
  int32_t top, left, bh, bw;                  // the crop box
  int32_t row0, nrows;                        // rows of the box (relative to top) the vertical taps touch
  int32_t hb, hk, hks, vb, vk, vks;           // word offsets of bounds / coefficients into `tables`, taps per row
  int32_t flags;                              // F_FLIP, the jitter enables and order (csrc/vl_colour_jitter.h)
  int64_t tmp;                                // byte offset of the sample's [nrows,S,3] intermediate
  float b, b1, c, c1, s, s1, hue;             // factor and 1 - factor (formed in double on the host), hue shift
  int32_t num_ops;
  ImageOp ops[MAX_OPS];
};
static_assert(sizeof(ImageOp) == 64 && sizeof(ImageAugRec) == 368, "vl_image_augment: the parameter record is 92 words");

struct NormP { float mean[3], std[3]; };

// A table entry or row outside the box is clamped into it: a bad record gives a wrong pixel, never a read outside the source.
__global__ void __launch_bounds__(256) image_h_kernel(const ImageAugRec* __restrict__ recs, int S, const int* __restrict__ tables,
                                                      unsigned char* __restrict__ tmp) {
  const ImageAugRec& p = recs[blockIdx.z];
  const int nrows = p.nrows;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)nrows * S) return;
  const int r = (int)(i / S), x = (int)(i - (long)r * S);
  const int* bounds = tables + p.hb;
  const int xmin = min(max(bounds[2 * x], 0), p.bw - 1), n = min(min(bounds[2 * x + 1], p.hks), p.bw - xmin);
  const int row = min(max(p.top + p.row0 + r, 0), p.H - 1);
  const unsigned char* src = (const unsigned char*)p.src;
  const unsigned char* end = src + (long)(p.H - 1) * p.stride + (long)p.W * 3;
  h_pixel<3>(src + (long)row * p.stride + (long)(p.left + xmin) * 3, tables + p.hk + (long)x * p.hks, n, end,
             tmp + p.tmp + ((long)r * S + x) * 3);
}

__global__ void __launch_bounds__(256) image_v_kernel(const ImageAugRec* __restrict__ recs, int S, const int* __restrict__ tables,
                                                      const unsigned char* __restrict__ tmp, unsigned char* __restrict__ img) {
  const ImageAugRec& p = recs[blockIdx.z];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= S * S) return;
  const int y = i / S, x = i - y * S;
  const int xs = (p.flags & F_FLIP) ? S - 1 - x : x;
  const int* bounds = tables + p.vb;
  const int y0 = min(max(bounds[2 * y] - p.row0, 0), p.nrows - 1), n = min(min(bounds[2 * y + 1], p.vks), p.nrows - y0);
  const unsigned char* t = tmp + p.tmp;
  int acc[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
  tap_loop<3>(t + ((long)y0 * S + xs) * 3, (long)S * 3, tables + p.vk + (long)y * p.vks, n, t + (long)p.nrows * S * 3, acc);
  unsigned char* o = img + ((long)blockIdx.z * S * S + i) * 3;
  o[0] = clip8(acc[0]); o[1] = clip8(acc[1]); o[2] = clip8(acc[2]);
}

// From here on every floating-point operation is rounded on its own, as in Pillow's C and in Python: a product and a sum are
// never contracted into an fma (the functions of the two headers above keep the default, as in vl_rgbd_augment).
#pragma clang fp contract(off)

// Pillow's (UINT8) of a float that its clip left in [0, 255]
__device__ __forceinline__ unsigned char clip8f(float v) { return v <= 0.f ? 0 : v >= 255.f ? 255 : (unsigned char)(int)v; }

// ImagingConvert rgb -> L
__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// a + (b - a) d in doubles, each operation rounded on its own (Geometry.c BILINEAR)
__device__ __forceinline__ double lerp_rn(double a, double b, double d) { return a + (b - a) * d; }

// The pixel passes below take the pixels first, first + stride, ...: a workgroup that owns a sample passes (threadIdx.x,
// RA_THREADS).

// Image.transform(size, AFFINE, m, BILINEAR) of an S x S x 3 image
__device__ void affine_op(const unsigned char* cur, unsigned char* nxt, int S, const double* m, int first, int stride) {
  const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
  for (int i = first; i < S * S; i += stride) {
    const int yo = i / S, xo = i - yo * S;
    const double xc = (double)xo + 0.5, yc = (double)yo + 0.5;
    double xin = m0 * xc + m1 * yc + m2;
    double yin = m3 * xc + m4 * yc + m5;
    unsigned char* o = nxt + (long)i * 3;
    if (!(xin >= 0.0 && xin < (double)S && yin >= 0.0 && yin < (double)S)) {      // a NaN is outside too
      o[0] = o[1] = o[2] = 0;
      continue;
    }
    xin -= 0.5; yin -= 0.5;
    const double fx = floor(xin), fy = floor(yin);
    const double dx = xin - fx, dy = yin - fy;
    const int x = (int)fx, y = (int)fy;
    const int x0 = min(max(x, 0), S - 1) * 3, x1 = min(max(x + 1, 0), S - 1) * 3;
    const unsigned char* r0 = cur + (long)min(max(y, 0), S - 1) * S * 3;
    const bool below = y + 1 >= 0 && y + 1 < S;
    const unsigned char* r1 = cur + (long)min(max(y + 1, 0), S - 1) * S * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v1 = lerp_rn((double)r0[x0 + c], (double)r0[x1 + c], dx);
      const double v2 = below ? lerp_rn((double)r1[x0 + c], (double)r1[x1 + c], dx) : v1;
      o[c] = (unsigned char)(int)lerp_rn(v1, v2, dy);
    }
  }
}

// ImageEnhance.*.enhance(f) = Image.blend(degenerate, image, f): degenerate + f (image - degenerate) in float32, clipped,
// truncated.  The degenerate image: black (Brightness), L (Color), the rounded mean of L (Contrast), ImageFilter.SMOOTH
// (Sharpness: (1 1 1 / 1 5 1 / 1 1 1) / 13 in float32 from 0.5, the row below first, the border copied).
__device__ void enhance_op(const unsigned char* cur, unsigned char* nxt, int S, int code, float f, int mean, int first, int stride) {
  const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  for (int i = first; i < S * S; i += stride) {
    const unsigned char* px = cur + (long)i * 3;
    int deg[3] = {0, 0, 0};
    if (code == OP_COLOR) {
      deg[0] = deg[1] = deg[2] = luma(px[0], px[1], px[2]);
    } else if (code == OP_CONTRAST) {
      deg[0] = deg[1] = deg[2] = mean;
    } else if (code == OP_SHARPNESS) {
      const int y = i / S, x = i - y * S;
      if (y == 0 || y == S - 1 || x == 0 || x == S - 1) {
        deg[0] = px[0]; deg[1] = px[1]; deg[2] = px[2];
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float ss = 0.5f;
#pragma unroll
          for (int dy = 1; dy >= -1; --dy) {
            const unsigned char* q = px + (long)dy * S * 3 + c;
            ss += (float)q[-3] * k1 + (float)q[0] * (dy == 0 ? k5 : k1) + (float)q[3] * k1;
          }
          deg[c] = clip8f(ss);
        }
      }
    }
    unsigned char* o = nxt + (long)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = clip8f((float)deg[c] + f * (float)((int)px[c] - deg[c]));
  }
}

struct ChanStat { int lo, hi, nz; unsigned total, last; };

// Contrast's degenerate value, by a workgroup of RA_THREADS: int(sum(L) / count + 0.5), the division and the sum in doubles as
// Python's; the sum itself is an integer
__device__ int luma_mean(const unsigned char* cur, int S, unsigned* s_sum) {
  const int tid = threadIdx.x, npx = S * S;
  if (tid == 0) *s_sum = 0;
  __syncthreads();
  unsigned sum = 0;
  for (int i = tid; i < npx; i += RA_THREADS) {
    const unsigned char* px = cur + (long)i * 3;
    sum += (unsigned)luma(px[0], px[1], px[2]);
  }
  atomicAdd(s_sum, sum);
  __syncthreads();
  return (int)((double)*s_sum / (double)npx + 0.5);
}

// ImageOps.posterize / solarize / autocontrast / equalize: a LUT per channel, built in LDS by a workgroup of RA_THREADS
__device__ void build_lut(const unsigned char* cur, int S, int code, int ipay, unsigned* s_hist, unsigned* s_pref, ChanStat* s_stat,
                          unsigned char* s_lut) {
  const int tid = threadIdx.x, npx = S * S;
  if (code == OP_AUTOCONTRAST || code == OP_EQUALIZE) {
    if (tid < 768) s_hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < npx; i += RA_THREADS) {
      const unsigned char* px = cur + (long)i * 3;
      atomicAdd(&s_hist[px[0]], 1u); atomicAdd(&s_hist[256 + px[1]], 1u); atomicAdd(&s_hist[512 + px[2]], 1u);
    }
    __syncthreads();
    if (tid < 3) {
      ChanStat st{-1, -1, 0, 0u, 0u};
      unsigned run = 0;
      for (int i = 0; i < 256; ++i) {
        const unsigned v = s_hist[tid * 256 + i];
        s_pref[tid * 256 + i] = run;              // pixels below value i
        run += v;
        if (v) { if (st.lo < 0) st.lo = i; st.hi = i; ++st.nz; st.last = v; }
      }
      st.total = run;
      s_stat[tid] = st;
    }
    __syncthreads();
  }
  if (tid < 768) {
    const int c = tid >> 8, i = tid & 255;
    int v = i;
    if (code == OP_POSTERIZE) {
      v = i & ipay;
    } else if (code == OP_SOLARIZE) {
      v = i < ipay ? i : 255 - i;
    } else if (code == OP_AUTOCONTRAST) {
      const ChanStat st = s_stat[c];
      if (st.hi > st.lo) {
        const double scale = 255.0 / (double)(st.hi - st.lo), offset = -(double)st.lo * scale;
        v = min(max((int)((double)i * scale + offset), 0), 255);
      }
    } else {
      const ChanStat st = s_stat[c];
      const unsigned step = st.nz <= 1 ? 0u : (st.total - st.last) / 255u;
      if (step) v = (int)min((step / 2u + s_pref[tid]) / step, 255u);
    }
    s_lut[tid] = (unsigned char)v;
  }
  __syncthreads();
}

__device__ void apply_lut(const unsigned char* cur, unsigned char* nxt, int S, const unsigned char* lut, int first, int stride) {
  for (int i = first; i < S * S; i += stride) {
    const unsigned char* px = cur + (long)i * 3;
    unsigned char* o = nxt + (long)i * 3;
    o[0] = lut[px[0]]; o[1] = lut[256 + px[1]]; o[2] = lut[512 + px[2]];
  }
}

__global__ void __launch_bounds__(RA_THREADS) image_aug_kernel(const ImageAugRec* __restrict__ recs, int S, unsigned char* img0,
                                                               unsigned char* img1, const NormP np, float* __restrict__ out,
                                                               unsigned char* __restrict__ out_u8) {
  __shared__ unsigned s_hist[768], s_pref[768];
  __shared__ unsigned char s_lut[768];
  __shared__ ChanStat s_stat[3];
  __shared__ unsigned s_sum;
  __shared__ float s_red[RA_WAVES];
  const ImageAugRec& p = recs[blockIdx.x];
  const int plane = S * S, tid = threadIdx.x;
  unsigned char* cur = img0 + (long)blockIdx.x * plane * 3;
  unsigned char* nxt = img1 + (long)blockIdx.x * plane * 3;
  const int nops = min(max(p.num_ops, 0), MAX_OPS);
  for (int k = 0; k < nops; ++k) {
    const ImageOp& op = p.ops[k];
    const int code = op.code;                     // the same in every thread: the branches below are uniform
    if (code <= OP_IDENTITY || code > OP_EQUALIZE) continue;
    if (code <= OP_ROTATE) {
      affine_op(cur, nxt, S, op.m, tid, RA_THREADS);
    } else if (code <= OP_SHARPNESS) {
      const int mean = code == OP_CONTRAST ? luma_mean(cur, S, &s_sum) : 0;
      enhance_op(cur, nxt, S, code, op.fpay, mean, tid, RA_THREADS);
    } else {
      build_lut(cur, S, code, op.ipay, s_hist, s_pref, s_stat, s_lut);
      apply_lut(cur, nxt, S, s_lut, tid, RA_THREADS);
    }
    __syncthreads();                              // the op's stores are visible to the whole workgroup before the next op reads
    unsigned char* t = cur; cur = nxt; nxt = t;
  }
  // the float tail: ToTensor (an IEEE division), ColorJitter, Normalize
  float* o = out + (long)blockIdx.x * 3 * plane;
  float mean = 0.f;
  if (p.flags & F_CONTRAST) {
    float sum = 0.f;
    for (int i = tid; i < plane; i += RA_THREADS) {
      const unsigned char* px = cur + (long)i * 3;
      float r = (float)px[0] / 255.0f, g = (float)px[1] / 255.0f, b = (float)px[2] / 255.0f;
      jitter<true>(r, g, b, p, 0.f);
      sum += grey(r, g, b);
    }
    mean = block_sum(sum, s_red) / (float)plane;
  }
  for (int i = tid; i < plane; i += RA_THREADS) {
    const unsigned char* px = cur + (long)i * 3;
    float r = (float)px[0] / 255.0f, g = (float)px[1] / 255.0f, b = (float)px[2] / 255.0f;
    if (out_u8) {
      unsigned char* u = out_u8 + ((long)blockIdx.x * plane + i) * 3;
      u[0] = px[0]; u[1] = px[1]; u[2] = px[2];
    }
    jitter<false>(r, g, b, p, mean);
    o[i] = (r - np.mean[0]) / np.std[0];
    o[plane + i] = (g - np.mean[1]) / np.std[1];
    o[2 * plane + i] = (b - np.mean[2]) / np.std[2];
  }
}

inline unsigned grid1(long n) { return (unsigned)((n + 255) / 256); }

inline bool bad_shape(int n, int S, int max_nrows) { return n <= 0 || n > 65535 || S <= 0 || S > 4096 || max_nrows <= 0; }

void launch_crop_resize(const ImageAugRec* recs, int n, int S, int max_nrows, const int* tables, unsigned char* tmp, unsigned char* img,
                        hipStream_t stream) {
  hipLaunchKernelGGL(image_h_kernel, dim3(grid1((long)max_nrows * S), 1, n), dim3(256), 0, stream, recs, S, tables, tmp);
  hipLaunchKernelGGL(image_v_kernel, dim3(grid1((long)S * S), 1, n), dim3(256), 0, stream, recs, S, tables, (const unsigned char*)tmp, img);
}

}  // namespace

extern "C" int vl_image_crop_resize_u8(const void* records, int n, int S, int max_nrows, const void* tables, uint8_t* tmp,
                                       uint8_t* out_u8, hipStream_t stream) {
  if (bad_shape(n, S, max_nrows))
    return vl_set_error("vl_image_crop_resize_u8: bad shape (1 <= n <= 65535, 1 <= S <= 4096, max_nrows >= 1)");
  if (!records || !tables || !tmp || !out_u8) return vl_set_error("vl_image_crop_resize_u8: null operand");
  if ((((uintptr_t)records) & 7) != 0) return vl_set_error("vl_image_crop_resize_u8: the records must be 8-byte aligned");
  launch_crop_resize((const ImageAugRec*)records, n, S, max_nrows, (const int*)tables, tmp, out_u8, stream);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}

extern "C" int vl_image_augment(const void* records, int n, int S, int max_nrows, int max_ops, const void* tables, uint8_t* tmp,
                                uint8_t* work, const float* mean, const float* stdv, float* out, uint8_t* out_u8, hipStream_t stream) {
  if (bad_shape(n, S, max_nrows)) return vl_set_error("vl_image_augment: bad shape (1 <= n <= 65535, 1 <= S <= 4096, max_nrows >= 1)");
  if (max_ops < 0 || max_ops > MAX_OPS) return vl_set_error("vl_image_augment: num_ops must be in [0, 4]");
  if (!records || !tables || !tmp || !work || !mean || !stdv || !out) return vl_set_error("vl_image_augment: null operand");
  if ((((uintptr_t)records) & 7) != 0) return vl_set_error("vl_image_augment: the records must be 8-byte aligned");
  NormP np;
  for (int c = 0; c < 3; ++c) { np.mean[c] = mean[c]; np.std[c] = stdv[c]; }
  if (np.std[0] == 0.f || np.std[1] == 0.f || np.std[2] == 0.f) return vl_set_error("vl_image_augment: std must be non-zero");
  const ImageAugRec* recs = (const ImageAugRec*)records;
  launch_crop_resize(recs, n, S, max_nrows, (const int*)tables, tmp, work, stream);
  hipLaunchKernelGGL(image_aug_kernel, dim3(n), dim3(RA_THREADS), 0, stream, recs, S, work, work + (size_t)n * S * S * 3, np, out, out_u8);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}
