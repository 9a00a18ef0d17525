// The training transform of the tactile recipe on the GPU, one call per batch:
//
//   vl_tactile_augment = ToTensor + RandomResizedCrop(bilinear) + RandomHorizontalFlip + RandomVerticalFlip +
//                        RandomRotation(nearest, fill 0) + Normalize on an RGB sample
//                        (modal_tactile/processors/tact_processor.py:189-233).
//
// Every random scalar is the host's (Tactile_Processor_Train.draw): a sample arrives as one 96-byte record.  Two launches:
//   1. horizontal pass: for the source rows of the crop box that the vertical taps touch, the S columns of the resized image,
//      taps relative to the box and clamped into it (F.interpolate sees only the slice).  Bytes are divided by 255 (ToTensor,
//      an IEEE division) as they are read.  One float4 (R, G, B, 0) per (row, column) goes to the intermediate.  Nothing is
//      flipped here.
//   2. vertical + gather pass: one thread per OUTPUT pixel (x, y).  The three index maps that follow the resize - the two
//      flips and the rotation - are folded into the address: the thread finds the pixel (sx, sy) of the flipped image that
//      the rotation's nearest sampling takes (torchvision's affine grid and grid_sample's un-normalisation, float32, every
//      operation rounded on its own), un-flips it to (sx', sy') of the resized image, and runs the vertical tap loop of
//      output row sy' over column sx' of the intermediate, one float4 load per tap.  A pixel whose source lies outside the
//      image is the fill: it takes no loads and ends as (0 - mean) / std.  The resized image is never in memory, and the
//      corners of it that the rotation throws away are never computed.
// The tap sum of a resized pixel (sy', sx') is one loop whose trip count and operands depend on (sy', sx') alone, so it has
// the same bits whichever output pixel asks for it: a rotated or flipped output is a permutation of the unrotated one.
#include "vl_common.h"
#include "vitlens_hip.h"

extern "C" int vl_set_error(const char* msg);

namespace {

// one record per sample, as include/vitlens_hip.h spells it out (96 bytes)
struct TactileAugRec {
  uint64_t src;                               // device pointer: uint8 [H,W,3]
  int32_t stride;                             // bytes per row of src
  int32_t H, W;
  int32_t top, left, bh, bw;                  // the crop box
  int32_t row0, nrows;                        // rows of the box (relative to top) the vertical taps touch
  int32_t hb, hw, hks, vb, vw, vks;           // word offsets of bounds / weights into `tables`, taps per row
  int32_t flags;                              // 1 horizontal flip, 2 vertical flip
  int64_t tmp;                                // offset of the sample's intermediate, in float4
  float t00, t01, t10, t11;                   // the rotation's rescaled inverse matrix (float32, formed on the host)
};
static_assert(sizeof(TactileAugRec) == 96, "vl_tactile_augment: the parameter record is 24 words");

constexpr int F_HFLIP = 1, F_VFLIP = 2;
constexpr int VG_TILE = 16;                   // the gather pass's workgroup: VG_TILE x VG_TILE output pixels, 256 threads

struct NormP { float mean[3], std[3]; };

__global__ void __launch_bounds__(256) tactile_h_kernel(const TactileAugRec* __restrict__ recs, int S, const int* __restrict__ tables,
                                                        f32x4* __restrict__ tmp) {
  const TactileAugRec& p = recs[blockIdx.z];
  const int nrows = p.nrows;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)nrows * S) return;
  const int r = (int)(i / S), x = (int)(i - (long)r * S);
  const int* bounds = tables + p.hb;
  const int xmin = bounds[2 * x], n = min(bounds[2 * x + 1], p.hks);
  const float* w = (const float*)(tables + p.hw) + (long)x * p.hks;
  // a row or column outside the image is clamped into it: a bad record gives a wrong pixel, never a read outside the source
  const int row = min(max(p.top + p.row0 + r, 0), p.H - 1);
  const unsigned char* rgb = (const unsigned char*)p.src + (long)row * p.stride;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < n; ++j) {
    const int col = min(max(p.left + min(max(xmin + j, 0), p.bw - 1), 0), p.W - 1);
    const unsigned char* px = rgb + (long)col * 3;
    const f32x4 v = {(float)px[0] / 255.0f, (float)px[1] / 255.0f, (float)px[2] / 255.0f, 0.f};
    acc += w[j] * v;
  }
  tmp[p.tmp + (long)r * S + x] = acc;
}

// F.rotate(NEAREST, expand=False, center=None) at output pixel (x, y) of an S x S image -> the pixel it samples, false
// where that lies outside the image (the fill).  torchvision's base grid is x - S/2 + 0.5 (an integer or a half-integer,
// exact), its grid the product with the rescaled matrix, grid_sample un-normalises with align_corners=False and rounds
// half to even.  Every operation is rounded on its own, as the separate torch kernels round them.
__device__ __forceinline__ bool rotate_source(const TactileAugRec& p, int S, int x, int y, int& sx, int& sy) {
#pragma clang fp contract(off)
  const float half = 0.5f * (float)S, fs = (float)S;
  const float xb = (float)x - half + 0.5f, yb = (float)y - half + 0.5f;
  const float gx = xb * p.t00 + yb * p.t01, gy = xb * p.t10 + yb * p.t11;
  const float ix = ((gx + 1.0f) * fs - 1.0f) / 2.0f, iy = ((gy + 1.0f) * fs - 1.0f) / 2.0f;
  const float rx = rintf(ix), ry = rintf(iy);
  if (!(rx >= 0.f && rx < fs && ry >= 0.f && ry < fs)) return false;     // a NaN is a fill too
  sx = (int)rx; sy = (int)ry;
  return true;
}

__global__ void __launch_bounds__(256) tactile_vg_kernel(const TactileAugRec* __restrict__ recs, int S, const int* __restrict__ tables,
                                                         const f32x4* __restrict__ tmp, const NormP np, float* __restrict__ out) {
  const TactileAugRec& p = recs[blockIdx.z];
  // a workgroup is a 16 x 16 tile of the output (a wave 16 x 4: 64-byte store segments): whatever the angle, its sources
  // lie in a square of at most 23 x 23 pixels of the intermediate, whose lines its lanes share; 256 pixels of one output
  // row would cross 180 rows of it
  const int x = blockIdx.x * VG_TILE + (threadIdx.x & (VG_TILE - 1)), y = blockIdx.y * VG_TILE + threadIdx.x / VG_TILE;
  if (x >= S || y >= S) return;
  const long plane = (long)S * S;
  float* o = out + (long)blockIdx.z * 3 * plane + (long)y * S + x;
  int sx, sy;
  if (!rotate_source(p, S, x, y, sx, sy)) {
    o[0] = (0.f - np.mean[0]) / np.std[0]; o[plane] = (0.f - np.mean[1]) / np.std[1]; o[2 * plane] = (0.f - np.mean[2]) / np.std[2];
    return;
  }
  if (p.flags & F_HFLIP) sx = S - 1 - sx;
  if (p.flags & F_VFLIP) sy = S - 1 - sy;
  const int* bounds = tables + p.vb;
  const int ymin = bounds[2 * sy], n = min(bounds[2 * sy + 1], p.vks);
  const float* w = (const float*)(tables + p.vw) + (long)sy * p.vks;
  const f32x4* t = tmp + p.tmp + sx;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < n; ++j) {
    const int yy = min(max(min(max(ymin + j, 0), p.bh - 1) - p.row0, 0), p.nrows - 1);
    acc += w[j] * t[(long)yy * S];
  }
  o[0] = (acc.x - np.mean[0]) / np.std[0]; o[plane] = (acc.y - np.mean[1]) / np.std[1]; o[2 * plane] = (acc.z - np.mean[2]) / np.std[2];
}

}  // namespace

extern "C" int vl_tactile_augment(const void* records, int n, int S, int max_nrows, const void* tables, float* tmp, const float* mean,
                                  const float* stdv, float* out, hipStream_t stream) {
  if (n <= 0 || n > 65535 || S <= 0 || S > 4096 || max_nrows <= 0)
    return vl_set_error("vl_tactile_augment: bad shape (1 <= n <= 65535, 1 <= S <= 4096, max_nrows >= 1)");
  if (!records || !tables || !tmp || !mean || !stdv || !out) return vl_set_error("vl_tactile_augment: null operand");
  if ((((uintptr_t)records) & 7) != 0 || (((uintptr_t)tmp) & 15) != 0)
    return vl_set_error("vl_tactile_augment: the records must be 8-byte aligned and the intermediate 16-byte aligned");
  NormP np;
  for (int c = 0; c < 3; ++c) { np.mean[c] = mean[c]; np.std[c] = stdv[c]; }
  if (np.std[0] == 0.f || np.std[1] == 0.f || np.std[2] == 0.f) return vl_set_error("vl_tactile_augment: std must be non-zero");
  const TactileAugRec* recs = (const TactileAugRec*)records;
  const unsigned gh = (unsigned)(((long)max_nrows * S + 255) / 256), gv = (unsigned)((S + VG_TILE - 1) / VG_TILE);
  hipLaunchKernelGGL(tactile_h_kernel, dim3(gh, 1, n), dim3(256), 0, stream, recs, S, (const int*)tables, (f32x4*)tmp);
  hipLaunchKernelGGL(tactile_vg_kernel, dim3(gv, gv, n), dim3(VG_TILE * VG_TILE), 0, stream, recs, S, (const int*)tables,
                     (const f32x4*)tmp, np, out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}
