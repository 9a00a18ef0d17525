// The launch-per-op baseline of the plain-image training transform, to measure beside the product's one-workgroup-per-sample
// kernel: the product's kernel file is compiled into this probe, and its per-pixel code is launched stage by
// stage over grids that cover every pixel of every sample.  After the two resampling launches, per op slot k: a statistics
// launch (one workgroup per sample: Contrast's mean of L, or the LUT of the four LUT ops, into global memory) and a pixel
// launch (256 threads per block, one pixel per thread, blockIdx.z = sample); then the float tail the same way (the grey mean
// with the product's fixed-order sum, then the pixel launch).  4 + 2 max_ops launches, whatever the batch.  A sample's current
// image is work[parity], parity = the number of its earlier ops that wrote an image.  The bytes are the product's; the floats
// agree to rounding (the colour chain is compiled into other kernels here, under the default contraction).
// Build: tools/build_image_aug_split_probe.sh -> tools/bin/libimage_aug_split.so; driver: tools/image_aug_split_probe.py.
#include <stdio.h>
#include "../vit-lens_amd/csrc/vl_image_augment.hip"

extern "C" int vl_set_error(const char* m) { fprintf(stderr, "error: %s\n", m); return 1; }

namespace {

struct SplitStat { int mean; float grey; unsigned char lut[768]; };

__device__ __forceinline__ bool writes_image(int code) { return code > OP_IDENTITY && code <= OP_EQUALIZE; }

// the sample's image before slot k
__device__ __forceinline__ int parity_before(const ImageAugRec& p, int k) {
  int n = 0;
  for (int j = 0; j < k; ++j) n += writes_image(p.ops[j].code) ? 1 : 0;
  return n & 1;
}

__global__ void __launch_bounds__(RA_THREADS) split_stats_kernel(const ImageAugRec* __restrict__ recs, int S, int k, const unsigned char* img0,
                                                                 const unsigned char* img1, SplitStat* __restrict__ stat) {
  __shared__ unsigned s_hist[768], s_pref[768];
  __shared__ unsigned char s_lut[768];
  __shared__ ChanStat s_stat[3];
  __shared__ unsigned s_sum;
  const ImageAugRec& p = recs[blockIdx.x];
  if (k >= min(max(p.num_ops, 0), MAX_OPS)) return;
  const int code = p.ops[k].code;
  const unsigned char* cur = (parity_before(p, k) ? img1 : img0) + (long)blockIdx.x * S * S * 3;
  if (code == OP_CONTRAST) {
    const int mean = luma_mean(cur, S, &s_sum);
    if (threadIdx.x == 0) stat[blockIdx.x].mean = mean;
  } else if (code >= OP_POSTERIZE && code <= OP_EQUALIZE) {
    build_lut(cur, S, code, p.ops[k].ipay, s_hist, s_pref, s_stat, s_lut);
    if (threadIdx.x < 768) stat[blockIdx.x].lut[threadIdx.x] = s_lut[threadIdx.x];
  }
}

__global__ void __launch_bounds__(256) split_apply_kernel(const ImageAugRec* __restrict__ recs, int S, int k, unsigned char* img0,
                                                          unsigned char* img1, const SplitStat* __restrict__ stat) {
  const ImageAugRec& p = recs[blockIdx.z];
  if (k >= min(max(p.num_ops, 0), MAX_OPS)) return;
  const ImageOp& op = p.ops[k];
  const int code = op.code;
  if (!writes_image(code)) return;
  const int par = parity_before(p, k);
  const long off = (long)blockIdx.z * S * S * 3;
  const unsigned char* cur = (par ? img1 : img0) + off;
  unsigned char* nxt = (par ? img0 : img1) + off;
  const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
  if (code <= OP_ROTATE) affine_op(cur, nxt, S, op.m, first, stride);
  else if (code <= OP_SHARPNESS) enhance_op(cur, nxt, S, code, op.fpay, stat[blockIdx.z].mean, first, stride);
  else apply_lut(cur, nxt, S, stat[blockIdx.z].lut, first, stride);
}

__global__ void __launch_bounds__(RA_THREADS) split_tail_stats_kernel(const ImageAugRec* __restrict__ recs, int S, const unsigned char* img0,
                                                                      const unsigned char* img1, SplitStat* __restrict__ stat) {
  __shared__ float s_red[RA_WAVES];
  const ImageAugRec& p = recs[blockIdx.x];
  if (!(p.flags & F_CONTRAST)) return;
  const int plane = S * S;
  const unsigned char* cur = (parity_before(p, min(max(p.num_ops, 0), MAX_OPS)) ? img1 : img0) + (long)blockIdx.x * plane * 3;
  float sum = 0.f;
  for (int i = threadIdx.x; i < plane; i += RA_THREADS) {
    const unsigned char* px = cur + (long)i * 3;
    float r = (float)px[0] / 255.0f, g = (float)px[1] / 255.0f, b = (float)px[2] / 255.0f;
    jitter<true>(r, g, b, p, 0.f);
    sum += grey(r, g, b);
  }
  const float mean = block_sum(sum, s_red) / (float)plane;
  if (threadIdx.x == 0) stat[blockIdx.x].grey = mean;
}

__global__ void __launch_bounds__(256) split_tail_apply_kernel(const ImageAugRec* __restrict__ recs, int S, const unsigned char* img0,
                                                               const unsigned char* img1, const SplitStat* __restrict__ stat, const NormP np,
                                                               float* __restrict__ out, unsigned char* __restrict__ out_u8) {
  const ImageAugRec& p = recs[blockIdx.z];
  const int plane = S * S, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  const unsigned char* px = (parity_before(p, min(max(p.num_ops, 0), MAX_OPS)) ? img1 : img0) + ((long)blockIdx.z * plane + i) * 3;
  float r = (float)px[0] / 255.0f, g = (float)px[1] / 255.0f, b = (float)px[2] / 255.0f;
  if (out_u8) {
    unsigned char* u = out_u8 + ((long)blockIdx.z * plane + i) * 3;
    u[0] = px[0]; u[1] = px[1]; u[2] = px[2];
  }
  jitter<false>(r, g, b, p, (p.flags & F_CONTRAST) ? stat[blockIdx.z].grey : 0.f);
  float* o = out + (long)blockIdx.z * 3 * plane;
  o[i] = (r - np.mean[0]) / np.std[0];
  o[plane + i] = (g - np.mean[1]) / np.std[1];
  o[2 * plane + i] = (b - np.mean[2]) / np.std[2];
}

}  // namespace

extern "C" long probe_split_stat_bytes(int n) { return (long)n * (long)sizeof(SplitStat); }

// the operands of vl_image_augment, and stat: probe_split_stat_bytes(n) device bytes
extern "C" int probe_image_augment_split(const void* records, int n, int S, int max_nrows, int max_ops, const void* tables, uint8_t* tmp,
                                         uint8_t* work, void* stat, const float* mean, const float* stdv, float* out, uint8_t* out_u8,
                                         hipStream_t stream) {
  if (bad_shape(n, S, max_nrows) || max_ops < 0 || max_ops > MAX_OPS || !records || !tables || !tmp || !work || !stat || !mean || !stdv || !out)
    return vl_set_error("probe_image_augment_split: bad operand");
  NormP np;
  for (int c = 0; c < 3; ++c) { np.mean[c] = mean[c]; np.std[c] = stdv[c]; }
  const ImageAugRec* recs = (const ImageAugRec*)records;
  unsigned char *img0 = work, *img1 = work + (size_t)n * S * S * 3;
  SplitStat* st = (SplitStat*)stat;
  const dim3 pixels(grid1((long)S * S), 1, n);
  launch_crop_resize(recs, n, S, max_nrows, (const int*)tables, tmp, img0, stream);
  for (int k = 0; k < max_ops; ++k) {
    hipLaunchKernelGGL(split_stats_kernel, dim3(n), dim3(RA_THREADS), 0, stream, recs, S, k, (const unsigned char*)img0, (const unsigned char*)img1, st);
    hipLaunchKernelGGL(split_apply_kernel, pixels, dim3(256), 0, stream, recs, S, k, img0, img1, (const SplitStat*)st);
  }
  hipLaunchKernelGGL(split_tail_stats_kernel, dim3(n), dim3(RA_THREADS), 0, stream, recs, S, (const unsigned char*)img0, (const unsigned char*)img1, st);
  hipLaunchKernelGGL(split_tail_apply_kernel, pixels, dim3(256), 0, stream, recs, S, (const unsigned char*)img0, (const unsigned char*)img1,
                     (const SplitStat*)st, np, out, out_u8);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}
