// Patch dropout (Li et al., "Scaling Language-Image Pre-training via Masking" - FLIP; PatchDropout of the reference,
// open_clip/transformer.py:53-90): in train mode a ViT tower keeps the class token and K = max(1, int(T (1 - p))) of its T
// tokens, the K with the largest of T random keys per sample (`rand.topk(K).indices`).
//
//   vl_patch_keep         = the selection: keep[b, j] = index of the j-th largest key of sample b (ties: lower index first) and
//                           its inverse inv[b, t] = j + 1 or 0.  One workgroup per sample; the keys go through LDS once as
//                           order-preserving 32-bit integers and every thread RANKS its own keys by counting the keys that
//                           beat them - exact, no sort network, no atomics, T^2 / 256 LDS broadcasts per thread (T <= 4096).
//                           Keys: the caller's floats (the module path uploads torch.randn's), or, with keys == NULL, the
//                           kernel's own Philox4x32-10 words (the fused steps: no host round trip).
//   vl_scatter_rows_keep  = the backward of the row gather, written as a gather through `inv`: every output row is written
//                           once (a kept token's gradient row, or zeros) - no fill pass, no atomics, bit-reproducible.
//
// The gather itself is fused into the token assembly: vl_assemble_ln_pre_keep (vl_rows.hip).
#include "vl_common.h"
#include "vl_philox.h"
#include "vitlens_hip.h"

namespace {

constexpr int PK_THREADS = 256;
constexpr int PK_MAX_T = 4096;

// float -> uint32 with the same order (finite values; -0.0 and +0.0 compare equal in torch.topk: one image for both)
__device__ __forceinline__ uint32_t order_bits(float f) {
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(PK_THREADS) patch_keep_kernel(const float* keys, uint64_t seed, int64_t sample0,
                                                                 int T, int K, int* keep, int* inv) {
  __shared__ uint32_t sk[PK_MAX_T];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (keys) {
    const float* kr = keys + (size_t)b * T;
    for (int t = tid; t < T; t += PK_THREADS) sk[t] = order_bits(kr[t]);
  } else {
    const uint64_t s = (uint64_t)sample0 + (uint64_t)b;
    for (int g = tid; g * 4 < T; g += PK_THREADS) {
      const U4 r = philox4x32_10(U4{(uint32_t)g, (uint32_t)s, (uint32_t)(s >> 32), 0u}, (uint32_t)seed, (uint32_t)(seed >> 32));
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) if (g * 4 + c < T) sk[g * 4 + c] = w[c];
    }
  }
  __syncthreads();
  for (int t = tid; t < T; t += PK_THREADS) {
    const uint32_t kt = sk[t];
    int rank = 0;
    // every lane reads the same word: an LDS broadcast.  A key beats kt when it is larger, or equal at a lower index
    for (int s = 0; s < t; ++s) rank += sk[s] >= kt;
    for (int s = t + 1; s < T; ++s) rank += sk[s] > kt;
    // rank is a permutation of 0 .. T-1, so every keep[b, 0 .. K-1] is written exactly once
    if (rank < K) keep[(size_t)b * K + rank] = t;
    inv[(size_t)b * T + t] = rank < K ? rank + 1 : 0;
  }
}

// One wave per output row (b, t): out[b, t, :] = inv[b, t] > 0 ? src[b, inv[b, t], :] : 0   (src rows 0 .. K per sample)
template <bool VEC>
__global__ void __launch_bounds__(256) scatter_rows_keep_kernel(const float* src, const int* inv, float* out, long rows, int T,
                                                                int K, int D) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long b = row / T;
  int j = inv[row];
  j = j < 0 ? 0 : (j > K ? K : j);                      // the index contract; keeps every read inside src
  const float* s = src + ((size_t)b * (K + 1) + j) * D;
  float* o = out + (size_t)row * D;
  if (VEC) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int e = lane * 4; e < D; e += 256) *(f32x4*)(o + e) = j > 0 ? *(const f32x4*)(s + e) : z;
  } else {
    for (int e = lane; e < D; e += 64) o[e] = j > 0 ? s[e] : 0.f;
  }
}

}  // namespace

extern "C" int vl_set_error(const char* msg);

extern "C" int vl_patch_keep(const float* keys, uint64_t seed, int64_t sample0, int B, int T, int K, int* keep,
                             int* inv, hipStream_t stream) {
  if (B <= 0 || T <= 0 || T > PK_MAX_T || K < 1 || K > T)
    return vl_set_error("vl_patch_keep: bad shape (B >= 1, 1 <= K <= T <= 4096)");
  if (!keep || !inv) return vl_set_error("vl_patch_keep: outputs missing");
  hipLaunchKernelGGL(patch_keep_kernel, dim3((unsigned)B), dim3(PK_THREADS), 0, stream, keys, seed, sample0, T, K, keep, inv);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}

extern "C" int vl_scatter_rows_keep(const float* src, const int* inv, float* out, int B, int T, int K, int D, hipStream_t stream) {
  if (B <= 0 || T <= 0 || D <= 0 || K < 1 || K > T) return vl_set_error("vl_scatter_rows_keep: bad shape (B, D >= 1, 1 <= K <= T)");
  if (!src || !inv || !out) return vl_set_error("vl_scatter_rows_keep: operands missing");
  const long rows = (long)B * T;
  if ((rows + 3) / 4 > 0x7fffffffL) return vl_set_error("vl_scatter_rows_keep: too many rows for one launch");
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  const bool vec = D % 4 == 0 && (((uintptr_t)src | (uintptr_t)out) & 15) == 0;
  if (vec) hipLaunchKernelGGL(scatter_rows_keep_kernel<true>, grid, block, 0, stream, src, inv, out, rows, T, K, D);
  else hipLaunchKernelGGL(scatter_rows_keep_kernel<false>, grid, block, 0, stream, src, inv, out, rows, T, K, D);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}
