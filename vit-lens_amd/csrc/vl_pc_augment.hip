// The training transform of the 3D recipes on the GPU, one launch per batch:
//
//   vl_pc_augment  = gather of the sampled points + pc_norm / normalize_pc + random_point_dropout + the composed
//                    random_scale / shift / rotate_perturbation / rotate (ViT-Lens: open_clip/modal_3d/datasets.py:97-204,
//                    471-479; OpenShape: VitLens-OpenShape/src/utils/data.py, src/data.py:74-88) + OpenShape's colour drop.
//
// The scalar draws (ratio, scale, shifts, angles) are the host's, composed there in fp64 into one 3x3 matrix and one shift
// per sample (PCProcessorTrain); the per-point dropout field is Philox4x32-10 keyed by the sample's seed, counter = point
// index / 4 (tests/pc_augment_ref.py restates it).  One workgroup owns a cloud, as in pc_gather_norm_kernel: centroid and
// radius are fixed-order wave + LDS reductions (deterministic), and up to PCA_LDS_POINTS selected points stay in LDS between
// the passes, so each is read from global memory once; larger selections are read again.
#include "vl_common.h"
#include "vl_philox.h"
#include "vitlens_hip.h"

namespace {

constexpr int PCA_THREADS = 1024;
constexpr int PCA_WAVES = PCA_THREADS / 64;
constexpr int PCA_LDS_POINTS = 8192;          // 12 bytes each: 96 KiB of the CU's 160 KiB

// one record per sample, as include/vitlens_hip.h spells it out (64 bytes)
struct PcAugParams { float A[9]; float t[3]; float drop_ratio; int flags; uint64_t seed; };
static_assert(sizeof(PcAugParams) == 64, "vl_pc_augment: the parameter record is 16 words");

// the butterfly leaves the same bits in every lane (a + b == b + a); the waves' partials are then added in wave order
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* s_red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float w = __shfl_xor(v, o, 64);
    v = MAX ? fmaxf(v, w) : v + w;
  }
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = s_red[0];
#pragma unroll
  for (int w = 1; w < PCA_WAVES; ++w) r = MAX ? fmaxf(r, s_red[w]) : r + s_red[w];
  __syncthreads();                             // s_red is reused by the next reduction
  return r;
}

template <bool LDS>
__global__ void __launch_bounds__(PCA_THREADS) pc_augment_kernel(const float* pts, const int64_t* idx, float* out, int N, int G, int C,
                                                                 const PcAugParams* params, float feat_fill) {
  extern __shared__ __attribute__((aligned(16))) float s_xyz[];    // LDS: [4 * ceil(G / 4)][3], the gathered points
  __shared__ float s_red[PCA_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const PcAugParams pr = params[b];
  const float* P = pts + (size_t)b * N * C;
  const int64_t* I = idx ? idx + (size_t)b * G : nullptr;
  // an index outside the cloud is clamped into it: a bad index list gives a wrong point, never a read outside pts
  auto row = [&](int g) {
    long i = I ? (long)I[g] : (long)g;
    i = i < 0 ? 0 : (i >= N ? N - 1 : i);
    return P + (size_t)i * C;
  };
  auto fetch = [&](int g, float& x, float& y, float& z) {
    if constexpr (LDS) { x = s_xyz[g * 3]; y = s_xyz[g * 3 + 1]; z = s_xyz[g * 3 + 2]; }
    else { const float* r = row(g); x = r[0]; y = r[1]; z = r[2]; }
  };
  const bool norm = pr.flags & 1;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  if (LDS || norm) {
    for (int g = tid; g < G; g += PCA_THREADS) {
      const float* r = row(g);
      const float x = r[0], y = r[1], z = r[2];
      if constexpr (LDS) { s_xyz[g * 3] = x; s_xyz[g * 3 + 1] = y; s_xyz[g * 3 + 2] = z; }
      sx += x; sy += y; sz += z;
    }
  }
  if constexpr (LDS) __syncthreads();
  float mx = 0.f, my = 0.f, mz = 0.f, rad = 1.f;
  bool zero = false;
  if (norm) {
    mx = block_reduce<false>(sx, s_red) / (float)G;
    my = block_reduce<false>(sy, s_red) / (float)G;
    mz = block_reduce<false>(sz, s_red) / (float)G;
    float m = 0.f;
    for (int g = tid; g < G; g += PCA_THREADS) {
      float x, y, z;
      fetch(g, x, y, z);
      const float dx = x - mx, dy = y - my, dz = z - mz;
      m = fmaxf(m, sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))));
    }
    rad = block_reduce<true>(m, s_red);
    zero = (pr.flags & 2) && rad < 1e-6f;      // normalize_pc's guard; without it the division is done as it comes (pc_norm)
  }
  auto normalised = [&](int g, float& x, float& y, float& z) {
    fetch(g, x, y, z);
    if (norm) {
      if (zero) { x = y = z = 0.f; }
      else { x = (x - mx) / rad; y = (y - my) / rad; z = (z - mz) / rad; }
    }
  };
  float x0, y0, z0;                             // what a dropped point becomes: output point 0, normalised
  normalised(0, x0, y0, z0);
  const uint32_t k0 = (uint32_t)pr.seed, k1 = (uint32_t)(pr.seed >> 32);
  const bool fill = pr.flags & 4;
  float* O = out + (size_t)b * G * C;
  // three 16-byte stores per group of four xyz-only points where the rows allow it (wave-uniform)
  const bool vec = C == 3 && (G & 3) == 0 && (((uintptr_t)out) & 15) == 0;
  const int groups = (G + 3) >> 2;
  for (int grp = tid; grp < groups; grp += PCA_THREADS) {
    const U4 w = philox4x32_10(U4{(uint32_t)grp, 0u, 0u, 0u}, k0, k1);
    const uint32_t word[4] = {w.x, w.y, w.z, w.w};
    float o[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = grp * 4 + j;
      float x = 0.f, y = 0.f, z = 0.f;
      if (g < G) {
        const float u = (float)(word[j] >> 8) * 5.9604644775390625e-8f;      // 2^-24: u in [0, 1), exact in fp32
        if (u <= pr.drop_ratio) { x = x0; y = y0; z = z0; }                    // the reference's <=
        else normalised(g, x, y, z);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c)
        o[j * 3 + c] = fmaf(x, pr.A[c], fmaf(y, pr.A[3 + c], fmaf(z, pr.A[6 + c], pr.t[c])));
    }
    if (vec) {
      f32x4* dst = (f32x4*)(O + (size_t)grp * 12);
      dst[0] = f32x4{o[0], o[1], o[2], o[3]};
      dst[1] = f32x4{o[4], o[5], o[6], o[7]};
      dst[2] = f32x4{o[8], o[9], o[10], o[11]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int g = grp * 4 + j;
        if (g >= G) break;
        float* d = O + (size_t)g * C;
        d[0] = o[j * 3]; d[1] = o[j * 3 + 1]; d[2] = o[j * 3 + 2];
        if (C > 3) {
          const float* r = row(g);
          for (int c = 3; c < C; ++c) d[c] = fill ? feat_fill : r[c];
        }
      }
    }
  }
}

}  // namespace

extern "C" int vl_set_error(const char* msg);

extern "C" int vl_pc_augment(const float* pts, const int64_t* idx, float* out, int B, int N, int G, int C, const void* params,
                             float feat_fill, hipStream_t stream) {
  if (B <= 0 || N <= 0 || G <= 0 || C < 3 || C > 8) return vl_set_error("vl_pc_augment: bad shape (B, N, G >= 1, 3 <= C <= 8)");
  if (!pts || !out || !params) return vl_set_error("vl_pc_augment: null operand");
  if (!idx && G != N) return vl_set_error("vl_pc_augment: without an index list G must equal N");
  if (pts == out) return vl_set_error("vl_pc_augment: out of place (a dropped point reads point 0)");
  if ((((uintptr_t)params) & 7) != 0) return vl_set_error("vl_pc_augment: the parameter records must be 8-byte aligned");
  const PcAugParams* pr = (const PcAugParams*)params;
  if (G <= PCA_LDS_POINTS) {
    static const hipError_t attr = hipFuncSetAttribute((const void*)pc_augment_kernel<true>,
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, PCA_LDS_POINTS * 12);
    if (attr != hipSuccess) return vl_set_error(hipGetErrorString(attr));
    const size_t smem = (size_t)((G + 3) / 4) * 48;
    hipLaunchKernelGGL(pc_augment_kernel<true>, dim3(B), dim3(PCA_THREADS), smem, stream, pts, idx, out, N, G, C, pr, feat_fill);
  } else {
    hipLaunchKernelGGL(pc_augment_kernel<false>, dim3(B), dim3(PCA_THREADS), 0, stream, pts, idx, out, N, G, C, pr, feat_fill);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}
