// Deterministic two-stage column reductions over the token rows (no atomics; HBM-bound):
//   vl_layernorm_bwd_params   dw += sum_r dy*xhat, db += sum_r dy          (trainable LayerNorms only)
//   vl_colsum                 out[j] += scale * sum_r a[r,j]               (bias gradients)
// stage 1: block (column block, 256-row slab) -> partial sums ws[slab][plane][cols] (colreduce_kernel); stage 2: fixed-order sum
// over the slabs, += into the destinations (slab_finalize_kernel).  Autograd counterparts of the parameter gradients of
// open_clip/transformer.py:17-34 (LayerNorm) and of every bias.
#include "vl_common.h"
#include "vitlens_hip.h"

namespace {

// V columns of one row as floats: one 16-, 8- or 4-byte load for V > 1 (8 bf16, 4 f32, 4 bf16), one element for V == 1.
template <int V, typename T>
__device__ __forceinline__ void ldv(const T* p, float (&f)[V]) {
  constexpr bool kF32 = sizeof(T) == 4;
  static_assert(V == 1 || (kF32 ? V == 4 : V == 4 || V == 8), "no load of this width");
  if constexpr (V == 1) {
    if constexpr (kF32) f[0] = *p; else f[0] = bf2f(*p);
  } else if constexpr (kF32) {
    const f32x4 v = *(const f32x4*)p;
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = v[e];
  } else {
    typedef __attribute__((ext_vector_type(V / 2))) unsigned int words_t;
    const words_t v = *(const words_t*)p;
#pragma unroll
    for (int e = 0; e < V / 2; ++e) { f[2 * e] = bf2f((bf16_t)(v[e] & 0xffff)); f[2 * e + 1] = bf2f((bf16_t)(v[e] >> 16)); }
  }
}

// Stage 1.  A 256-thread block is 256/NR column groups of V columns x NR row lanes over one slab of rows: lane ry adds the rows
// r0+ry, r0+ry+NR, ... in increasing order, the loads of U of them issued before any is added; lanes 1..3 hand their sums to
// lane 0 through LDS (NR == 1: no LDS, no barrier).  LN: the LayerNorm pair, plane 0 = sum a*(x-mean[r])*rstd[r], plane 1 = sum a
// (a = dy); otherwise the plain column sum of a (x, mean, rstd unused).
// V > 1 needs V-element friendly rows (vec_ok below).  What the one-column-per-thread form (V = 1, NR = 1) gave on the shapes
// that have a vector form - it moves 128 or 256 bytes per wave load:
//   bf16 sum       [65 792, 4 096]  1.6 TB/s, 0.33 ms - more than both transposes of the path it stands beside
//   f32 sum        [65 536, 1 024]  2.3 TB/s, 116 us in the C4 step (the Perceiver's fp32 residual-gradient stream: to_out / FF w2)
//   bf16/bf16 LN   [65 792, 1 024]  2 TB/s, 132 us
//   bf16/f32 LN    [65 536, 1 024]  139 us (the Perceiver's LayerNorms: bf16 gradient of the normalised rows, fp32 residual stream;
//                                   its vector form is ln_bwd_params4_bf16_f32_kernel below, not an instantiation of this template)
template <int V, int NR, int U, bool LN, typename TA, typename TX>
__global__ void __launch_bounds__(256) colreduce_kernel(const TA* a, long lda, const TX* x, long xs, const float* mean,
                                                        const float* rstd, float* ws, int rows, int cols, int slab) {
  static_assert(NR == 1 || NR == 4, "the LDS combine below is written for four row lanes");
  constexpr int NC = 256 / NR, PL = LN ? 2 : 1;
  const int cx = threadIdx.x % NC, ry = NR > 1 ? threadIdx.x / NC : 0;      // (NR == 1: a row counter the compiler knows is uniform)
  const int j = (blockIdx.x * NC + cx) * V;
  const int r0 = blockIdx.y * slab, r1 = min(rows, r0 + slab);
  float s[PL][V];
#pragma unroll
  for (int k = 0; k < PL; ++k)
#pragma unroll
    for (int e = 0; e < V; ++e) s[k][e] = 0.f;
  auto add = [&](const float (&g)[V], const float (&xv)[V], float m, float rs) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if constexpr (LN) { s[0][e] = fmaf(g[e], (xv[e] - m) * rs, s[0][e]); s[1][e] += g[e]; }
      else s[0][e] += g[e];
    }
  };
  if (j < cols) {
    int r = r0 + ry;
    for (; r + (U - 1) * NR < r1; r += U * NR) {
      float g[U][V], xv[U][V], m[U], rs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ldv<V>(a + (long)(r + u * NR) * lda + j, g[u]);
        if constexpr (LN) { ldv<V>(x + (long)(r + u * NR) * xs + j, xv[u]); m[u] = mean[r + u * NR]; rs[u] = rstd[r + u * NR]; }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) add(g[u], xv[u], m[u], rs[u]);
    }
    if constexpr (U > 1) {
      for (; r < r1; r += NR) {
        float g[V], xv[V], m = 0.f, rs = 0.f;
        ldv<V>(a + (long)r * lda + j, g);
        if constexpr (LN) { ldv<V>(x + (long)r * xs + j, xv); m = mean[r]; rs = rstd[r]; }
        add(g, xv, m, rs);
      }
    }
  }
  float* out = ws + (long)blockIdx.y * PL * cols + j;
  if constexpr (NR > 1) {
    __shared__ float sh[NR - 1][NC][PL * V];
    if (ry) {
#pragma unroll
      for (int k = 0; k < PL; ++k)
#pragma unroll
        for (int e = 0; e < V; ++e) sh[ry - 1][cx][k * V + e] = s[k][e];
    }
    __syncthreads();
    if (ry == 0 && j < cols) {
#pragma unroll
      for (int k = 0; k < PL; ++k)
#pragma unroll
        for (int e = 0; e < V; ++e)
          out[(long)k * cols + e] = (s[k][e] + sh[0][cx][k * V + e]) + (sh[1][cx][k * V + e] + sh[2][cx][k * V + e]);
    }
  } else if (j < cols) {
#pragma unroll
    for (int k = 0; k < PL; ++k) out[(long)k * cols] = s[k][0];
  }
}

// colreduce_kernel<4, 4, 2, true, bf16_t, float> written out, and kept: the same sums in the same order (its short last batch adds
// the repeated row times zero instead of running a remainder loop), but on [65 536, 1 024] the template's instantiation took
// 0.6 - 0.9 % longer in four A/B sessions, at the edge of or beyond the parent's own spread (profiles/colreduce_ab.log: neither
// U = 4 nor another order of its loads closed the gap; one guarded loop in place of batch + remainder did, and cost the
// bf16 sum 16 %).  Same partial layout, same finalize.
__global__ void __launch_bounds__(256) ln_bwd_params4_bf16_f32_kernel(const bf16_t* dy, long dys, const float* x, long xs, const float* mean,
                                                                      const float* rstd, float* ws, int rows, int D, int slab) {
  __shared__ float sh[3][64][8];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int j = (blockIdx.x * 64 + cx) * 4;
  const int r0 = blockIdx.y * slab, r1 = min(rows, r0 + slab);
  float a[4], b[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { a[e] = 0.f; b[e] = 0.f; }
  if (j < D) {
    for (int r = r0 + ry; r < r1; r += 8) {
      const bool two = r + 4 < r1;
      const int r2 = two ? r + 4 : r;
      const u32x2 g0 = *(const u32x2*)(dy + (long)r * dys + j), g1 = *(const u32x2*)(dy + (long)r2 * dys + j);
      const f32x4 x0 = *(const f32x4*)(x + (long)r * xs + j), x1 = *(const f32x4*)(x + (long)r2 * xs + j);
      const float m0 = mean[r], s0 = rstd[r], m1 = mean[r2], s1 = two ? rstd[r2] : 0.f;
      const float k1 = two ? 1.f : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gl = bf2f((bf16_t)((e & 1) ? (g0[e >> 1] >> 16) : (g0[e >> 1] & 0xffff)));
        const float hl = bf2f((bf16_t)((e & 1) ? (g1[e >> 1] >> 16) : (g1[e >> 1] & 0xffff)));
        a[e] = fmaf(gl, (x0[e] - m0) * s0, a[e]);
        b[e] += gl;
        a[e] = fmaf(hl, (x1[e] - m1) * s1, a[e]);
        b[e] = fmaf(hl, k1, b[e]);
      }
    }
  }
  if (ry) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { sh[ry - 1][cx][e] = a[e]; sh[ry - 1][cx][4 + e] = b[e]; }
  }
  __syncthreads();
  if (ry == 0 && j < D) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ws[((long)blockIdx.y * 2) * D + j + e] = (a[e] + sh[0][cx][e]) + (sh[1][cx][e] + sh[2][cx][e]);
      ws[((long)blockIdx.y * 2 + 1) * D + j + e] = (b[e] + sh[0][cx][4 + e]) + (sh[1][cx][4 + e] + sh[2][cx][4 + e]);
    }
  }
}

// out_k[j] += scale * sum_s ws[s][k][j]   (k < K planes), fixed summation order.
// One block = 64 columns of one plane x 16 slab groups: thread (j, g) adds the slabs s = g, g+16, ... in order, the 16
// group sums are combined by a fixed tree through LDS.  (The first version gave every column ONE thread and the whole
// grid 4 blocks: 514 dependent loads per thread, 120 us per call = 4 ms of the C3 step.)
__global__ void __launch_bounds__(1024) slab_finalize_kernel(const float* ws, int nslab, int K, int D, float scale, float* out0, float* out1) {
  __shared__ float sh[16][64];
  const int jl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + jl, k = blockIdx.y;
  float s = 0.f;
  if (j < D)
    for (int t = g; t < nslab; t += 16) s += ws[((long)t * K + k) * D + j];
  sh[g][jl] = s;
  __syncthreads();
  if (g == 0 && j < D) {
    float a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = sh[i][jl];
#pragma unroll
    for (int w = 8; w > 0; w >>= 1)
#pragma unroll
      for (int i = 0; i < w; ++i) a[i] += a[i + w];
    float* o = k == 0 ? out0 : out1;
    o[j] += a[0] * scale;
  }
}

}  // namespace

extern "C" int vl_set_error(const char* msg);
#define VL_HIP_OK(e) do { hipError_t _e = (e); if (_e != hipSuccess) return vl_set_error(hipGetErrorString(_e)); } while (0)

static const int kSlabRows = 256;
extern "C" long vl_colreduce_ws_floats(int rows, int cols, int planes) {
  return (long)((rows + kSlabRows - 1) / kSlabRows) * planes * cols;
}

// V columns of T per thread are loadable: whole groups of V in a row, every row and the base on a V-element boundary.
template <typename T>
static bool vec_ok(int V, const void* p, long stride, int cols) {
  return cols % V == 0 && stride % V == 0 && (uintptr_t)p % (V * sizeof(T)) == 0;
}

template <int V, int NR, int U, bool LN, typename TA, typename TX>
static void stage1_launch(const void* a, long lda, const void* x, long xs, const float* mean, const float* rstd, float* ws,
                          int rows, int cols, int nslab, hipStream_t stream) {
  constexpr int per_block = 256 / NR * V;
  hipLaunchKernelGGL((colreduce_kernel<V, NR, U, LN, TA, TX>), dim3((cols + per_block - 1) / per_block, nslab), dim3(256), 0, stream,
                     (const TA*)a, lda, (const TX*)x, xs, mean, rstd, ws, rows, cols, kSlabRows);
}

// Both stages: out0[j] += scale * sum_r f(r, j) (and out1, the second plane of the LayerNorm pair).  V columns per thread on four
// row lanes where both operands allow it, else one column per thread (V == 1: always).  Four rows' loads in flight for the
// plain sums, two for the LayerNorm pairs.
template <int V, bool LN, typename TA, typename TX>
static void colreduce_launch(const void* a, long lda, const void* x, long xs, const float* mean, const float* rstd, float* ws,
                             int rows, int cols, float scale, float* out0, float* out1, hipStream_t stream) {
  const int nslab = (rows + kSlabRows - 1) / kSlabRows;
  bool vec = false;
  if constexpr (V > 1) {
    vec = vec_ok<TA>(V, a, lda, cols) && (!LN || vec_ok<TX>(V, x, xs, cols));
    if constexpr (LN && V == 4) {       // bf16 dy, fp32 x: the hand-written form (see there)
      if (vec)
        hipLaunchKernelGGL(ln_bwd_params4_bf16_f32_kernel, dim3((cols + 255) / 256, nslab), dim3(256), 0, stream, (const bf16_t*)a, lda,
                           (const float*)x, xs, mean, rstd, ws, rows, cols, kSlabRows);
    } else if (vec) {
      stage1_launch<V, 4, LN ? 2 : 4, LN, TA, TX>(a, lda, x, xs, mean, rstd, ws, rows, cols, nslab, stream);
    }
  }
  if (!vec) stage1_launch<1, 1, 1, LN, TA, TX>(a, lda, x, xs, mean, rstd, ws, rows, cols, nslab, stream);
  hipLaunchKernelGGL(slab_finalize_kernel, dim3((cols + 63) / 64, LN ? 2 : 1), dim3(1024), 0, stream, ws, nslab, LN ? 2 : 1, cols,
                     scale, out0, out1);
}

extern "C" int vl_layernorm_bwd_params(const void* dy, int dy_dtype, long dy_stride, const void* x, int x_dtype, long x_stride,
                                       const float* mean, const float* rstd, float* dw, float* db, int rows, int D,
                                       float* ws, hipStream_t stream) {
  if (rows <= 0 || D <= 0) return vl_set_error("vl_layernorm_bwd_params: empty problem");
  if (!ws) return vl_set_error("vl_layernorm_bwd_params: workspace of vl_colreduce_ws_floats(rows, D, 2) floats required");
#define VL_LN_PARAMS(V, TA, TX) colreduce_launch<V, true, TA, TX>(dy, dy_stride, x, x_stride, mean, rstd, ws, rows, D, 1.0f, dw, db, stream)
  if (dy_dtype == VL_BF16 && x_dtype == VL_F32) VL_LN_PARAMS(4, bf16_t, float);
  else if (dy_dtype == VL_BF16) VL_LN_PARAMS(8, bf16_t, bf16_t);
  else if (x_dtype == VL_F32) VL_LN_PARAMS(1, float, float);      // an fp32 dy has no vector form
  else VL_LN_PARAMS(1, float, bf16_t);
#undef VL_LN_PARAMS
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int vl_colsum(const void* a, int a_dtype, long lda, float* out, int rows, int cols, float scale, float* ws, hipStream_t stream) {
  if (rows <= 0 || cols <= 0) return vl_set_error("vl_colsum: empty problem");
  if (!ws) return vl_set_error("vl_colsum: workspace of vl_colreduce_ws_floats(rows, cols, 1) floats required");
  if (a_dtype == VL_BF16) colreduce_launch<8, false, bf16_t, bf16_t>(a, lda, nullptr, 0, nullptr, nullptr, ws, rows, cols, scale, out, out, stream);
  else colreduce_launch<4, false, float, float>(a, lda, nullptr, 0, nullptr, nullptr, ws, rows, cols, scale, out, out, stream);
  VL_HIP_OK(hipGetLastError());
  return 0;
}
