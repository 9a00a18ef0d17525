// Row-wise backward kernels + optimizer for the trainable part of the path (HBM-bound, wave-per-row).
//   vl_layernorm_bwd      dx = LN'(dy) (+ upstream residual gradient), f32 and optional bf16 copy
//   (the LayerNorm parameter gradients and the bias gradients - column reductions over the rows - are vl_colreduce.hip)
//   vl_gelu_bf16          y = gelu(u)                                       (recompute of the MLP hidden)
//   vl_adamw_step         torch.optim.AdamW update (decoupled weight decay), one launch per tensor
//   vl_sumsq_f32          squared 2-norm of the flat gradient buffer: two stages, fp64 partials, bit-reproducible
//   vl_adamw_multi_step   the same update on a device table of tensors in ONE launch, with clip_grad_norm_'s coefficient
//   vl_adamw_multi_step_groups   the same launch with a learning-rate scale per tensor and tensors exempt from clipping
//                         derived on the device from that squared norm (training/train.py: --grad-clip-norm)
//   vl_clamp_scalar       logit_scale.clamp_(0, ln 100)   (training/train.py:248-249)
// Autograd counterparts of open_clip/transformer.py:17-34 (LayerNorm), :226-234 (MLP) and of
// `optim.AdamW` as configured in training/depth/depth_tri_main.py:394-419.
#include "vl_common.h"
#include "vitlens_hip.h"

namespace {

__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16_t* p) { return bf2f(*p); }

__device__ __forceinline__ void ld4(const float* p, float (&v)[4]) {
  const f32x4 t = *(const f32x4*)p; v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
}
__device__ __forceinline__ void ld4(const bf16_t* p, float (&v)[4]) {
  const u32x2 t = *(const u32x2*)p;
  v[0] = bf2f((bf16_t)(t[0] & 0xffff)); v[1] = bf2f((bf16_t)(t[0] >> 16));
  v[2] = bf2f((bf16_t)(t[1] & 0xffff)); v[3] = bf2f((bf16_t)(t[1] >> 16));
}
__device__ __forceinline__ void st4(float* p, const float (&v)[4]) { f32x4 t = {v[0], v[1], v[2], v[3]}; *(f32x4*)p = t; }
__device__ __forceinline__ void st4(bf16_t* p, const float (&v)[4]) {
  u32x2 t; t[0] = pack2bf(v[0], v[1]); t[1] = pack2bf(v[2], v[3]); *(u32x2*)p = t;
}

struct LnBwdP {
  const void* dy; const void* x; const float* mean; const float* rstd; const float* w;
  const void* dres;       // optional upstream gradient of the residual stream (added to dx), gradient-stream dtype
  void* dx; bf16_t* dxb;  // outputs: dx in the gradient-stream dtype (may alias dres), optional bf16 copy
  long dys, xs, dxs;      // row strides
  int rows, D;
  // sparse residual gradient (dres_every > 1): only the rows r = i * dres_every have one, row i of dres (row stride dres_s);
  // every other row's upstream residual gradient is zero and nothing is read for it.  dres_every <= 1: one per row, stride dxs.
  int dres_every; long dres_s;
};

// One wave per row.  NCH > 0: the row (D = NCH*256 elements) is read ONCE into registers with 8/16-byte accesses;
// NCH == 0: any D, two passes over global memory.  TG = dtype of the residual-gradient stream (dres / dx).
// HALF: D = NCH*256 + 128 (1408 = 5*256 + 128, the EVA ViT-g width): lanes 0-31 hold four more elements each, lanes 32-63 hold
// zeros there, which add nothing to either wave sum, and store nothing.
template <int NCH, typename TDY, typename TX, typename TG, bool HALF = false>
__global__ void __launch_bounds__(256) ln_bwd_kernel(const LnBwdP p) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.rows) return;
  const TDY* dy = (const TDY*)p.dy + (long)row * p.dys;
  const TX* x = (const TX*)p.x + (long)row * p.xs;
  const TG* dres = nullptr;
  if (p.dres) {
    if (p.dres_every <= 1) dres = (const TG*)p.dres + (long)row * p.dxs;
    else if (row % p.dres_every == 0) dres = (const TG*)p.dres + (long)(row / p.dres_every) * p.dres_s;
  }
  TG* dx = p.dx ? (TG*)p.dx + (long)row * p.dxs : nullptr;
  bf16_t* dxb = p.dxb ? p.dxb + (long)row * p.dxs : nullptr;
  const float mu = p.mean[row], rs = p.rstd[row];
  const int D = p.D;
  if constexpr (NCH > 0) {
    constexpr int NV = NCH + (HALF ? 1 : 0);
    const bool tail = lane < 32;      // HALF: this lane owns four elements of the half chunk
    float g[NV][4], xh[NV][4];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const int e = c * 256 + lane * 4;
      if (HALF && c == NCH && !tail) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { g[c][k] = 0.f; xh[c][k] = 0.f; }
        continue;
      }
      float ww[4];
      ld4(dy + e, g[c]); ld4(x + e, xh[c]); ld4(p.w + e, ww);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g[c][k] *= ww[k]; xh[c][k] = (xh[c][k] - mu) * rs;
        s1 += g[c][k]; s2 = fmaf(g[c][k], xh[c][k], s2);
      }
    }
    s1 = wave_sum(s1) / (float)D; s2 = wave_sum(s2) / (float)D;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      if (HALF && c == NCH && !tail) break;
      const int e = c * 256 + lane * 4;
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = rs * (g[c][k] - s1 - xh[c][k] * s2);
      if (dres) {
        float r[4]; ld4(dres + e, r);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += r[k];
      }
      if (dx) st4(dx + e, v);
      if (dxb) st4(dxb + e, v);
    }
  } else {
    float s1 = 0.f, s2 = 0.f;
    for (int e = lane; e < D; e += 64) {
      const float g = ld1(dy + e) * p.w[e];
      const float xh = (ld1(x + e) - mu) * rs;
      s1 += g; s2 = fmaf(g, xh, s2);
    }
    s1 = wave_sum(s1) / (float)D; s2 = wave_sum(s2) / (float)D;
    for (int e = lane; e < D; e += 64) {
      const float g = ld1(dy + e) * p.w[e];
      const float xh = (ld1(x + e) - mu) * rs;
      float v = rs * (g - s1 - xh * s2);
      if (dres) v += ld1(dres + e);
      if (dx) { if constexpr (sizeof(TG) == 4) dx[e] = v; else dx[e] = f2bf(v); }
      if (dxb) dxb[e] = f2bf(v);
    }
  }
}

__global__ void __launch_bounds__(256) gelu_kernel(const bf16_t* u, bf16_t* y, long n) {
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8; i < n; i += (long)gridDim.x * 256 * 8) {
    const u32x4 v = *(const u32x4*)(u + i);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      o[e] = pack2bf(gelu_erf(bf2f((bf16_t)(v[e] & 0xffff))), gelu_erf(bf2f((bf16_t)(v[e] >> 16))));
    *(u32x4*)(y + i) = o;
  }
}

__global__ void __launch_bounds__(256) geglu_kernel(const bf16_t* h, bf16_t* y, long n) {
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long)gridDim.x * 256 * 4) {
    const u32x4 v = *(const u32x4*)(h + 2 * i);
    u32x2 o;
    o[0] = pack2bf(bf2f((bf16_t)(v[0] & 0xffff)) * gelu_erf(bf2f((bf16_t)(v[0] >> 16))),
                   bf2f((bf16_t)(v[1] & 0xffff)) * gelu_erf(bf2f((bf16_t)(v[1] >> 16))));
    o[1] = pack2bf(bf2f((bf16_t)(v[2] & 0xffff)) * gelu_erf(bf2f((bf16_t)(v[2] >> 16))),
                   bf2f((bf16_t)(v[3] & 0xffff)) * gelu_erf(bf2f((bf16_t)(v[3] >> 16))));
    *(u32x2*)(y + i) = o;
  }
}

// AdamW (PyTorch semantics): p *= 1 - lr*wd ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ;
//                            p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
// The update of ONE element, shared by the per-tensor and the multi-tensor kernel.  Which products the compiler fuses into
// an fma depends on the code around the expression, so the roundings are spelled out - the ones adamw_kernel has always had
// (1 - lr*wd and the first moment fused, everything else rounded per operation) - and contraction is off in here: both
// kernels produce the same bits from the same inputs.
struct AdamwC { float lr, b1, b2, eps, bc1, bc2_sqrt; };
__device__ __forceinline__ void adamw_update(float& pi, const float gi, float& mi, float& vi, const AdamwC c, const float wd) {
#pragma clang fp contract(off)
  const float decay = fmaf(-c.lr, wd, 1.0f);
  mi = fmaf(1.0f - c.b1, gi, c.b1 * mi);
  vi = c.b2 * vi + ((1.0f - c.b2) * gi) * gi;
  pi = pi * decay - ((c.lr / c.bc1) * mi) / (sqrtf(vi) / c.bc2_sqrt + c.eps);
}

__global__ void __launch_bounds__(256) adamw_kernel(float* p, const float* g, float* m, float* v, long n, float lr, float b1,
                                                    float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale) {
  const AdamwC c{lr, b1, b2, eps, bc1, bc2_sqrt};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_update(pi, g[i] * gscale, mi, vi, c, wd);
    m[i] = mi; v[i] = vi;
    p[i] = pi;
  }
}

// ---- global gradient norm: sum of squares in two stages, fixed grid, fixed combination order (no atomics) ----
constexpr int kSumsqMaxBlocks = 2048;          // partials = workspace doubles
constexpr int kSumsqPerBlock = 256 * 16;       // elements a workgroup takes per sweep of the grid (4 x 16 bytes per thread)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the 256 threads of a workgroup, the same order every time; valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v) {
  __shared__ double sh[4];
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// x[0:head) scalar (up to the first 16-byte boundary), the aligned body in 16-byte loads, the last n4 % 4 elements scalar.
// Squares are exact in fp64 and a thread's accumulators are fp64: the result is the fp64 sum, rounded to fp32 once.
__global__ void __launch_bounds__(256) sumsq_partial_kernel(const float* x, long n, double* part) {
  const long head = min(n, (long)((4 - (((uintptr_t)x >> 2) & 3)) & 3));
  const f32x4* x4 = (const f32x4*)(x + head);
  const long n4 = (n - head) >> 2;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  const long stride = (long)gridDim.x * 1024;
  for (long base = (long)blockIdx.x * 1024; base < n4; base += stride) {
    const long i = base + threadIdx.x;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 t0, t1, t2, t3;
    if (base + 1024 <= n4) {          // (workgroup-uniform)
      t0 = x4[i]; t1 = x4[i + 256]; t2 = x4[i + 512]; t3 = x4[i + 768];
    } else {                          // the one ragged span at the end of the body
      t0 = i < n4 ? x4[i] : z; t1 = i + 256 < n4 ? x4[i + 256] : z;
      t2 = i + 512 < n4 ? x4[i + 512] : z; t3 = i + 768 < n4 ? x4[i + 768] : z;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a0 = fma((double)t0[e], (double)t0[e], a0); a1 = fma((double)t1[e], (double)t1[e], a1);
      a2 = fma((double)t2[e], (double)t2[e], a2); a3 = fma((double)t3[e], (double)t3[e], a3);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) {          // head and tail: fewer than 4 elements each
    const long t = threadIdx.x < 4 ? threadIdx.x : head + n4 * 4 + (threadIdx.x - 4);
    const bool live = threadIdx.x < 4 ? t < head : t < n;
    if (live) a1 = fma((double)x[t], (double)x[t], a1);
  }
  const double s = block_sum_f64((a0 + a1) + (a2 + a3));
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) sumsq_final_kernel(const double* part, int nparts, float* out) {
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) a += part[i];
  const double s = block_sum_f64(a);
  if (threadIdx.x == 0) out[0] = (float)s;
}

// ---- AdamW on a table of tensors in one launch, clip_grad_norm_'s coefficient derived from the device-side squared norm ----
constexpr int kAdamTile = 2048;          // elements per tile: 256 threads x 2 x 16 bytes

// clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1); a NaN norm stays NaN (fminf would drop it)
__device__ __forceinline__ float clip_coef(const float norm, const float max_norm) {
  const float c = max_norm / (norm + 1e-6f);
  return c > 1.0f ? 1.0f : c;
}

// GROUPS (vl_adamw_multi_step_groups): slot s steps with lr * groups[s].lr_scale, and a slot with groups[s].no_clip set sees
// coef = 1 - read per slot beside weight_decay.  lr * 1.0f is lr, so a table of ones with no exempt slot gives the bits of the
// instantiation without groups, which compiles from the same source as before.
template <bool GROUPS>
__global__ void __launch_bounds__(256) adamw_multi_kernel(const vl_adamw_slot* slots, const vl_adamw_group* groups, int nslots,
                                                          AdamwC c, float gscale, float max_norm, const float* sumsq,
                                                          float* norm_out) {
  // first[s] = index of slot s's first tile; wave 0 scans the tile counts (16 consecutive slots per lane)
  __shared__ int first[VL_ADAMW_MAX_SLOTS + 1];
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    int cnt[16], sum = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int s = lane * 16 + k;
      cnt[k] = s < nslots ? (int)((slots[s].n + kAdamTile - 1) / kAdamTile) : 0;
      sum += cnt[k];
    }
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    int run = incl - sum;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int s = lane * 16 + k;
      if (s < nslots) first[s] = run;
      run += cnt[k];
    }
    if (lane == 63) first[nslots] = incl;
  }
  __syncthreads();
  const int ntiles = first[nslots];
  const float norm = gscale * sqrtf(sumsq[0]);
  const float gmul = clip_coef(norm, max_norm);
  if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int lo = 0, hi = nslots - 1;          // the last slot whose first tile is <= tile (empty slots own no tile)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (first[mid] <= tile) lo = mid; else hi = mid - 1;
    }
    const vl_adamw_slot S = slots[lo];
    const long base = (long)(tile - first[lo]) * kAdamTile;
    const int cntE = (int)min((long)kAdamTile, S.n - base);
    float* p = S.p + base; const float* g = S.g + base; float* m = S.m + base; float* v = S.v + base;
    const float wd = S.weight_decay;
    AdamwC cs = c;
    float gm = gmul;
    if (GROUPS) {
      const vl_adamw_group G = groups[lo];
      cs.lr = c.lr * G.lr_scale;
      if (G.no_clip) gm = 1.0f;
    }
    const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
    const int nvec = vec ? (cntE >> 2) : 0;
    for (int i = threadIdx.x; i < nvec; i += 256) {
      f32x4 pp = ((f32x4*)p)[i], mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
      const f32x4 gg = ((const f32x4*)g)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pp[e], me = mm[e], ve = vv[e];
        adamw_update(pe, gg[e] * gscale * gm, me, ve, cs, wd);
        pp[e] = pe; mm[e] = me; vv[e] = ve;
      }
      ((f32x4*)m)[i] = mm; ((f32x4*)v)[i] = vv; ((f32x4*)p)[i] = pp;
    }
    for (int i = nvec * 4 + threadIdx.x; i < cntE; i += 256) {
      float pe = p[i], me = m[i], ve = v[i];
      adamw_update(pe, g[i] * gscale * gm, me, ve, cs, wd);
      m[i] = me; v[i] = ve; p[i] = pe;
    }
  }
}

// (fminf / fmaxf return the other operand for a NaN: a diverged logit_scale would come out as lo.  torch.clamp_ keeps the NaN)
__global__ void clamp_scalar_kernel(float* p, float lo, float hi) { const float v = *p; *p = v != v ? v : fminf(fmaxf(v, lo), hi); }

// p[i] = value: the accumulators of a step (loss terms, hit counters - the bits of 0.0f are those of int 0) start from zero
__global__ void __launch_bounds__(256) fill_kernel(float* p, float value, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] = value;
}

// out[i] = a[i] + b[i] (f32), used to merge gradient contributions of shared tensors
__global__ void __launch_bounds__(256) axpy_kernel(float* y, const float* x, float alpha, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = fmaf(alpha, x[i], y[i]);
}

// out[i] = x[i] * exp(*log_scale) * mul: the learnable temperature applied ON THE DEVICE (model.py:619 `logit_scale.exp()`):
// the step never reads the scalar on the host
__global__ void __launch_bounds__(256) scale_exp_kernel(const float* x, float* out, long n, const float* log_scale, float mul) {
  const float s = __expf(log_scale[0]) * mul;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = x[i] * s;
}

// rows -> sum over the batch index: out[t, :] += sum_b x[(b*T_stride + t_off + t), :]   (pos-embedding grads)
__global__ void __launch_bounds__(256) batch_rowsum_kernel(const float* x, float* out, int B, int T, int D, long bstride, long toff) {
  const long n = (long)T * D;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long t = i / D; const int d = (int)(i - t * D);
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += x[((long)b * bstride + toff + t) * D + d];
    out[i] += s;
  }
}

}  // namespace

extern "C" int vl_set_error(const char* msg);
#define VL_HIP_OK(e) do { hipError_t _e = (e); if (_e != hipSuccess) return vl_set_error(hipGetErrorString(_e)); } while (0)
static int grid_for(long n) { long g = (n + 255) / 256; return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g)); }

template <typename TDY, typename TX, typename TG>
static void ln_bwd_launch(const LnBwdP& p, hipStream_t stream) {
  const dim3 g((p.rows + 3) / 4), b(256);
  // the register forms read and write every operand four elements (8 or 16 bytes) at a time: the strides AND the bases must be
  // multiples of that (the column reductions' rule, vl_colreduce.hip), the sparse residual's own stride included
  auto al4 = [](const void* q, size_t elem) { return (uintptr_t)q % (4 * elem) == 0; };      // a null (absent) operand passes
  const bool al = (p.dys % 4 == 0) && (p.xs % 4 == 0) && (p.dxs % 4 == 0) &&
                   (!(p.dres && p.dres_every > 1) || p.dres_s % 4 == 0) && al4(p.dy, sizeof(TDY)) && al4(p.x, sizeof(TX)) &&
                   al4(p.w, 4) && al4(p.dres, sizeof(TG)) && al4(p.dx, sizeof(TG)) && al4(p.dxb, 2);
  const bool vec = al && (p.D % 256 == 0);
  if (al && p.D == 1408) hipLaunchKernelGGL((ln_bwd_kernel<5, TDY, TX, TG, true>), g, b, 0, stream, p);    // 5*256 + 128: EVA ViT-g
  else if (vec && p.D == 1024) hipLaunchKernelGGL((ln_bwd_kernel<4, TDY, TX, TG>), g, b, 0, stream, p);
  else if (vec && p.D == 768) hipLaunchKernelGGL((ln_bwd_kernel<3, TDY, TX, TG>), g, b, 0, stream, p);
  else if (vec && p.D == 512) hipLaunchKernelGGL((ln_bwd_kernel<2, TDY, TX, TG>), g, b, 0, stream, p);
  else if (vec && p.D == 256) hipLaunchKernelGGL((ln_bwd_kernel<1, TDY, TX, TG>), g, b, 0, stream, p);
  else hipLaunchKernelGGL((ln_bwd_kernel<0, TDY, TX, TG>), g, b, 0, stream, p);
}

static int ln_bwd_run(const void* dy, int dy_dtype, long dy_stride, const void* x, int x_dtype, long x_stride,
                      const float* mean, const float* rstd, const float* w, const void* dres, int dres_every, long dres_stride,
                      void* dx, int g_dtype, void* dx_bf16, long dx_stride, int rows, int D, hipStream_t stream) {
  if (rows <= 0 || D <= 0) return vl_set_error("vl_layernorm_bwd: empty problem");
  for (const int dt : {dy_dtype, x_dtype, g_dtype})
    if (dt != VL_F32 && dt != VL_BF16) return vl_set_error("vl_layernorm_bwd: dy_dtype, x_dtype and g_dtype must be VL_F32 or VL_BF16");
  LnBwdP p{dy, x, mean, rstd, w, dres, dx, (bf16_t*)dx_bf16, dy_stride, x_stride, dx_stride, rows, D, dres_every, dres_stride};
  const int key = (dy_dtype == VL_BF16 ? 4 : 0) | (x_dtype == VL_BF16 ? 2 : 0) | (g_dtype == VL_BF16 ? 1 : 0);
  switch (key) {
    case 0: ln_bwd_launch<float, float, float>(p, stream); break;
    case 1: ln_bwd_launch<float, float, bf16_t>(p, stream); break;
    case 2: ln_bwd_launch<float, bf16_t, float>(p, stream); break;
    case 3: ln_bwd_launch<float, bf16_t, bf16_t>(p, stream); break;
    case 4: ln_bwd_launch<bf16_t, float, float>(p, stream); break;
    case 5: ln_bwd_launch<bf16_t, float, bf16_t>(p, stream); break;
    case 6: ln_bwd_launch<bf16_t, bf16_t, float>(p, stream); break;
    default: ln_bwd_launch<bf16_t, bf16_t, bf16_t>(p, stream); break;
  }
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int vl_layernorm_bwd_g(const void* dy, int dy_dtype, long dy_stride, const void* x, int x_dtype, long x_stride,
                                  const float* mean, const float* rstd, const float* w, const void* dres, void* dx, int g_dtype,
                                  void* dx_bf16, long dx_stride, int rows, int D, hipStream_t stream) {
  return ln_bwd_run(dy, dy_dtype, dy_stride, x, x_dtype, x_stride, mean, rstd, w, dres, 1, dx_stride, dx, g_dtype, dx_bf16, dx_stride,
                    rows, D, stream);
}

// vl_layernorm_bwd_g whose upstream residual gradient exists on every dres_every-th row only (the class-token rows behind a
// block that ran on those rows alone): row i * dres_every adds row i of dres (row stride dres_stride), every other row adds
// nothing.  dx is written for ALL rows, so the caller needs no zero-filled residual-gradient buffer; dres must not alias dx.
extern "C" int vl_layernorm_bwd_sres(const void* dy, int dy_dtype, long dy_stride, const void* x, int x_dtype, long x_stride,
                                     const float* mean, const float* rstd, const float* w, const void* dres, int dres_every,
                                     long dres_stride, void* dx, int g_dtype, void* dx_bf16, long dx_stride, int rows, int D,
                                     hipStream_t stream) {
  if (!dres || !dx || dres_every < 1) return vl_set_error("vl_layernorm_bwd_sres: dres, dx and dres_every >= 1 are required");
  if (dres == dx) return vl_set_error("vl_layernorm_bwd_sres: dres must not alias dx");
  return ln_bwd_run(dy, dy_dtype, dy_stride, x, x_dtype, x_stride, mean, rstd, w, dres, dres_every, dres_stride, dx, g_dtype, dx_bf16,
                    dx_stride, rows, D, stream);
}

extern "C" int vl_layernorm_bwd(const void* dy, int dy_dtype, long dy_stride, const void* x, int x_dtype, long x_stride,
                                const float* mean, const float* rstd, const float* w, const float* dres, float* dx,
                                void* dx_bf16, long dx_stride, int rows, int D, hipStream_t stream) {
  return vl_layernorm_bwd_g(dy, dy_dtype, dy_stride, x, x_dtype, x_stride, mean, rstd, w, dres, dx, VL_F32, dx_bf16, dx_stride, rows, D, stream);
}

extern "C" int vl_gelu_bf16(const void* u, void* y, long n, hipStream_t stream) {
  if (n <= 0) return 0;
  if (n & 7) return vl_set_error("vl_gelu_bf16: n must be a multiple of 8");
  hipLaunchKernelGGL(gelu_kernel, dim3(grid_for(n / 8)), dim3(256), 0, stream, (const bf16_t*)u, (bf16_t*)y, n);
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int vl_geglu_bf16(const void* h, void* y, long rows, int n_out, hipStream_t stream) {
  const long n = rows * n_out;
  if (n <= 0) return 0;
  if (n_out & 3) return vl_set_error("vl_geglu_bf16: n_out must be a multiple of 4");
  hipLaunchKernelGGL(geglu_kernel, dim3(grid_for(n / 4)), dim3(256), 0, stream, (const bf16_t*)h, (bf16_t*)y, n);
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int vl_adamw_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                             float eps, float weight_decay, int step, float grad_scale, hipStream_t stream) {
  if (n <= 0) return 0;
  if (step < 1) return vl_set_error("vl_adamw_step: step counts from 1");
  const float bc1 = 1.0f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.0f - powf(beta2, (float)step));
  hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(n)), dim3(256), 0, stream, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay,
                     bc1, bc2s, grad_scale);
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" long vl_sumsq_ws_floats(void) { return 2L * kSumsqMaxBlocks; }

extern "C" int vl_sumsq_f32(const float* x, long n, float* out, float* ws, hipStream_t stream) {
  if (n < 0) return vl_set_error("vl_sumsq_f32: negative n");
  if (!out || !ws || (n > 0 && !x)) return vl_set_error("vl_sumsq_f32: null argument");
  if (((uintptr_t)x & 3) || ((uintptr_t)out & 3)) return vl_set_error("vl_sumsq_f32: x and out must be 4-byte aligned");
  if ((uintptr_t)ws & 7) return vl_set_error("vl_sumsq_f32: workspace of vl_sumsq_ws_floats() floats, 8-byte aligned, required");
  // one workgroup per 4096 elements up to the cap: the grid, and with it the order of the sum, depends on n alone
  const long want = (n / 4 + 1023) / 1024;
  const int nb = (int)(want > kSumsqMaxBlocks ? kSumsqMaxBlocks : (want < 1 ? 1 : want));
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb), dim3(256), 0, stream, x, n, (double*)ws);
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)ws, nb, out);
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int vl_adamw_multi_step(const vl_adamw_slot* slots, int nslots, float lr, float beta1, float beta2, float eps, int step,
                                   float grad_scale, float max_norm, const float* sumsq, float* norm_out, hipStream_t stream) {
  if (nslots < 0 || nslots > VL_ADAMW_MAX_SLOTS) return vl_set_error("vl_adamw_multi_step: 0 <= nslots <= VL_ADAMW_MAX_SLOTS");
  if (step < 1) return vl_set_error("vl_adamw_multi_step: step counts from 1");
  if (!(max_norm > 0.0f)) return vl_set_error("vl_adamw_multi_step: max_norm must be positive");
  if (!sumsq || (nslots > 0 && !slots)) return vl_set_error("vl_adamw_multi_step: null argument");
  if (nslots == 0) return 0;
  const AdamwC c{lr, beta1, beta2, eps, 1.0f - powf(beta1, (float)step), sqrtf(1.0f - powf(beta2, (float)step))};
  // the table lives on the device: the grid cannot follow the element count, the tiles are dealt round-robin to 2048 workgroups
  hipLaunchKernelGGL(adamw_multi_kernel<false>, dim3(2048), dim3(256), 0, stream, slots, (const vl_adamw_group*)nullptr, nslots, c,
                     grad_scale, max_norm, sumsq, norm_out);
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int vl_adamw_multi_step_groups(const vl_adamw_slot* slots, const vl_adamw_group* groups,
                                          const vl_adamw_group* groups_host, int nslots, float lr, float beta1, float beta2,
                                          float eps, int step, float grad_scale, float max_norm, const float* sumsq,
                                          float* norm_out, hipStream_t stream) {
  if (nslots < 0 || nslots > VL_ADAMW_MAX_SLOTS) return vl_set_error("vl_adamw_multi_step_groups: 0 <= nslots <= VL_ADAMW_MAX_SLOTS");
  if (step < 1) return vl_set_error("vl_adamw_multi_step_groups: step counts from 1");
  if (!(max_norm > 0.0f)) return vl_set_error("vl_adamw_multi_step_groups: max_norm must be positive");
  if (!sumsq || (nslots > 0 && (!slots || !groups || !groups_host))) return vl_set_error("vl_adamw_multi_step_groups: null argument");
  // the table is checked on the host's copy of it: nothing on the device is read back
  for (int s = 0; s < nslots; ++s) {
    const float ls = groups_host[s].lr_scale;
    if (!(ls >= 0.0f) || std::isinf(ls)) return vl_set_error("vl_adamw_multi_step_groups: lr_scale must be finite and >= 0");
    if (groups_host[s].no_clip != 0 && groups_host[s].no_clip != 1)
      return vl_set_error("vl_adamw_multi_step_groups: no_clip is 0 or 1");
  }
  if (nslots == 0) return 0;
  const AdamwC c{lr, beta1, beta2, eps, 1.0f - powf(beta1, (float)step), sqrtf(1.0f - powf(beta2, (float)step))};
  hipLaunchKernelGGL(adamw_multi_kernel<true>, dim3(2048), dim3(256), 0, stream, slots, groups, nslots, c, grad_scale, max_norm,
                     sumsq, norm_out);
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int vl_clamp_scalar(float* p, float lo, float hi, hipStream_t stream) {
  hipLaunchKernelGGL(clamp_scalar_kernel, dim3(1), dim3(1), 0, stream, p, lo, hi);
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int vl_fill_f32(float* p, float value, long n, hipStream_t stream) {
  if (n < 0 || (n > 0 && !p)) return vl_set_error("vl_fill_f32: n >= 0 and a buffer");
  if (n == 0) return 0;
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n)), dim3(256), 0, stream, p, value, n);
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int vl_axpy_f32(float* y, const float* x, float alpha, long n, hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(axpy_kernel, dim3(grid_for(n)), dim3(256), 0, stream, y, x, alpha, n);
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int vl_scale_exp_f32(const float* x, float* out, long n, const float* log_scale, float mul, hipStream_t stream) {
  if (n <= 0) return 0;
  if (!x || !out || !log_scale) return vl_set_error("vl_scale_exp_f32: null argument");
  hipLaunchKernelGGL(scale_exp_kernel, dim3(grid_for(n)), dim3(256), 0, stream, x, out, n, log_scale, mul);
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int vl_batch_rowsum(const float* x, float* out, int B, int T, int D, long batch_stride_rows, long row_offset,
                               hipStream_t stream) {
  if (B <= 0 || T <= 0 || D <= 0) return vl_set_error("vl_batch_rowsum: empty problem");
  hipLaunchKernelGGL(batch_rowsum_kernel, dim3(grid_for((long)T * D)), dim3(256), 0, stream, x, out, B, T, D, batch_stride_rows, row_offset);
  VL_HIP_OK(hipGetLastError());
  return 0;
}
