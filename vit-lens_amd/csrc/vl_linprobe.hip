// The linear probe (open_clip/linprobe_model.py ViTLensLP, training/optimizer.py LARS, training/zero_shot.py test_linprob_single):
// a frozen backbone's pooled feature -> Dropout -> BatchNorm1d(affine=False, eps=1e-6) -> Linear, trained with label
// cross-entropy and LARS.  The Linear is vl_gemm_f32 (forward and dW); the rest of the head is here, all true fp32 in and out
// with fp64 accumulators, every reduction in a fixed order (no floating-point atomics: two calls agree bit for bit).
//
//   vl_lp_bn_fwd        Dropout + batch statistics + normalisation (+ the transpose that makes dW one GEMM).  One workgroup
//                       owns a strip of 16 columns for ALL rows: 4 column quads x 64 row lanes, 16-byte loads.  Train: mean,
//                       then the sum of squared deviations (two passes - the columns come out of a LayerNorm and are far from
//                       centred), then the write; the strip's B x 64 bytes stay in L2 between the passes.
//   vl_ce_label         nn.CrossEntropyLoss() (mean) and its gradient.  Row statistics (one wave per row, any C), then 64 x 64
//                       tiles that write G coalesced, turn the tile through LDS for GT and leave the tile's column sums in the
//                       workspace, then one small launch that adds the row losses and the per-tile column sums in a fixed order.
//   vl_lars_multi_step  LARS on a device table of tensors: a launch that leaves each 2048-element tile's |p|^2 and |dp|^2 in
//                       fp64, and the update launch, where a workgroup adds the partials of its tile's tensor in a fixed order
//                       and derives the trust ratio itself - the host reads neither norm.
//   vl_topk_hits        rank of the target's logit within its row (one wave per row), integer adds only.
#include "vl_common.h"
#include "vl_philox.h"
#include "vitlens_hip.h"

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the 256 threads of a workgroup, the same value in every thread; `sh` holds 4 doubles
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  __syncthreads();                                     // (the previous use of sh is over)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- Dropout -> BatchNorm1d(affine=False) ------------------------------------------------------------------------------
constexpr int BN_STRIP = 16;          // columns per workgroup: 4 quads of 4

struct BnArgs {
  const float* x; long ldx;
  const uint8_t* keep; uint32_t thr; float scale; uint32_t k0, k1; uint64_t sample0; int drop;
  float* rmean; float* rvar; float momentum; float eps;
  float* xhat; long ldh; float* xhatT; long ldt; float* mean; float* var;
  int B, D;
};

// the row's 4 values of this thread's quad after dropout
__device__ __forceinline__ f32x4 bn_load(const BnArgs& a, int b, int d) {
  f32x4 v = *(const f32x4*)(a.x + (size_t)b * a.ldx + d);
  if (a.drop) {
    bool k[4];
    if (a.keep) {
      const uint32_t w = *(const uint32_t*)(a.keep + (size_t)b * a.D + d);          // D % 4 == 0, d % 4 == 0, base aligned
#pragma unroll
      for (int e = 0; e < 4; ++e) k[e] = ((w >> (8 * e)) & 0xffu) != 0;
    } else {
      const uint64_t s = a.sample0 + (uint64_t)b;
      const U4 r = philox4x32_10(U4{(uint32_t)(d >> 2), (uint32_t)s, (uint32_t)(s >> 32), 0u}, a.k0, a.k1);
      k[0] = r.x >= a.thr; k[1] = r.y >= a.thr; k[2] = r.z >= a.thr; k[3] = r.w >= a.thr;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k[e] ? v[e] * a.scale : 0.0f;
  }
  return v;
}

// sum over the 64 row lanes (threads with the same tid & 3) of 4 doubles per thread, in a fixed order; result in every thread
__device__ __forceinline__ void bn_reduce(double (&s)[4], double (*sh)[4][4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int o = 32; o >= 4; o >>= 1) s[e] += __shfl_xor(s[e], o, 64);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane < 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) sh[wave][lane][e] = s[e];
  }
  __syncthreads();
  const int q = threadIdx.x & 3;
#pragma unroll
  for (int e = 0; e < 4; ++e) s[e] = (sh[0][q][e] + sh[1][q][e]) + (sh[2][q][e] + sh[3][q][e]);
}

template <bool TRAIN>
__global__ void __launch_bounds__(256) lp_bn_kernel(const BnArgs a) {
  __shared__ double sh[4][4][4];
  const int q = threadIdx.x & 3, rl = threadIdx.x >> 2;
  const int d = blockIdx.x * BN_STRIP + q * 4;
  const bool live = d < a.D;                             // the last strip of a D that is no multiple of 16
  const int B = a.B;
  double mu[4], rs[4];
  if (TRAIN) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) for (int b = rl; b < B; b += 64) {
      const f32x4 v = bn_load(a, b, d);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += (double)v[e];
    }
    bn_reduce(s, sh);
#pragma unroll
    for (int e = 0; e < 4; ++e) { mu[e] = s[e] / (double)B; s[e] = 0.0; }
    if (live) for (int b = rl; b < B; b += 64) {
      const f32x4 v = bn_load(a, b, d);
#pragma unroll
      for (int e = 0; e < 4; ++e) { const double t = (double)v[e] - mu[e]; s[e] = fma(t, t, s[e]); }
    }
    bn_reduce(s, sh);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double var = s[e] / (double)B;
      rs[e] = 1.0 / sqrt(var + (double)a.eps);
      s[e] = var;
    }
    if (live && rl == 0) {
      const double m = (double)a.momentum, unb = (double)B / (double)(B - 1);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (a.mean) a.mean[d + e] = (float)mu[e];
        if (a.var) a.var[d + e] = (float)s[e];
        if (a.rmean) a.rmean[d + e] = (float)((1.0 - m) * (double)a.rmean[d + e] + m * mu[e]);
        if (a.rvar) a.rvar[d + e] = (float)((1.0 - m) * (double)a.rvar[d + e] + m * s[e] * unb);
      }
    }
  } else {
    if (live) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        mu[e] = (double)a.rmean[d + e];
        rs[e] = 1.0 / sqrt((double)a.rvar[d + e] + (double)a.eps);
      }
    }
  }
  if (!live) return;
  for (int b = rl; b < B; b += 64) {
    const f32x4 v = bn_load(a, b, d);
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = (float)(((double)v[e] - mu[e]) * rs[e]);
    *(f32x4*)(a.xhat + (size_t)b * a.ldh + d) = y;
    if (a.xhatT) {
#pragma unroll
      for (int e = 0; e < 4; ++e) a.xhatT[(size_t)(d + e) * a.ldt + b] = y[e];
    }
  }
  if (a.xhatT) {
    for (long b = (long)B + rl; b < a.ldt; b += 64) {
#pragma unroll
      for (int e = 0; e < 4; ++e) a.xhatT[(size_t)(d + e) * a.ldt + b] = 0.0f;
    }
  }
}

// ---- label cross-entropy ----------------------------------------------------------------------------------------------
// one wave per row: lse[b] and the row's loss term lse - logits[b, t] (NaN for a target outside [0, C))
__global__ void __launch_bounds__(256) ce_label_rows_kernel(const float* logits, long ld, const int64_t* target, int B, int C,
                                                            float* lse, float* rowloss) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* row = logits + (size_t)b * ld;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
  m = wave_max(m);
  double s = 0.0;
  for (int c = lane; c < C; c += 64) s += (double)expf(row[c] - m);
  s = wave_sum_d(s);
  if (lane == 0) {
    const int64_t t = target[b];
    const bool bad = t < 0 || t >= C;
    const int tc = bad ? 0 : (int)t;                     // clamped before the read
    const float l = m + (float)log(s);
    lse[b] = l;
    rowloss[b] = bad ? __builtin_nanf("") : l - row[tc];
  }
}

// 64 x 64 tile of G = gscale (softmax - onehot) / B: G coalesced along c, GT coalesced along b, the tile's column sums
__global__ void __launch_bounds__(256) ce_label_grad_kernel(const float* logits, long ld, const int64_t* target, int B, int C,
                                                            const float* lse, float mul, float* G, long ldg, float* GT,
                                                            long ldgt, float* part) {
  __shared__ float tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int c = c0 + tx;
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int rloc = ty + 4 * i, b = r0 + rloc;
    float g = 0.0f;
    if (b < B && c < C) {
      const int64_t t = target[b];
      const bool bad = t < 0 || t >= C;
      const float p = expf(logits[(size_t)b * ld + c] - lse[b]);
      g = bad ? __builtin_nanf("") : (p - (t == c ? 1.0f : 0.0f)) * mul;
      if (G) G[(size_t)b * ldg + c] = g;
    }
    tile[rloc][tx] = g;
  }
  __syncthreads();
  if (GT) {
    const bool last = r0 + 64 >= B;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int cloc = ty + 4 * i, cc = c0 + cloc;
      if (cc >= C) continue;
      float* o = GT + (size_t)cc * ldgt;
      const int b = r0 + tx;
      if (b < B) o[b] = tile[tx][cloc];
      if (last) for (long j = (long)B + tx; j < ldgt; j += 64) o[j] = 0.0f;          // zeros behind column B
    }
  }
  if (part && ty == 0 && c < C) {
    const int nr = min(64, B - r0);
    double s = 0.0;
    for (int r = 0; r < nr; ++r) s += (double)tile[r][tx];
    part[(size_t)blockIdx.y * C + c] = (float)s;
  }
}

// block 0: loss = mean of the row terms; blocks 1..: dbias[c] = sum over the row tiles of the column sums
__global__ void __launch_bounds__(256) ce_label_final_kernel(const float* rowloss, int B, float* loss, const float* part, int nbt,
                                                             int C, float* dbias) {
  __shared__ double sh[4];
  if (blockIdx.x == 0) {
    double s = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) s += (double)rowloss[b];
    s = block_sum_d(s, sh);
    if (threadIdx.x == 0) loss[0] = (float)(s / (double)B);
    return;
  }
  const int c = (blockIdx.x - 1) * 256 + threadIdx.x;
  if (!dbias || c >= C) return;
  double s = 0.0;
  for (int t = 0; t < nbt; ++t) s += (double)part[(size_t)t * C + c];
  dbias[c] = (float)s;
}

// ---- LARS ---------------------------------------------------------------------------------------------------------------
constexpr int kLarsTile = 2048;          // elements per tile: 256 threads x 2 x 16 bytes

// first[s] = index of slot s's first tile (wave 0 scans the tile counts, 16 consecutive slots per lane)
__device__ __forceinline__ void lars_scan(const vl_lars_slot* slots, int nslots, int* first) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    int cnt[16], sum = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int s = lane * 16 + k;
      cnt[k] = s < nslots ? (int)((slots[s].n + kLarsTile - 1) / kLarsTile) : 0;
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
}
__device__ __forceinline__ int lars_slot_of(const int* first, int nslots, int tile) {
  int lo = 0, hi = nslots - 1;          // the last slot whose first tile is <= tile (empty slots own no tile)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// clip_grad_norm_'s coefficient (vl_adamw_multi_step's): 1 without a max_norm
__device__ __forceinline__ float lars_clip(float gscale, float max_norm, const float* sumsq) {
  if (!(max_norm > 0.0f)) return 1.0f;
  const float c = max_norm / (gscale * sqrtf(sumsq[0]) + 1e-6f);
  return c > 1.0f ? 1.0f : c;
}
// The gradient the optimizer sees and the update direction of an adapted tensor (the two launches share these expressions),
// and the momentum update.  Contraction is off: every operation rounds to fp32 on its own, as the reference's separate torch
// calls do (hipcc would otherwise fuse the multiply into the add - the __f*_rn intrinsics are plain operators to it).
__device__ __forceinline__ float lars_g(float g, float gscale, float gmul) {
#pragma clang fp contract(off)
  return (g * gscale) * gmul;
}
__device__ __forceinline__ float lars_dp(float g1, float wd, float p) {
#pragma clang fp contract(off)
  const float t = wd * p;
  return g1 + t;
}
// mu = momentum mu + dp;  p -= lr mu
__device__ __forceinline__ void lars_apply(float& p, float& mu, float dp, float momentum, float lr) {
#pragma clang fp contract(off)
  const float a = momentum * mu;
  mu = a + dp;
  const float b = lr * mu;
  p = p - b;
}
__device__ __forceinline__ float lars_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

__global__ void __launch_bounds__(256) lars_norm_kernel(const vl_lars_slot* slots, int nslots, float gscale, float max_norm,
                                                        const float* sumsq, double* part, int cap) {
  __shared__ int first[VL_LARS_MAX_SLOTS + 1];
  __shared__ double sh[4];
  lars_scan(slots, nslots, first);
  const int ntiles = min(first[nslots], cap);
  const float gmul = lars_clip(gscale, max_norm, sumsq);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int si = lars_slot_of(first, nslots, tile);
    const vl_lars_slot S = slots[si];
    if (!S.adapt) continue;                              // (workgroup-uniform)
    const long base = (long)(tile - first[si]) * kLarsTile;
    const int cnt = (int)min((long)kLarsTile, S.n - base);
    const float* p = S.p + base; const float* g = S.g + base;
    double pp = 0.0, dd = 0.0;
    for (int i = threadIdx.x; i < cnt; i += 256) {
      const float pe = p[i], de = lars_dp(lars_g(g[i], gscale, gmul), S.weight_decay, pe);
      pp = fma((double)pe, (double)pe, pp);
      dd = fma((double)de, (double)de, dd);
    }
    pp = block_sum_d(pp, sh);
    dd = block_sum_d(dd, sh);
    if (threadIdx.x == 0) { part[2 * (size_t)tile] = pp; part[2 * (size_t)tile + 1] = dd; }
  }
}

__global__ void __launch_bounds__(256) lars_update_kernel(const vl_lars_slot* slots, int nslots, float lr, float momentum,
                                                          float trust, float gscale, float max_norm, const float* sumsq,
                                                          const double* part, int cap) {
  __shared__ int first[VL_LARS_MAX_SLOTS + 1];
  __shared__ double sh[4];
  lars_scan(slots, nslots, first);
  const int ntiles = min(first[nslots], cap);
  const float gmul = lars_clip(gscale, max_norm, sumsq);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int si = lars_slot_of(first, nslots, tile);
    const vl_lars_slot S = slots[si];
    float q = 1.0f;
    if (S.adapt) {                                       // the tensor's two norms: its tiles' partials in a fixed order
      const int t0 = first[si], t1 = min(first[si + 1], cap);
      double pp = 0.0, dd = 0.0;
      for (int t = t0 + threadIdx.x; t < t1; t += 256) { pp += part[2 * (size_t)t]; dd += part[2 * (size_t)t + 1]; }
      pp = block_sum_d(pp, sh);
      dd = block_sum_d(dd, sh);
      const double pn = sqrt(pp), dn = sqrt(dd);
      if (pn > 0.0 && dn > 0.0) q = (float)((double)trust * pn / dn);          // (a NaN norm compares false: q = 1, as torch.where)
    }
    const long base = (long)(tile - first[si]) * kLarsTile;
    const int cnt = (int)min((long)kLarsTile, S.n - base);
    float* p = S.p + base; const float* g = S.g + base; float* mu = S.mu + base;
    for (int i = threadIdx.x; i < cnt; i += 256) {
      const float pe = p[i];
      const float g1 = lars_g(g[i], gscale, gmul);
      const float dp = S.adapt ? lars_mul(lars_dp(g1, S.weight_decay, pe), q) : g1;
      float pn = pe, m = mu[i];
      lars_apply(pn, m, dp, momentum, lr);
      mu[i] = m;
      p[i] = pn;
    }
  }
}

// ---- top-k hits ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) topk_hits_kernel(const float* logits, long ld, const int64_t* target, int B, int C, int k0,
                                                        int k1, int* hits, uint8_t* correct) {
  __shared__ int sh[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long b = (long)blockIdx.x * 4 + wave;
  int h0 = 0, h1 = 0;
  if (b < B) {
    const float* row = logits + (size_t)b * ld;
    const int64_t t = target[b];
    const bool bad = t < 0 || t >= C;
    const int tc = bad ? 0 : (int)t;
    const float v = row[tc];
    int rank = 0;
    for (int c = lane; c < C; c += 64) {
      const float x = row[c];
      rank += (x > v) || (x == v && c < tc);             // a NaN compares false both ways
    }
    rank = wave_sum_i(rank);
    h0 = !bad && rank < k0;
    h1 = !bad && rank < k1;
    if (correct && lane == 0) { correct[2 * b] = (uint8_t)h0; correct[2 * b + 1] = (uint8_t)h1; }
  }
  if (lane == 0) { sh[wave][0] = h0; sh[wave][1] = h1; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int s = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
    if (s) atomicAdd(hits + threadIdx.x, s);
  }
}

}  // namespace

extern "C" int vl_set_error(const char* msg);

static int launched(void) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}

extern "C" int vl_lp_bn_fwd(const float* x, long ldx, const uint8_t* keep, float p, uint64_t seed, int64_t sample0, int train,
                            float* running_mean, float* running_var, float momentum, float eps, float* xhat, long ldh,
                            float* xhatT, long ldt, float* mean, float* var, int B, int D, hipStream_t stream) {
  if (B < 1 || D < 4 || (D & 3)) return vl_set_error("vl_lp_bn_fwd: bad shape (B >= 1, D a positive multiple of 4)");
  if (train && B < 2) return vl_set_error("vl_lp_bn_fwd: batch statistics need B >= 2 (nn.BatchNorm1d raises there too)");
  if (!x || !xhat) return vl_set_error("vl_lp_bn_fwd: x and xhat are required");
  if (ldx < D || ldh < D || (ldx & 3) || (ldh & 3)) return vl_set_error("vl_lp_bn_fwd: ldx, ldh must be multiples of 4 and >= D");
  if (((uintptr_t)x | (uintptr_t)xhat) & 15) return vl_set_error("vl_lp_bn_fwd: x and xhat must be 16-byte aligned");
  if (xhatT && (ldt < B || (ldt & 3))) return vl_set_error("vl_lp_bn_fwd: ldt must be a multiple of 4 and >= B");
  if (!(p >= 0.0f && p < 1.0f)) return vl_set_error("vl_lp_bn_fwd: dropout probability must be in [0, 1)");
  if (!(eps >= 0.0f)) return vl_set_error("vl_lp_bn_fwd: eps must be >= 0");
  if (!train && (!running_mean || !running_var)) return vl_set_error("vl_lp_bn_fwd: eval mode needs the running statistics");
  if (train && (!running_mean) != (!running_var)) return vl_set_error("vl_lp_bn_fwd: running_mean and running_var come together");
  if (train && !(momentum >= 0.0f && momentum <= 1.0f)) return vl_set_error("vl_lp_bn_fwd: momentum must be in [0, 1]");
  const int drop = train && p > 0.0f;
  if (drop && keep && ((uintptr_t)keep & 3)) return vl_set_error("vl_lp_bn_fwd: keep must be 4-byte aligned");
  BnArgs a;
  a.x = x; a.ldx = ldx; a.keep = drop ? keep : nullptr;
  a.thr = (uint32_t)((double)p * 4294967296.0);          // a Philox word below it is a dropped element
  a.scale = 1.0f / (1.0f - p);
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.sample0 = (uint64_t)sample0; a.drop = drop;
  a.rmean = running_mean; a.rvar = running_var; a.momentum = momentum; a.eps = eps;
  a.xhat = xhat; a.ldh = ldh; a.xhatT = xhatT; a.ldt = ldt; a.mean = mean; a.var = var; a.B = B; a.D = D;
  const dim3 grid((unsigned)((D + BN_STRIP - 1) / BN_STRIP)), block(256);
  if (train) hipLaunchKernelGGL(lp_bn_kernel<true>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(lp_bn_kernel<false>, grid, block, 0, stream, a);
  return launched();
}

extern "C" long vl_ce_label_ws_floats(int B, int C) {
  if (B < 1 || C < 1) return 0;
  return 2L * B + (long)((B + 63) / 64) * C;
}

extern "C" int vl_ce_label(const float* logits, long ld, const int64_t* target, int B, int C, float gscale, float* loss,
                           float* G, long ldg, float* GT, long ldgt, float* dbias, float* ws, hipStream_t stream) {
  if (B < 1 || C < 1) return vl_set_error("vl_ce_label: bad shape (B >= 1, C >= 1)");
  if (!logits || !target || !loss) return vl_set_error("vl_ce_label: logits, target and loss are required");
  if (!ws) return vl_set_error("vl_ce_label: a workspace of vl_ce_label_ws_floats(B, C) floats is required");
  if (ld < C) return vl_set_error("vl_ce_label: ld must be >= C");
  if (G && ldg < C) return vl_set_error("vl_ce_label: ldg must be >= C");
  if (GT && (ldgt < B || (ldgt & 3))) return vl_set_error("vl_ce_label: ldgt must be a multiple of 4 and >= B");
  const int nbt = (B + 63) / 64;
  if (nbt > 65535) return vl_set_error("vl_ce_label: B beyond 65535 * 64 rows");
  float* lse = ws; float* rowloss = ws + B; float* part = ws + 2L * B;
  hipLaunchKernelGGL(ce_label_rows_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, logits, ld, target, B, C, lse,
                     rowloss);
  if (G || GT || dbias)
    hipLaunchKernelGGL(ce_label_grad_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)nbt), dim3(256), 0, stream, logits, ld,
                       target, B, C, lse, gscale / (float)B, G, ldg, GT, ldgt, dbias ? part : nullptr);
  hipLaunchKernelGGL(ce_label_final_kernel, dim3(1u + (dbias ? (unsigned)((C + 255) / 256) : 0u)), dim3(256), 0, stream, rowloss,
                     B, loss, part, nbt, C, dbias);
  return launched();
}

extern "C" long vl_lars_ws_floats(long total_elems, int nslots) {
  if (total_elems < 0 || nslots < 0) return 0;
  return 4L * (total_elems / kLarsTile + nslots);          // two doubles per tile
}

extern "C" int vl_lars_multi_step(const vl_lars_slot* slots, int nslots, float lr, float momentum, float trust_coefficient,
                                  float grad_scale, float max_norm, const float* sumsq, float* ws, long ws_floats,
                                  hipStream_t stream) {
  if (nslots < 0 || nslots > VL_LARS_MAX_SLOTS) return vl_set_error("vl_lars_multi_step: 0 <= nslots <= VL_LARS_MAX_SLOTS");
  if (nslots == 0) return 0;
  if (!slots) return vl_set_error("vl_lars_multi_step: null slot table");
  if (max_norm > 0.0f && !sumsq) return vl_set_error("vl_lars_multi_step: max_norm > 0 needs sumsq (vl_sumsq_f32 of the gradients)");
  if (!ws || ((uintptr_t)ws & 7) || ws_floats < 4)
    return vl_set_error("vl_lars_multi_step: workspace of vl_lars_ws_floats(total, nslots) floats, 8-byte aligned, required");
  const long cap = ws_floats / 4 > 0x7fffffffL ? 0x7fffffffL : ws_floats / 4;
  // the table lives on the device: the grid cannot follow the element count, the tiles are dealt round-robin to 2048 workgroups
  hipLaunchKernelGGL(lars_norm_kernel, dim3(2048), dim3(256), 0, stream, slots, nslots, grad_scale, max_norm, sumsq, (double*)ws,
                     (int)cap);
  hipLaunchKernelGGL(lars_update_kernel, dim3(2048), dim3(256), 0, stream, slots, nslots, lr, momentum, trust_coefficient,
                     grad_scale, max_norm, sumsq, (const double*)ws, (int)cap);
  return launched();
}

extern "C" int vl_topk_hits(const float* logits, long ld, const int64_t* target, int B, int C, int k0, int k1, int* hits,
                            uint8_t* correct, hipStream_t stream) {
  if (B < 1 || C < 1) return vl_set_error("vl_topk_hits: bad shape (B >= 1, C >= 1)");
  if (!logits || !target || !hits) return vl_set_error("vl_topk_hits: logits, target and hits are required");
  if (ld < C) return vl_set_error("vl_topk_hits: ld must be >= C");
  if (k0 < 1 || k1 < 1) return vl_set_error("vl_topk_hits: k counts from 1");
  hipLaunchKernelGGL(topk_hits_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, logits, ld, target, B, C, k0, k1, hits,
                     correct);
  return launched();
}
