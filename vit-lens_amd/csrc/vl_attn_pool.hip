// Single-query attention, forward and backward: what the LAST block of a class-token-pooled ViT needs of its attention.
//
// The tower's feature is proj(ln_post(x[:, 0])): of the last block's output only the class-token row is read, so its
// attention has ONE query row per (batch, head) - q row `qrow` of the packed in-projection output - against all L keys and
// values (which still come from every token, the in-projection stays dense).  The backward mirrors it: only that row has
// an upstream gradient dO, so dQ is one row, dK[j] = dS_j q and dV[j] = p_j dO are rank-1 in the key index.
//
// One wave per (batch, head).  Lane (r, c) = (lane >> 3, lane & 7) reads the 16-byte chunk c (8 of the 64 head columns) of
// key row 8 i + r: a wave load covers 8 whole 128-byte rows, four of them in flight per lane.  Dot products are reduced over
// the 8 lanes of a row with three butterfly steps; sums over the keys (P V, dQ) stay in registers per lane and are reduced
// over r once at the end.  The kernels are bound by reading K and V once: fp32 math throughout, no matrix pipe.
//
// Conventions of the dense kernels (vl_attn.hip, vl_attn_bwd_fused.hip): q is multiplied by qscale = softmax_scale * log2e and
// rounded to bf16, scores live in the log2 domain, lse is stored in the natural-log domain of the scaled scores;
// dq = scale * sum_j dS_j k_j, dk_j = ln2 * dS_j * q2 (q2 = the rounded scaled query), dv_j = p_j dO.
//
// vl_attn_bwd_q1 also writes ZEROS to the dQ rows of every other token: the dX GEMM of the in-projection that follows reads
// a fully defined [tokens, 3 width] gradient without a separate fill pass.
#include <stdio.h>
#include "vl_attn_common.h"
#include "vitlens_hip.h"

namespace {
using namespace vlattn;

constexpr int Q1_MAXL = 1024;
constexpr float Q1_LOG2E = 1.4426950408889634f, Q1_LN2 = 0.6931471805599453f;

struct Q1FwdP {
  TV q, k, v;
  bf16_t* o; long ld_o;      // [B, >= H*64]: row b, columns h*64 ..
  float* lse;                // [B, H] or null
  int B, H, L, qrow;
  float qscale;
};

struct Q1BwdP {
  TV q, k, v;
  const bf16_t* dO; long ld_do;      // [B, >= H*64]
  const bf16_t* o; long ld_o;        // the forward's output
  const float* lse;                  // [B, H]
  bf16_t *dq, *dk, *dv;              // token-major [B*L, .] destinations, already offset to their column block
  long ld_dq, ld_dkv;
  int B, H, L, qrow;
  float qscale, scale;
};

__device__ __forceinline__ void q1_unpack8(u32x4 w, float (&f)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[2 * e] = bf2f((bf16_t)(w[e] & 0xffffu)); f[2 * e + 1] = bf2f((bf16_t)(w[e] >> 16)); }
}
__device__ __forceinline__ u32x4 q1_pack8(const float (&f)[8]) {
  u32x4 w;
#pragma unroll
  for (int e = 0; e < 4; ++e) w[e] = pack2bf(f[2 * e], f[2 * e + 1]);
  return w;
}
__device__ __forceinline__ float q1_dot8(const float (&a)[8], const float (&b)[8]) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s = fmaf(a[e], b[e], s);
  return s;
}
// sum over the 8 lanes that share a row (lane bits 0-2) / over the 8 rows of a pass (lane bits 3-5)
__device__ __forceinline__ float q1_sum_c(float v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
  return v;
}
__device__ __forceinline__ float q1_sum_r(float v) {
  v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
  return v;
}
// the query row, scaled and rounded to bf16 as the dense kernels stage it
__device__ __forceinline__ void q1_load_q(const TV& q, int b, int h, int qrow, int c, float qscale, float (&q2)[8]) {
  const bf16_t* Qb = q.p + (long)b * q.sb + (long)h * q.sh + (long)qrow * q.sr;
  float f[8];
  q1_unpack8(*(const u32x4*)(Qb + c * 8), f);
#pragma unroll
  for (int e = 0; e < 8; ++e) q2[e] = bf2f(f2bf(f[e] * qscale));
}

__global__ void __launch_bounds__(64) attn_fwd_q1_kernel(const Q1FwdP p) {
  __shared__ float sS[Q1_MAXL];
  const int bh = blockIdx.x, b = bh / p.H, h = bh - b * p.H;
  const int lane = threadIdx.x, r = lane >> 3, c = lane & 7;
  const int L = p.L;
  const bf16_t* Kb = p.k.p + (long)b * p.k.sb + (long)h * p.k.sh + c * 8;
  const bf16_t* Vb = p.v.p + (long)b * p.v.sb + (long)h * p.v.sh + c * 8;
  float q2[8];
  q1_load_q(p.q, b, h, p.qrow, c, p.qscale, q2);
  // ---- scores (log2 domain) into LDS, running maximum ----
  float mx = -INFINITY;
  for (int j0 = 0; j0 < L; j0 += 32) {
    u32x4 kr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = j0 + u * 8 + r;
      kr[u] = *(const u32x4*)(Kb + (long)(row < L ? row : L - 1) * p.k.sr);      // (past the end: the last row again, unused)
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = j0 + u * 8 + r;
      float kf[8];
      q1_unpack8(kr[u], kf);
      const float s = q1_sum_c(q1_dot8(q2, kf));
      if (row < L) {
        mx = fmaxf(mx, s);
        if (c == 0) sS[row] = s;
      }
    }
  }
  mx = wave_max(mx);
  __syncthreads();
  float l = 0.f;
  for (int j = lane; j < L; j += 64) {
    const float pj = __builtin_amdgcn_exp2f(sS[j] - mx);
    sS[j] = pj;
    l += pj;
  }
  l = wave_sum(l);
  __syncthreads();
  // ---- o = P V / l ----
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int j0 = 0; j0 < L; j0 += 32) {
    u32x4 vr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = j0 + u * 8 + r;
      vr[u] = *(const u32x4*)(Vb + (long)(row < L ? row : L - 1) * p.v.sr);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = j0 + u * 8 + r;
      const float pj = row < L ? sS[row] : 0.f;
      float vf[8];
      q1_unpack8(vr[u], vf);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, vf[e], acc[e]);
    }
  }
  const float inv = 1.0f / l;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = q1_sum_r(acc[e]) * inv;
  if (r == 0) *(u32x4*)(p.o + (long)b * p.ld_o + h * 64 + c * 8) = q1_pack8(acc);
  if (p.lse && lane == 0) p.lse[bh] = (mx + __log2f(l)) * Q1_LN2;
}

__global__ void __launch_bounds__(64) attn_bwd_q1_kernel(const Q1BwdP p) {
  const int bh = blockIdx.x, b = bh / p.H, h = bh - b * p.H;
  const int lane = threadIdx.x, r = lane >> 3, c = lane & 7;
  const int L = p.L;
  const bf16_t* Kb = p.k.p + (long)b * p.k.sb + (long)h * p.k.sh + c * 8;
  const bf16_t* Vb = p.v.p + (long)b * p.v.sb + (long)h * p.v.sh + c * 8;
  float q2[8], g[8], of[8];
  q1_load_q(p.q, b, h, p.qrow, c, p.qscale, q2);
  q1_unpack8(*(const u32x4*)(p.dO + (long)b * p.ld_do + h * 64 + c * 8), g);
  q1_unpack8(*(const u32x4*)(p.o + (long)b * p.ld_o + h * 64 + c * 8), of);
  const float delta = q1_sum_c(q1_dot8(g, of));        // rowsum(dO * O)
  const float nl = -p.lse[bh] * Q1_LOG2E;
  const long row0 = (long)b * L;
  bf16_t* dQ = p.dq + h * 64 + c * 8;
  bf16_t* dK = p.dk + h * 64 + c * 8;
  bf16_t* dV = p.dv + h * 64 + c * 8;
  float aq[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) aq[e] = 0.f;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int j0 = 0; j0 < L; j0 += 32) {
    u32x4 kr[4], vr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = j0 + u * 8 + r;
      const long rc = row < L ? row : L - 1;
      kr[u] = *(const u32x4*)(Kb + rc * p.k.sr);
      vr[u] = *(const u32x4*)(Vb + rc * p.v.sr);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = j0 + u * 8 + r;
      float kf[8], vf[8];
      q1_unpack8(kr[u], kf); q1_unpack8(vr[u], vf);
      const float s = q1_sum_c(q1_dot8(q2, kf));
      const float dp = q1_sum_c(q1_dot8(g, vf));
      const float pj = __builtin_amdgcn_exp2f(s + nl);
      const float ds = pj * (dp - delta);
      if (row < L) {
        float dk[8], dv[8];
        const float dsl = ds * Q1_LN2;
#pragma unroll
        for (int e = 0; e < 8; ++e) { dk[e] = dsl * q2[e]; dv[e] = pj * g[e]; aq[e] = fmaf(ds, kf[e], aq[e]); }
        *(u32x4*)(dK + (row0 + row) * p.ld_dkv) = q1_pack8(dk);
        *(u32x4*)(dV + (row0 + row) * p.ld_dkv) = q1_pack8(dv);
        if (row != p.qrow) *(u32x4*)(dQ + (row0 + row) * p.ld_dq) = zero;      // no other query row has a gradient
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) aq[e] = q1_sum_r(aq[e]) * p.scale;
  if (r == 0) *(u32x4*)(dQ + (row0 + p.qrow) * p.ld_dq) = q1_pack8(aq);
}

}  // namespace

extern "C" int vl_set_error(const char* msg);

static const char* q1_check(const long* strides, int nstr, int B, int H, int L, int dh, int qrow) {
  if (B <= 0 || H <= 0) return "empty problem";
  if (dh != 64) return "head dim 64 only (the dense kernels take the others)";
  if (L < 1 || L > Q1_MAXL) return "1 <= L <= 1024 required";
  if (qrow < 0 || qrow >= L) return "query row index outside [0, L)";
  if ((long)B * H > 0x7fffffffL) return "too many (batch, head) pairs";
  if (!strides) return "strides are required";
  for (int i = 0; i < nstr; ++i)
    if (strides[i] & 7) return "operand strides must be multiples of 8 elements (16-byte rows)";
  return nullptr;
}

extern "C" int vl_attn_fwd_q1(const void* q, const void* k, const void* v, const long* strides, void* out, long ld_out,
                              float* lse, int B, int H, int L, int dh, int qrow, float qscale, hipStream_t stream) {
  char msg[160];
  if (const char* why = q1_check(strides, 9, B, H, L, dh, qrow)) {
    snprintf(msg, sizeof(msg), "vl_attn_fwd_q1: %s", why);
    return vl_set_error(msg);
  }
  if (!q || !k || !v || !out) return vl_set_error("vl_attn_fwd_q1: null operand");
  if (((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)out)) & 15) || (ld_out & 7) || ld_out < (long)H * 64)
    return vl_set_error("vl_attn_fwd_q1: operands must be 16-byte aligned, ld_out a multiple of 8 and >= H * 64");
  const long* s = strides;
  Q1FwdP p{TV{(const bf16_t*)q, s[0], s[1], s[2]}, TV{(const bf16_t*)k, s[3], s[4], s[5]}, TV{(const bf16_t*)v, s[6], s[7], s[8]},
           (bf16_t*)out, ld_out, lse, B, H, L, qrow, qscale};
  hipLaunchKernelGGL(attn_fwd_q1_kernel, dim3((unsigned)(B * H)), dim3(64), 0, stream, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}

extern "C" int vl_attn_bwd_q1(const void* q, const void* k, const void* v, const long* strides, const void* dO, long ld_do,
                              const void* o, long ld_o, const float* lse, void* dq, void* dk, void* dv, long ld_dq, long ld_dkv,
                              int B, int H, int L, int dh, int qrow, float qscale, float scale, hipStream_t stream) {
  char msg[160];
  if (const char* why = q1_check(strides, 9, B, H, L, dh, qrow)) {
    snprintf(msg, sizeof(msg), "vl_attn_bwd_q1: %s", why);
    return vl_set_error(msg);
  }
  if (!q || !k || !v || !dO || !o || !lse || !dq || !dk || !dv) return vl_set_error("vl_attn_bwd_q1: null operand");
  if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)dO) | ((uintptr_t)o) | ((uintptr_t)dq) | ((uintptr_t)dk) |
       ((uintptr_t)dv)) & 15)
    return vl_set_error("vl_attn_bwd_q1: operands and gradient destinations must be 16-byte aligned");
  if ((ld_do & 7) || (ld_o & 7) || (ld_dq & 7) || (ld_dkv & 7) || ld_do < (long)H * 64 || ld_o < (long)H * 64 ||
      ld_dq < (long)H * 64 || ld_dkv < (long)H * 64)
    return vl_set_error("vl_attn_bwd_q1: row strides must be multiples of 8 and >= H * 64");
  const long* s = strides;
  Q1BwdP p{TV{(const bf16_t*)q, s[0], s[1], s[2]}, TV{(const bf16_t*)k, s[3], s[4], s[5]}, TV{(const bf16_t*)v, s[6], s[7], s[8]},
           (const bf16_t*)dO, ld_do, (const bf16_t*)o, ld_o, lse, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, ld_dq, ld_dkv,
           B, H, L, qrow, qscale, scale};
  hipLaunchKernelGGL(attn_bwd_q1_kernel, dim3((unsigned)(B * H)), dim3(64), 0, stream, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}
