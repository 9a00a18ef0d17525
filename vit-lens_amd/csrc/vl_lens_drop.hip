// Perceiver dropout for gfx950: the Lens's attn_dropout inside the flash-style attention forward and its two-kernel backward,
// and ff_dropout as row kernels around the FeedForward's down-projection (open_clip/perceiver.py:91-102 `nn.Dropout` behind
// net.2, :105-154 `attn = self.dropout(sim.softmax(-1))`).  Train mode only; the default p = 0 never gets here (the callers keep
// today's entries).
//
// The probabilities of the attention are never in memory, so neither is their mask: it is a pure function of numbers that the
// forward, the backward and any recompute evaluate alike.  Element e is KEPT iff its Philox4x32-10 word is >= round(p 2^32)
// (uint32); a kept value is multiplied by 1 / (1 - p), computed in fp32.  Key (lo32, hi32) of the seed; counter
//     (group, lo32(sample0 + b), hi32(sample0 + b), sublayer)
//   attention probability (h, i, j):  group = (h Lq + i) ceil(Lk / 4) + j / 4,  word j % 4
//   FeedForward output (row i, col c): group = i (D / 4) + c / 4,               word c % 4
// (include/vitlens_hip.h; tests/perceiver_drop_ref.py is the numpy restatement).  `sublayer` = the position of the sub-layer
// in the Perceiver's forward, `sample0 + b` the per-sample number of step.drop_sample0 with tower id 2.
//
//   forward   : the body of vl_attn.hip's kernel (vl_attn_fwd_body.inc) with the mask applied to a tile's unnormalised fp32
//               probabilities BEHIND the running sum (the normaliser and lse count every key) and in front of the bf16
//               packing for P.V.  In the body's layout a lane owns query `qidx` and keys key0 + (r & 3) + 8 (r >> 2): four
//               aligned groups of four keys, one Philox call each.  One instantiation per head dim, with the key-chunk loop
//               (any Lk) and without the shared-last-row and LDS-DMA variants, which only p = 0 has.
//   backward A: vl_attn_bwd.hip's dQ kernel; dP is masked and scaled in the same layout (four calls per lane per tile),
//               dS = P (dP M / (1 - p) - delta).
//   backward B: its dK / dV kernel; here a lane owns ONE key and 16 queries, i.e. 16 groups: 16 calls per lane per tile, one
//               word of each used.  dV accumulates (P M / (1 - p))^T dO, dK the same dS.  (Left open: four neighbouring lanes
//               need the four words of the same calls - a quad transpose would cut the calls to four.)
//   FeedForward: x1 = x0 + y M / (1 - p) on fp32 rows, and the branch gradient dy = dx1 M / (1 - p) as the bf16 operand of
//               the dW2 / dGEGLU products plus, unrounded, for db2's column sum (p = 0 sums the fp32 residual gradient there:
//               a bf16 copy would add a rounding that path does not have).  Separate multiply and add, each rounded once:
//               what numpy computes.
#include "vl_attn_common.h"
#include "vl_philox.h"
#include "vitlens_hip.h"

namespace {
using namespace vlattn;

struct DropArgs {
  uint32_t k0, k1;       // Philox key: lo32, hi32 of the seed
  uint64_t sample0;      // per-sample number of batch row 0
  uint32_t sub;          // counter word 3: the sub-layer's position in the forward
  uint32_t thr;          // keep iff word >= thr
  float inv_keep;        // 1 / (1 - p)
  uint32_t kg4;          // attention: ceil(Lk / 4) groups per (head, query)
};

// multipliers (0 or 1 / (1 - p)) of the four elements of group g
__device__ __forceinline__ void drop_mul4(const DropArgs& d, uint32_t slo, uint32_t shi, uint32_t g, float* m) {
  const U4 r = philox4x32_10(U4{g, slo, shi, d.sub}, d.k0, d.k1);
  m[0] = r.x >= d.thr ? d.inv_keep : 0.f;
  m[1] = r.y >= d.thr ? d.inv_keep : 0.f;
  m[2] = r.z >= d.thr ? d.inv_keep : 0.f;
  m[3] = r.w >= d.thr ? d.inv_keep : 0.f;
}
// ... of element `word` of group g alone
__device__ __forceinline__ float drop_mul1(const DropArgs& d, uint32_t slo, uint32_t shi, uint32_t g, int word) {
  const U4 r = philox4x32_10(U4{g, slo, shi, d.sub}, d.k0, d.k1);
  const uint32_t w = word == 0 ? r.x : (word == 1 ? r.y : (word == 2 ? r.z : r.w));
  return w >= d.thr ? d.inv_keep : 0.f;
}
// A query-per-lane tile (forward, backward A): v[r] belongs to query qidx and key key0 + (r & 3) + 8 (r >> 2), key0 % 4 == 0.
// Keys at or beyond Lk and queries beyond Lq hold zeros (or are never stored): whatever group their index lands in is unused.
template <class V>
__device__ __forceinline__ void drop_tile_q(V& v, const DropArgs& d, int Lq, int h, int qidx, int key0) {
  const uint64_t s = d.sample0 + (uint64_t)blockIdx.z;
  const uint32_t slo = (uint32_t)s, shi = (uint32_t)(s >> 32);
  const uint32_t g0 = ((uint32_t)h * (uint32_t)Lq + (uint32_t)qidx) * d.kg4 + ((uint32_t)key0 >> 2);
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    float m[4];
    drop_mul4(d, slo, shi, g0 + 2u * gq, m);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[gq * 4 + e] *= m[e];
  }
}

// ------------------------------------------------------------------------------------------------------------ forward
constexpr int KC = 288;        // as in vl_attn.hip
constexpr int VSP = KC + 8;
constexpr int NWMAX = 8;
constexpr float RESCALE_THR = 8.0f;

struct AttnP {
  TV q, k, v;
  float qscale;
  bf16_t* out;
  float* lse;
  int B, H, Lq, Lk, causal;
  int dh;
  VL_PROF_FIELD
  int lq_main;
  DropArgs drop;
};

#define VL_ATTN_FWD_DROP(pv, p, h, qidx, key0) drop_tile_q(pv, (p).drop, (p).Lq, h, qidx, key0)

template <int DH>
__global__ void __launch_bounds__(NWMAX * 64, DH == 128 ? 2 : 4) attn_fwd_drop_kernel(const AttnP p) {
  constexpr bool TAILQ = false, MULTI = true, F16 = false, DMA = false, VARLEN = false;
  [[maybe_unused]] constexpr long row0 = 0;
#include "vl_attn_fwd_body.inc"
}

// ------------------------------------------------------------------------------------------------------------ backward
constexpr int NC = 288;        // queries per LDS chunk of kernel B
constexpr int NCA = 160;       // keys per LDS chunk of kernel A
constexpr float LOG2E = 1.4426950408889634f;

struct AttnBwdP {
  TV q, k, v, dO, o;
  const float* lse;
  float* delta;
  bf16_t *dq, *dk, *dv;
  long ld_dq, ld_dkv;
  int B, H, Lq, Lk, causal;
  int dh;
  float qscale, scale;
  int l_main;
  DropArgs drop;
};

// kernel A: one wave per 32 queries -> dQ, delta (vl_attn_bwd.hip: attn_bwd_dq_kernel without the shared last row)
template <int DH, int NCA>
__global__ void __launch_bounds__(NWMAX * 64, DH == 128 ? 2 : 4) attn_bwd_dq_drop_kernel(const AttnBwdP p) {
  constexpr int RB = DH * 2, KS = DH / 16, DT = DH / 32, TS = NCA + 8;
  constexpr bool PAD = DH == 128;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sK = smem;
  unsigned char* sV = smem + NCA * RB;
  bf16_t* sKt = (bf16_t*)(smem + 2 * NCA * RB);

  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), nwq = nthr >> 6;
  const int fr = lane & 31, fg = lane >> 5;
  const size_t bh = (size_t)b * p.H + h;
  const bf16_t* Qb = p.q.p + b * p.q.sb + h * p.q.sh;
  const bf16_t* Kb = p.k.p + b * p.k.sb + h * p.k.sh;
  const bf16_t* Vb = p.v.p + b * p.v.sb + h * p.v.sh;
  const bf16_t* Gb = p.dO.p + b * p.dO.sb + h * p.dO.sh;
  const bf16_t* Ob = p.o.p + b * p.o.sb + h * p.o.sh;
  const int q0 = (blockIdx.x * nwq + wid) * 32;
  const bool active = q0 < p.l_main;
  const int qidx = q0 + fr;
  const int qrow = qidx < p.l_main ? qidx : p.l_main - 1;
  const int dhr = PAD ? p.dh : DH, nch = dhr >> 3;
  const uint64_t samp = p.drop.sample0 + (uint64_t)b;
  const uint32_t slo = (uint32_t)samp, shi = (uint32_t)(samp >> 32);

  u32x4 qraw[KS], graw[KS], oraw[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    qraw[ks] = z; graw[ks] = z; oraw[ks] = z;
    if (!PAD || ks * 2 + fg < nch) {
      qraw[ks] = *(const u32x4*)(Qb + (long)qrow * p.q.sr + ks * 16 + fg * 8);
      graw[ks] = *(const u32x4*)(Gb + (long)qrow * p.dO.sr + ks * 16 + fg * 8);
      oraw[ks] = *(const u32x4*)(Ob + (long)qrow * p.o.sr + ks * 16 + fg * 8);
    }
  }
  const float lse_raw = p.lse[bh * p.Lq + qrow];
  stage2<DH, NCA, true, true, true, false, 2>(StageSrc{sK, sKt, Kb, p.k.sr, 1.f, nch}, StageSrc{sV, nullptr, Vb, p.v.sr, 1.f, nch},
                                              0, p.Lk, tid, nthr);
  bf16x8 qf[KS], dof[KS];
  float dlt = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = __builtin_bit_cast(bf16x8, p.qscale != 1.0f ? scale_bf16x8(qraw[ks], p.qscale) : qraw[ks]);
    dof[ks] = __builtin_bit_cast(bf16x8, graw[ks]);
    dlt = dot8(dof[ks], __builtin_bit_cast(bf16x8, oraw[ks]), dlt);
  }
  dlt = xhalf_sum(dlt);
  if (active && fg == 0 && qidx < p.l_main) p.delta[bh * p.Lq + qidx] = dlt;
  const float lse2 = lse_raw * LOG2E;

  f32x16 dq[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) dq[t] = zero16();

  const int blk_q_hi = min(p.l_main - 1, (int)(blockIdx.x * nwq + nwq) * 32 - 1);
  for (int kc0 = 0; kc0 < p.Lk; kc0 += NCA) {
    if (p.causal && kc0 > blk_q_hi) break;
    if (kc0 > 0) {
      __syncthreads();
      stage2<DH, NCA, true, true, true, false, 1>(StageSrc{sK, sKt, Kb, p.k.sr, 1.f, nch}, StageSrc{sV, nullptr, Vb, p.v.sr, 1.f, nch},
                                                  kc0, p.Lk, tid, nthr);
    }
    __syncthreads();
    if (!active) continue;
    int ntile = (min(p.Lk - kc0, NCA) + 31) >> 5;
    if (p.causal) ntile = min(ntile, ((q0 + 31 - kc0) >> 5) + 1);
    for (int kt = 0; kt < ntile; ++kt) {
      f32x16 s = zero16(), dp = zero16();
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<DH>(sK, kt * 32 + fr, ks, fg), qf[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<DH>(sV, kt * 32 + fr, ks, fg), dof[ks], dp, 0, 0, 0);
      }
      const int key0 = kc0 + kt * 32 + fg * 4;
      const bool need_mask = (key0 - fg * 4 + 32 > p.Lk) || (p.causal && key0 - fg * 4 + 31 > q0);
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = key0 + (r & 3) + 8 * (r >> 2);
          if (key >= p.Lk || (p.causal && key > qidx)) s[r] = -INFINITY;
        }
      }
      // dS = P (dP M / (1 - p) - delta), one group of four keys at a time (the scheduling barrier keeps the four Philox
      // chains from being interleaved: their temporaries would not fit beside the accumulators)
      float ds[16];
      const uint32_t g0 = ((uint32_t)h * (uint32_t)p.Lq + (uint32_t)qidx) * p.drop.kg4 + ((uint32_t)key0 >> 2);
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        float m[4];
        drop_mul4(p.drop, slo, shi, g0 + 2u * gq, m);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = gq * 4 + e;
          ds[r] = __builtin_amdgcn_exp2f(s[r] - lse2) * fmaf(dp[r], m[e], -dlt);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const bf16x8 df = pack8(ds + c * 8);
#pragma unroll
        for (int t = 0; t < DT; ++t)
          dq[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_t<NCA>(sKt, t * 32 + fr, kt, c, fg), df, dq[t], 0, 0, 0);
      }
    }
  }
  if (active)
    store_rows_t<DT>(dq, p.scale, p.dq + ((size_t)b * p.Lq + qrow) * p.ld_dq + h * dhr, fg, qidx < p.l_main, nch);
}

// kernel B: one wave per 32 keys -> dK, dV (vl_attn_bwd.hip: attn_bwd_dkv_kernel without the shared last key).  -delta is
// read beside the dP product instead of entering it as the C operand: the mask multiplies dO V^T alone.
template <int DH, int NCB>
__global__ void __launch_bounds__(NWMAX * 64, 2) attn_bwd_dkv_drop_kernel(const AttnBwdP p) {
  constexpr int RB = DH * 2, KS = DH / 16, DT = DH / 32, TS = NCB + 8;
  constexpr bool PAD = DH == 128;
  // output d-tiles per pass: all of them, or two of the padded instantiation's four (S, dP and the keep bits recomputed in the
  // second pass), as in the p = 0 kernel
  constexpr int TPP = PAD ? 2 : DT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sQ = smem;
  unsigned char* sdO = smem + NCB * RB;
  bf16_t* sQt = (bf16_t*)(smem + 2 * NCB * RB);
  bf16_t* sdOt = sQt + DH * TS;
  float* sNegL = (float*)(sdOt + DH * TS);
  float* sNegD = sNegL + NCB;

  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), nwk = nthr >> 6;
  const int fr = lane & 31, fg = lane >> 5;
  const size_t bh = (size_t)b * p.H + h;
  const bf16_t* Qb = p.q.p + b * p.q.sb + h * p.q.sh;
  const bf16_t* Kb = p.k.p + b * p.k.sb + h * p.k.sh;
  const bf16_t* Vb = p.v.p + b * p.v.sb + h * p.v.sh;
  const bf16_t* Gb = p.dO.p + b * p.dO.sb + h * p.dO.sh;
  const int k0 = (blockIdx.x * nwk + wid) * 32;
  const bool active = k0 < p.l_main;
  const int kidx = k0 + fr;
  const int krow = kidx < p.l_main ? kidx : p.l_main - 1;
  const int dhr = PAD ? p.dh : DH, nch = dhr >> 3;
  const uint64_t samp = p.drop.sample0 + (uint64_t)b;
  const uint32_t slo = (uint32_t)samp, shi = (uint32_t)(samp >> 32);
  const uint32_t kgrp = (uint32_t)kidx >> 2;
  const int kword = kidx & 3;

  bf16x8 kf[KS], vf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kf[ks] = zero_bf8(); vf[ks] = zero_bf8();
    if (!PAD || ks * 2 + fg < nch) {
      kf[ks] = *(const bf16x8*)(Kb + (long)krow * p.k.sr + ks * 16 + fg * 8);
      vf[ks] = *(const bf16x8*)(Vb + (long)krow * p.v.sr + ks * 16 + fg * 8);
    }
  }
  const float ln2 = 0.6931471805599453f;
#pragma unroll 1
  for (int tp = 0; tp < DT; tp += TPP) {
  f32x16 dk[TPP], dv[TPP];
#pragma unroll
  for (int t = 0; t < TPP; ++t) { dk[t] = zero16(); dv[t] = zero16(); }

  for (int qc0 = 0; qc0 < p.Lq; qc0 += NCB) {
    __syncthreads();
    stage2<DH, NCB, true, true, true, true>(StageSrc{sQ, sQt, Qb, p.q.sr, p.qscale, nch}, StageSrc{sdO, sdOt, Gb, p.dO.sr, 1.f, nch},
                                           qc0, p.Lq, tid, nthr);
    for (int i = tid; i < NCB; i += nthr) {
      const bool ok = qc0 + i < p.Lq;
      sNegL[i] = ok ? -p.lse[bh * p.Lq + qc0 + i] * LOG2E : -INFINITY;
      sNegD[i] = ok ? -p.delta[bh * p.Lq + qc0 + i] : 0.f;
    }
    __syncthreads();
    const int ntile = (min(p.Lq - qc0, NCB) + 31) >> 5;
    if (!active) continue;
    int t0 = 0;
    if (p.causal) t0 = max(0, (k0 - qc0) >> 5);
    for (int qt = t0; qt < ntile; ++qt) {
      // rows of the accumulator = queries (r & 3) + 8 (r >> 2) + 4 fg of this tile; column = this lane's key.  The 16 keep
      // bits first, while neither score tile is live, in a loop that stays rolled: unrolled, the sixteen Philox chains are
      // interleaved and their temporaries spill beside the accumulators (the padded instantiation: 39 registers).  The group
      // of query row r = one per-lane base + a wave-uniform multiple of ceil(Lk / 4)
      uint32_t keep = 0u;
      const uint32_t gq0 = ((uint32_t)h * (uint32_t)p.Lq + (uint32_t)(qc0 + qt * 32 + 4 * fg)) * p.drop.kg4 + kgrp;
#pragma unroll 1
      for (int r = 0; r < 16; ++r) {
        const uint32_t g = gq0 + (uint32_t)((r & 3) + 8 * (r >> 2)) * p.drop.kg4;
        keep |= (drop_mul1(p.drop, slo, shi, g, kword) != 0.f ? 1u : 0u) << r;
      }
      f32x16 s, dp = zero16();
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const f32x4 l4 = *(const f32x4*)(sNegL + qt * 32 + qd * 8 + fg * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[qd * 4 + e] = l4[e];
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<DH>(sQ, qt * 32 + fr, ks, fg), kf[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<DH>(sdO, qt * 32 + fr, ks, fg), vf[ks], dp, 0, 0, 0);
      }
      if (p.causal && qc0 + qt * 32 < k0 + 31) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qg = qc0 + qt * 32 + (r & 3) + 8 * (r >> 2) + 4 * fg;
          if (kidx > qg) s[r] = -INFINITY;
        }
      }
      float pv[16], ds[16];
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const f32x4 d4 = *(const f32x4*)(sNegD + qt * 32 + qd * 8 + fg * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = qd * 4 + e;
          const float m = (keep >> r) & 1u ? p.drop.inv_keep : 0.f;
          const float pr = __builtin_amdgcn_exp2f(s[r]);       // (padded query rows: -inf -> 0)
          ds[r] = pr * fmaf(dp[r], m, d4[e]);                  // dS = P (dP M / (1 - p) - delta)
          pv[r] = pr * m;
        }
      }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const bf16x8 pf = pack8(pv + c * 8), df = pack8(ds + c * 8);
#pragma unroll
        for (int t = 0; t < TPP; ++t) {
          dv[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_t<NCB>(sdOt, (tp + t) * 32 + fr, qt, c, fg), pf, dv[t], 0, 0, 0);
          dk[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_t<NCB>(sQt, (tp + t) * 32 + fr, qt, c, fg), df, dk[t], 0, 0, 0);
        }
      }
    }
  }
  if (active) {
    store_rows_t<TPP>(dk, ln2, p.dk + ((size_t)b * p.Lk + krow) * p.ld_dkv + h * dhr + tp * 32, fg, kidx < p.l_main, nch - tp * 4);
    store_rows_t<TPP>(dv, 1.f, p.dv + ((size_t)b * p.Lk + krow) * p.ld_dkv + h * dhr + tp * 32, fg, kidx < p.l_main, nch - tp * 4);
  }
  }   // passes over the output d-tiles
}

// ------------------------------------------------------------------------------------------------------- FeedForward rows
// one thread per group of four columns; gi = row * (D / 4) + c / 4 over all B n rows
template <bool BWD>
__global__ void __launch_bounds__(256) ff_drop_kernel(const float* y, const float* x0, float* x1, bf16_t* dy, long total, int n,
                                                      int D4, DropArgs d) {
  // (no contraction: the product is rounded before the sum, as numpy rounds it; the __f*_rn intrinsics do not stop hipcc's)
#pragma clang fp contract(off)
  const long gi = (long)blockIdx.x * 256 + threadIdx.x;
  if (gi >= total) return;
  const long row = gi / D4;
  const uint32_t c4 = (uint32_t)(gi - row * D4);
  const uint64_t s = d.sample0 + (uint64_t)(row / n);
  float m[4];
  drop_mul4(d, (uint32_t)s, (uint32_t)(s >> 32), (uint32_t)(row % n) * (uint32_t)D4 + c4, m);
  const f32x4 yv = *(const f32x4*)(y + gi * 4);
  if constexpr (BWD) {
    const f32x4 t = {yv[0] * m[0], yv[1] * m[1], yv[2] * m[2], yv[3] * m[3]};
    const u32x2 w = {pack2bf(t[0], t[1]), pack2bf(t[2], t[3])};
    *(u32x2*)(dy + gi * 4) = w;
    if (x1) *(f32x4*)(x1 + gi * 4) = t;                // the unrounded copy: db2 is its column sum
  } else {
    const f32x4 xv = *(const f32x4*)(x0 + gi * 4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = yv[e] * m[e];
      o[e] = xv[e] + t;
    }
    *(f32x4*)(x1 + gi * 4) = o;
  }
}

}  // namespace

extern "C" int vl_set_error(const char* msg);

// p -> threshold and scale; 0 on success
static int drop_args(const char* who, double p, uint64_t seed, int64_t sample0, int sublayer, uint64_t groups, uint32_t kg4,
                     DropArgs* d) {
  static thread_local char msg[160];
  if (!(p >= 0.0 && p < 1.0)) { snprintf(msg, sizeof msg, "%s: dropout probability must be in [0, 1)", who); return vl_set_error(msg); }
  const double t = nearbyint(p * 4294967296.0);
  if (t >= 4294967296.0) { snprintf(msg, sizeof msg, "%s: dropout probability rounds to 1", who); return vl_set_error(msg); }
  if (sublayer < 0) { snprintf(msg, sizeof msg, "%s: sublayer must be >= 0", who); return vl_set_error(msg); }
  if (groups > 0xffffffffull) { snprintf(msg, sizeof msg, "%s: more than 2^32 element groups per sample", who); return vl_set_error(msg); }
  *d = DropArgs{(uint32_t)seed, (uint32_t)(seed >> 32), (uint64_t)sample0, (uint32_t)sublayer, (uint32_t)t,
                1.0f / (1.0f - (float)p), kg4};
  return 0;
}

template <int DH>
static int launch_fwd_drop(const AttnP& p, int gx, int nwq, hipStream_t stream) {
  const size_t smem = (size_t)KC * DH * 2 + (size_t)DH * VSP * 2 + (size_t)NWMAX * 32 * 4 + (size_t)(KC / 32) * (2 + DH) * 4 +
                      (size_t)DH * 2;
  static const hipError_t attr = hipFuncSetAttribute((const void*)attn_fwd_drop_kernel<DH>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (attr != hipSuccess) return vl_set_error(hipGetErrorString(attr));
  hipLaunchKernelGGL((attn_fwd_drop_kernel<DH>), dim3(gx, p.H, p.B), dim3(nwq * 64), smem, stream, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}

static bool head_dim_ok(int dh) { return dh == 32 || dh == 64 || (dh > 64 && dh <= 128 && (dh & 7) == 0); }

extern "C" int vl_attn_fwd_drop_bf16(const void* q, const void* k, const void* v, const long* strides, void* out, float* lse,
                                     int B, int H, int Lq, int Lk, int dh, float qscale, int causal, double pdrop, uint64_t seed,
                                     int64_t sample0, int sublayer, hipStream_t stream) {
  if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return vl_set_error("vl_attn_fwd_drop_bf16: empty problem");
  if (!head_dim_ok(dh))
    return vl_set_error("vl_attn_fwd_drop_bf16: head dim must be 32, 64, or a multiple of 8 in (64, 128] (run zero-padded to 128)");
  if (!strides || !q || !k || !v || !out) return vl_set_error("vl_attn_fwd_drop_bf16: q, k, v, out and strides required");
  for (int i = 0; i < 9; ++i)
    if (strides[i] & 7) return vl_set_error("vl_attn_fwd_drop_bf16: operand strides must be multiples of 8 elements (16-byte rows)");
  if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v)) & 15) return vl_set_error("vl_attn_fwd_drop_bf16: operands must be 16-byte aligned");
  const uint32_t kg4 = (uint32_t)((Lk + 3) / 4);
  AttnP p{};
  if (drop_args("vl_attn_fwd_drop_bf16", pdrop, seed, sample0, sublayer, (uint64_t)H * (uint64_t)Lq * kg4, kg4, &p.drop)) return 1;
  p.q = TV{(const bf16_t*)q, strides[0], strides[1], strides[2]};
  p.k = TV{(const bf16_t*)k, strides[3], strides[4], strides[5]};
  p.v = TV{(const bf16_t*)v, strides[6], strides[7], strides[8]};
  p.qscale = qscale; p.out = (bf16_t*)out; p.lse = lse;
  p.B = B; p.H = H; p.Lq = Lq; p.Lk = Lk; p.causal = causal; p.dh = dh; p.lq_main = Lq;
  const int qtiles = (Lq + 31) / 32;
  const int nwq = qtiles < NWMAX ? qtiles : NWMAX;
  const int gx = (qtiles + nwq - 1) / nwq;
  return dh == 64 ? launch_fwd_drop<64>(p, gx, nwq, stream)
                  : (dh == 32 ? launch_fwd_drop<32>(p, gx, nwq, stream) : launch_fwd_drop<128>(p, gx, nwq, stream));
}

template <int DH>
static int launch_bwd_drop(const AttnBwdP& pin, hipStream_t stream) {
  constexpr int NCB = DH == 128 ? 96 : NC;
  const size_t smA = (size_t)2 * NCA * DH * 2 + (size_t)DH * (NCA + 8) * 2;
  const size_t smB = (size_t)2 * NCB * DH * 2 + (size_t)2 * DH * (NCB + 8) * 2 + (size_t)2 * NCB * 4;
  static const hipError_t attrA = hipFuncSetAttribute((const void*)attn_bwd_dq_drop_kernel<DH, NCA>,
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)smA);
  static const hipError_t attrB = hipFuncSetAttribute((const void*)attn_bwd_dkv_drop_kernel<DH, NCB>,
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)smB);
  if (attrA != hipSuccess) return vl_set_error(hipGetErrorString(attrA));
  if (attrB != hipSuccess) return vl_set_error(hipGetErrorString(attrB));
  AttnBwdP p = pin;
  const int qtiles = (p.Lq + 31) / 32, ktiles = (p.Lk + 31) / 32;
  const int nwq = qtiles < NWMAX ? qtiles : NWMAX, nwk = ktiles < NWMAX ? ktiles : NWMAX;
  p.l_main = p.Lq;
  hipLaunchKernelGGL((attn_bwd_dq_drop_kernel<DH, NCA>), dim3((qtiles + nwq - 1) / nwq, p.H, p.B), dim3(nwq * 64), smA, stream, p);
  p.l_main = p.Lk;
  hipLaunchKernelGGL((attn_bwd_dkv_drop_kernel<DH, NCB>), dim3((ktiles + nwk - 1) / nwk, p.H, p.B), dim3(nwk * 64), smB, stream, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}

extern "C" int vl_attn_bwd_drop_bf16(const void* q, const void* k, const void* v, const void* dO, const void* o,
                                     const long* strides, const float* lse, float* delta, void* dq, void* dk, void* dv,
                                     long ld_dq, long ld_dkv, int B, int H, int Lq, int Lk, int dh, float qscale, int causal,
                                     float scale, double pdrop, uint64_t seed, int64_t sample0, int sublayer,
                                     hipStream_t stream) {
  if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return vl_set_error("vl_attn_bwd_drop_bf16: empty problem");
  if (!head_dim_ok(dh))
    return vl_set_error("vl_attn_bwd_drop_bf16: head dim must be 32, 64, or a multiple of 8 in (64, 128] (run zero-padded to 128)");
  if (!strides || !delta || !lse) return vl_set_error("vl_attn_bwd_drop_bf16: strides, lse and the delta workspace are required");
  if (!q || !k || !v || !dO || !o || !dq || !dk || !dv) return vl_set_error("vl_attn_bwd_drop_bf16: operands and destinations required");
  for (int i = 0; i < 15; ++i)
    if (strides[i] & 7) return vl_set_error("vl_attn_bwd_drop_bf16: operand strides must be multiples of 8 elements (16-byte rows)");
  if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)dO) | ((uintptr_t)o)) & 15)
    return vl_set_error("vl_attn_bwd_drop_bf16: operands must be 16-byte aligned");
  if ((((uintptr_t)dq) | ((uintptr_t)dk) | ((uintptr_t)dv)) & 15 || (ld_dq & 7) || (ld_dkv & 7))
    return vl_set_error("vl_attn_bwd_drop_bf16: gradient destinations must be 16-byte aligned with row strides multiple of 8");
  const long* s = strides;
  const uint32_t kg4 = (uint32_t)((Lk + 3) / 4);
  AttnBwdP p{};
  if (drop_args("vl_attn_bwd_drop_bf16", pdrop, seed, sample0, sublayer, (uint64_t)H * (uint64_t)Lq * kg4, kg4, &p.drop)) return 1;
  p.q = TV{(const bf16_t*)q, s[0], s[1], s[2]};    p.k = TV{(const bf16_t*)k, s[3], s[4], s[5]};
  p.v = TV{(const bf16_t*)v, s[6], s[7], s[8]};    p.dO = TV{(const bf16_t*)dO, s[9], s[10], s[11]};
  p.o = TV{(const bf16_t*)o, s[12], s[13], s[14]};
  p.lse = lse; p.delta = delta; p.dq = (bf16_t*)dq; p.dk = (bf16_t*)dk; p.dv = (bf16_t*)dv;
  p.ld_dq = ld_dq; p.ld_dkv = ld_dkv; p.B = B; p.H = H; p.Lq = Lq; p.Lk = Lk; p.causal = causal; p.dh = dh;
  p.qscale = qscale; p.scale = scale;
  return dh == 64 ? launch_bwd_drop<64>(p, stream) : (dh == 32 ? launch_bwd_drop<32>(p, stream) : launch_bwd_drop<128>(p, stream));
}

static int ff_drop(const char* who, bool bwd, const float* y, const float* x0, float* x1, void* dy, int B, int n, int D, double pdrop,
                   uint64_t seed, int64_t sample0, int sublayer, hipStream_t stream) {
  static thread_local char msg[160];
  if (B <= 0 || n <= 0 || D <= 0 || (D & 3)) {
    snprintf(msg, sizeof msg, "%s: bad shape (B, n >= 1, D a positive multiple of 4)", who);
    return vl_set_error(msg);
  }
  if (!y || (bwd ? !dy : (!x0 || !x1)) || ((((uintptr_t)y) | ((uintptr_t)x0) | ((uintptr_t)x1)) & 15) || (((uintptr_t)dy) & 7)) {
    snprintf(msg, sizeof msg, "%s: operands missing or not 16-byte aligned", who);
    return vl_set_error(msg);
  }
  DropArgs d;
  if (drop_args(who, pdrop, seed, sample0, sublayer, (uint64_t)n * (uint64_t)(D / 4), 0u, &d)) return 1;
  const long total = (long)B * n * (D / 4);
  if ((total + 255) / 256 > 0x7fffffffL) { snprintf(msg, sizeof msg, "%s: too many elements for one launch", who); return vl_set_error(msg); }
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (bwd) hipLaunchKernelGGL(ff_drop_kernel<true>, grid, block, 0, stream, y, x0, x1, (bf16_t*)dy, total, n, D / 4, d);
  else hipLaunchKernelGGL(ff_drop_kernel<false>, grid, block, 0, stream, y, x0, x1, (bf16_t*)dy, total, n, D / 4, d);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}

extern "C" int vl_ff_drop_fwd(const float* y, const float* x0, float* x1, int B, int n, int D, double p, uint64_t seed,
                              int64_t sample0, int sublayer, hipStream_t stream) {
  return ff_drop("vl_ff_drop_fwd", false, y, x0, x1, nullptr, B, n, D, p, seed, sample0, sublayer, stream);
}

extern "C" int vl_ff_drop_bwd(const float* dx1, void* dy, float* dy_f32, int B, int n, int D, double p, uint64_t seed,
                              int64_t sample0, int sublayer, hipStream_t stream) {
  return ff_drop("vl_ff_drop_bwd", true, dx1, nullptr, dy_f32, dy, B, n, D, p, seed, sample0, sublayer, stream);
}
