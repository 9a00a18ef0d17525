// Perceiver dropout for gfx950: the Lens's attn_dropout inside the flash-style attention forward, and ff_dropout as row kernels
// around the FeedForward's down-projection (open_clip/perceiver.py:91-102 `nn.Dropout` behind net.2, :105-154
// `attn = self.dropout(sim.softmax(-1))`).  The attention backward under dropout is the DROP instantiation of vl_attn_bwd.hip's
// two kernels.  Train mode only; the default p = 0 never gets here (the callers keep today's entries).
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
//   backward  : vl_attn_bwd.hip (vl_drop.h holds the mask's arithmetic for both files).
//   FeedForward: x1 = x0 + y M / (1 - p) on fp32 rows, and the branch gradient dy = dx1 M / (1 - p) as the bf16 operand of
//               the dW2 / dGEGLU products plus, unrounded, for db2's column sum (p = 0 sums the fp32 residual gradient there:
//               a bf16 copy would add a rounding that path does not have).  Separate multiply and add, each rounded once:
//               what numpy computes.
#include "vl_attn_common.h"
#include "vl_drop.h"
#include "vitlens_hip.h"

namespace {
using namespace vlattn;
using namespace vldrop;

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
