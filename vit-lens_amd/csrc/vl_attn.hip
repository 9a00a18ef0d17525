// Fused (flash-style) attention forward for gfx950.
//
// Replaces F.multi_head_attention_forward inside nn.MultiheadAttention
// (open_clip/transformer.py:241-252; additive causal mask :870-876) and the einsum attention of
// the Perceiver "Lens" (open_clip/perceiver.py:128-145).  The S = QK^T matrix and the
// probabilities never reach HBM.
//
// Layout contract: q, k, v are strided [B,H,L,DH] views (vl_attn_common.h) -- normally column blocks of the packed
// in-projection output [tokens, 3*width]; q is multiplied by qscale = softmax_scale*log2(e) when it is loaded (the
// reference scales q in bf16 too, functional.py via transformer.py:241).  (Round 1 took head-split copies and V
// transposed from the GEMM epilogue: 2-byte scattered stores that doubled the in-projection's epilogue time; the
// transposition now happens while V is staged into LDS.)
//
// One workgroup = one (batch, head) x up to 8 query tiles of 32 rows (one wave per tile), two workgroups per CU
// (<= 80 KB LDS, <= 128 VGPRs) so that one workgroup's staging overlaps the other's MFMA/VALU work.  K and V^T for a
// chunk of 288 keys sit in LDS and are shared by all query waves.  Operands are swapped -- S^T = K.Q^T and
// O^T = V^T.P^T -- so that with the 32x32x16 MFMA accumulator layout every lane owns ONE query column: the softmax row
// reduction is 16 in-register values + one cross-half exchange, the running max / sum are per-lane scalars, and P feeds
// the second MFMA straight from registers.  The k-slot permutation of the accumulator layout is absorbed by the ORDER
// in which V^T's key index is laid out in LDS (bits 2 and 3 of the key index swapped), so every V^T fragment is one
// ds_read_b128.
//
// The kernel is VALU-bound (16 v_exp_f32 per lane per 32x32 tile against 8 MFMAs), so the softmax arithmetic is trimmed
// to the exponentials: the running maximum enters as the MFMA's C operand (a register block holding -m), p = exp2(s)
// needs no subtraction, and the block / the output accumulators are rescaled only when the maximum grew by more than
// 2^8 (wave-uniform branch; p <= 256 in between, exact in fp32 / bf16 range).
//
// L = 257 (ViT-L/14 at 224: 8 full tiles + ONE row): the lone last query would cost a ninth wave nine tile passes for
// one row.  Instead the 8 waves finish their own tiles and then share it: wave w computes the row's scores against key
// tile w with the roles of the MFMA operands swapped (lane = key), reduces across lanes, multiplies by V through one
// more MFMA and the 9 partial (max, sum, O) triples are merged through LDS.
#include "vl_attn_common.h"
#include "vitlens_hip.h"

namespace {
using namespace vlattn;

constexpr int KC = 288;        // keys per LDS chunk (9 tiles of 32)
constexpr int KC_DENSE = KC;
constexpr int VSP = KC + 8;    // V^T LDS row stride in elements: 592 B = 16 B x odd -> conflict-free ds_read_b128
constexpr int NWMAX = 8;       // query waves per workgroup
constexpr float RESCALE_THR = 8.0f;

struct AttnP {
  TV q, k, v;
  float qscale;  // applied to q at load (1 = already scaled)
  bf16_t* out;   // [B, Lq, H*DH]
  float* lse;    // [B, H, Lq] (natural-log domain of the scaled scores) or null
  int B, H, Lq, Lk, causal;
  int dh;        // real head dim (= DH, or 72..128 in the DH = 128 instantiation)
  VL_PROF_FIELD
  int lq_main;   // queries handled by the per-wave tiles (Lq, or Lq-1 when the last row is shared)
};
// VARLEN: captions of different lengths packed one behind the other (vl_attn_fwd_varlen_f16); B = captions, Lq = Lk = the
// longest one, the strides' batch terms are unused
struct AttnPV : AttnP {
  const int* vstart;   // [B] first packed row of caption b
  const int* vlen;     // [B] its rows
};

// MULTI: more keys than one LDS chunk (the chunk loop restages inside the accumulation; kept out of the common
// single-chunk instantiations, where its 12 loads in flight would push the tile loop's registers to scratch)
// F16: q, k, v and the output are IEEE half (vl_attn_fwd_f16; the frozen text tower), P is rounded to half for the P.V product
// DMA (round 6; head dim 64, one chunk, bf16 - the ViT towers' and the Perceiver latents' self-attention): K and V rows go
// HBM -> LDS by LDS-DMA (`buffer_load_dwordx4 ... lds`), both as ROW images; the V^T fragments of the P.V product come out of
// gfx950's transpose read (`ds_read_b64_tr_b16`, the fused backward's addressing) instead of a transposed image that every
// thread built with 2-byte LDS stores from 12 loads held in registers.  The phase timeline of round 5 had 11.4 k of a
// workgroup's 33.2 k cycles in "load + stage" (profiles/r05_attn_phase_timeline.log): with the DMA the staging is the
// memory round trip and nothing else.  The shared last row's per-wave share runs BEFORE the tile loop and the wave that
// merges the partials does so after its own tiles, without a workgroup barrier at the end of the kernel.
template <int DH, bool TAILQ, bool MULTI, bool F16 = false, bool DMA = false>
__global__ void __launch_bounds__(NWMAX * 64, DH == 128 ? 2 : 4) attn_fwd_kernel(const AttnP p) {
  static_assert(!F16 || (!TAILQ && DH == 64), "half operands: head dim 64, no shared last row (the text tower's shape)");
  static_assert(!DMA || (DH == 64 && !MULTI && !F16), "LDS-DMA staging: head dim 64, one key chunk, bf16");
  constexpr bool VARLEN = false;
  [[maybe_unused]] constexpr long row0 = 0;      // (named by the discarded VARLEN branches of the body)
#include "vl_attn_fwd_body.inc"
}

// VARLEN (the packed text tower; half operands, head dim 64, causal): blockIdx.z = caption b, whose rows are
// start[b] .. start[b] + len[b] - 1 of the packed operands and of the output, Lq = Lk = len[b].  The same body on a copy of the
// arguments with the caption's lengths and the operand bases moved to its first packed row.  The query waves beyond len[b] only
// help staging; a workgroup whose first tile lies beyond it leaves at once.  KCT = the keys the LDS images hold (a multiple of 32
// that covers the longest caption): short captions get small images and many workgroups per CU instead of two, and only
// roundup(len[b], 32) rows are staged - with clamped row indices and no load under a lane condition (stage2<CLAMP>): the rows
// >= len[b] of the images are copies of the caption's last row, their scores are masked and their probabilities are exact zeros.
template <int KCT>
__global__ void __launch_bounds__(NWMAX * 64, 4) attn_fwd_varlen_kernel(const AttnPV pin) {
  static_assert(KCT % 32 == 0 && KCT >= 32 && KCT <= KC_DENSE, "LDS chunk: whole key tiles, at most the dense chunk");
  constexpr int DH = 64;
  constexpr bool TAILQ = false, MULTI = false, F16 = true, DMA = false, VARLEN = true;
  constexpr int KC = KCT;             // (shadow the file's constants: every LDS offset of the body follows this chunk)
  constexpr int VSP = KC + 8;
  AttnP pcap = pin;
  long row0;                          // the caption's first row in the packed output / lse
  {
    const int b = blockIdx.z;
    const int len = min(pin.vlen[b], KC);     // (the host sized KC from the longest caption; the plan gives len >= 1)
    if (len <= 0 || (int)((blockIdx.x * (blockDim.x >> 6)) * 32) >= len) return;      // uniform across the workgroup, before any barrier
    row0 = pin.vstart[b];
    pcap.Lq = pcap.Lk = pcap.lq_main = len;
    pcap.q.p += row0 * pin.q.sr; pcap.k.p += row0 * pin.k.sr; pcap.v.p += row0 * pin.v.sr;
    pcap.q.sb = pcap.k.sb = pcap.v.sb = 0;
  }
  const AttnP& p = pcap;
#include "vl_attn_fwd_body.inc"
}

}  // namespace

extern "C" int vl_set_error(const char* msg);

template <int DH, bool TAILQ, bool MULTI, bool F16 = false, bool DMA = false>
static int launch_fwd(const AttnP& p, int gx, int nwq, hipStream_t stream) {
  const size_t smem = (size_t)KC * DH * 2 + (size_t)DH * VSP * 2 + (size_t)NWMAX * 32 * 4 + (size_t)(KC / 32) * (2 + DH) * 4 +
                      (size_t)DH * 2;
  static const hipError_t attr = hipFuncSetAttribute((const void*)attn_fwd_kernel<DH, TAILQ, MULTI, F16, DMA>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (attr != hipSuccess) return vl_set_error(hipGetErrorString(attr));
  hipLaunchKernelGGL((attn_fwd_kernel<DH, TAILQ, MULTI, F16, DMA>), dim3(gx, p.H, p.B), dim3(nwq * 64), smem, stream, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}

template <int KCT>
static int launch_fwd_varlen(const AttnPV& p, int gx, int nwq, hipStream_t stream) {
  constexpr int DH = 64;             // (the body's LDS layout for a chunk of KCT keys)
  const size_t smem = (size_t)KCT * DH * 2 + (size_t)DH * (KCT + 8) * 2 + (size_t)NWMAX * 32 * 4 + (size_t)(KCT / 32) * (2 + DH) * 4 +
                      (size_t)DH * 2;
  static const hipError_t attr = hipFuncSetAttribute((const void*)attn_fwd_varlen_kernel<KCT>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (attr != hipSuccess) return vl_set_error(hipGetErrorString(attr));
  hipLaunchKernelGGL((attn_fwd_varlen_kernel<KCT>), dim3(gx, p.H, p.B), dim3(nwq * 64), smem, stream, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}

extern "C" int vl_attn_fwd_bf16(const void* q, const void* k, const void* v, const long* strides, void* out, float* lse,
                                int B, int H, int Lq, int Lk, int dh, float qscale, int causal, hipStream_t stream) {
  if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return vl_set_error("vl_attn_fwd_bf16: empty problem");
  if (dh != 32 && dh != 64 && !(dh > 64 && dh <= 128 && (dh & 7) == 0))
    return vl_set_error("vl_attn_fwd_bf16: head dim must be 32, 64, or a multiple of 8 in (64, 128] (run zero-padded to 128)");
  if (!strides) return vl_set_error("vl_attn_fwd_bf16: strides required");
  for (int i = 0; i < 9; ++i)
    if (strides[i] & 7) return vl_set_error("vl_attn_fwd_bf16: operand strides must be multiples of 8 elements (16-byte rows)");
  if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v)) & 15) return vl_set_error("vl_attn_fwd_bf16: operands must be 16-byte aligned");
  AttnP p{TV{(const bf16_t*)q, strides[0], strides[1], strides[2]}, TV{(const bf16_t*)k, strides[3], strides[4], strides[5]},
          TV{(const bf16_t*)v, strides[6], strides[7], strides[8]}, qscale, (bf16_t*)out, lse, B, H, Lq, Lk, causal, dh,
#ifdef VL_ATTN_PROF
          vl_attn_prof_buf,
#endif
          Lq};
  // one row beyond whole tiles (257 tokens): shared by the waves of the single workgroup instead of a ninth wave
  const bool tailq = (Lq % 32 == 1) && Lq > 32 && Lq - 1 <= NWMAX * 32 && Lk <= KC && (!causal || Lk <= Lq);
  if (tailq) p.lq_main = Lq - 1;
  const int qtiles = (p.lq_main + 31) / 32;
  const int nwq = qtiles < NWMAX ? qtiles : NWMAX;
  const int gx = (qtiles + nwq - 1) / nwq;
  const bool multi = Lk > KC;
#define VL_FWD(DHV)                                                                  \
  (tailq ? launch_fwd<DHV, true, false>(p, gx, nwq, stream)                          \
         : (multi ? launch_fwd<DHV, false, true>(p, gx, nwq, stream) : launch_fwd<DHV, false, false>(p, gx, nwq, stream)))
  // head dim 64, one key chunk: K / V staged by LDS-DMA, V^T fragments by transpose reads (DMA = true)
  if (dh == 64 && !multi)
    return tailq ? launch_fwd<64, true, false, false, true>(p, gx, nwq, stream) : launch_fwd<64, false, false, false, true>(p, gx, nwq, stream);
  return dh == 64 ? VL_FWD(64) : (dh == 32 ? VL_FWD(32) : VL_FWD(128));
#undef VL_FWD
}

// The same kernel on IEEE-half operands (q, k, v, out fp16; lse fp32): head dim 64, at most one LDS chunk of keys (288), any
// mask mode - the frozen text tower (77 tokens, causal; open_clip/model.py:528-540, transformer.py:241-252, 870-876).
extern "C" int vl_attn_fwd_f16(const void* q, const void* k, const void* v, const long* strides, void* out, float* lse,
                               int B, int H, int Lq, int Lk, int dh, float qscale, int causal, hipStream_t stream) {
  if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return vl_set_error("vl_attn_fwd_f16: empty problem");
  if (dh != 64) return vl_set_error("vl_attn_fwd_f16: head dim must be 64");
  if (Lk > KC) return vl_set_error("vl_attn_fwd_f16: at most 288 keys");
  if (!strides) return vl_set_error("vl_attn_fwd_f16: strides required");
  for (int i = 0; i < 9; ++i)
    if (strides[i] & 7) return vl_set_error("vl_attn_fwd_f16: operand strides must be multiples of 8 elements (16-byte rows)");
  if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v)) & 15) return vl_set_error("vl_attn_fwd_f16: operands must be 16-byte aligned");
  AttnP p{TV{(const bf16_t*)q, strides[0], strides[1], strides[2]}, TV{(const bf16_t*)k, strides[3], strides[4], strides[5]},
          TV{(const bf16_t*)v, strides[6], strides[7], strides[8]}, qscale, (bf16_t*)out, lse, B, H, Lq, Lk, causal, dh,
#ifdef VL_ATTN_PROF
          vl_attn_prof_buf,
#endif
          Lq};
  const int qtiles = (Lq + 31) / 32;
  const int nwq = qtiles < NWMAX ? qtiles : NWMAX;
  const int gx = (qtiles + nwq - 1) / nwq;
  return launch_fwd<64, false, false, true>(p, gx, nwq, stream);
}

// Causal self-attention of captions of DIFFERENT lengths packed one behind the other - the text tower on the rows up to each
// caption's pooled position only (vl_text_pack_plan).  q, k, v: column blocks of the packed in-projection output
// [rows, 3*width] fp16, strides = (head, row) element strides of q, k, v; caption b owns the rows start[b] .. start[b] + len[b] - 1
// of the operands and of out [rows, H*64] fp16; lse (optional) is [rows, H].  One workgroup per (caption, head) with
// ceil(max_len / 32) query waves (two workgroups of up to 8 waves beyond 256 rows).  max_len >= every len[b], <= 288.
extern "C" int vl_attn_fwd_varlen_f16(const void* q, const void* k, const void* v, const long* strides, const int* start,
                                      const int* len, void* out, float* lse, int B, int H, int max_len, int dh, float qscale,
                                      hipStream_t stream) {
  if (B <= 0 || H <= 0 || max_len <= 0) return vl_set_error("vl_attn_fwd_varlen_f16: empty problem");
  if (dh != 64) return vl_set_error("vl_attn_fwd_varlen_f16: head dim must be 64");
  if (max_len > KC) return vl_set_error("vl_attn_fwd_varlen_f16: at most 288 rows per caption");
  if (!q || !k || !v || !out) return vl_set_error("vl_attn_fwd_varlen_f16: q, k, v and out required");
  if (!strides || !start || !len) return vl_set_error("vl_attn_fwd_varlen_f16: strides, start and len required");
  for (int i = 0; i < 6; ++i)
    if (strides[i] & 7) return vl_set_error("vl_attn_fwd_varlen_f16: operand strides must be multiples of 8 elements (16-byte rows)");
  if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v)) & 15) return vl_set_error("vl_attn_fwd_varlen_f16: operands must be 16-byte aligned");
  AttnPV p{{TV{(const bf16_t*)q, 0, strides[0], strides[1]}, TV{(const bf16_t*)k, 0, strides[2], strides[3]},
            TV{(const bf16_t*)v, 0, strides[4], strides[5]}, qscale, (bf16_t*)out, lse, B, H, max_len, max_len, 1, dh,
#ifdef VL_ATTN_PROF
            vl_attn_prof_buf,
#endif
            max_len},
           start, len};
  const int qtiles = (max_len + 31) / 32;
  const int nwq = qtiles < NWMAX ? qtiles : NWMAX;
  const int gx = (qtiles + nwq - 1) / nwq;
  if (max_len <= 32) return launch_fwd_varlen<32>(p, gx, nwq, stream);
  if (max_len <= 96) return launch_fwd_varlen<96>(p, gx, nwq, stream);
  return launch_fwd_varlen<KC>(p, gx, nwq, stream);
}
