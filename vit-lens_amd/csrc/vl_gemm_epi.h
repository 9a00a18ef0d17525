// Epilogue arithmetic of the bf16 NT GEMMs, once: what vl_gemm.hip (direct, fp32-transpose and 16-byte transpose epilogues),
// vl_gemm_pp.hip and vl_gemm_park.hip do with an output value between the accumulator and the store, and the host-side rules
// (which act / out2 combinations the bf16 family takes, which template ACT code a launch means) that go with it.  The kernels
// keep what is theirs: addressing, the LDS transposes, the stores and their order, LayerNorm folding, row statistics, fp16
// packing, park's GEGLU / DGEGLU slab forms.
//
// GELU, its derivative and QuickGELU are evaluated on PAIRS (gelu_erf2 / gelu_erf_grad2 / qgelu2, vl_common.h); the pair forms
// round like the scalar ones, bit for bit (tests/test_gelu_pairs_host.py, tests/test_qgelu_pairs_host.py).  One exception,
// measured: QuickGELU in front of the pack in vl_gemm.hip's kernels (epi_act2, QG_PAIRS).
//
// Template ACT codes (EPI_BF16 unless said otherwise):
//   0 none, 1 GELU, 2 ReLU (also EPI_RES_BF16: after the add), 3 GELU with the pre-activation also written to out2,
//   4 GELU with gelu'(pre-activation) written to out2 (EPI_DGELU: the aux operand IS the saved derivative, of either activation),
//   5 QuickGELU, 6 QuickGELU with qgelu'(pre-activation) written to out2.
//   vl_gemm_park.hip only: 10 + code = the code with LayerNorm folded into the epilogue, 20 = EPI_RES_BF16 + partial row statistics.
// 1, 2 and 5 act on the fp32 values BEFORE they are packed (epi_act2 / epi_prepack).  Behind a 16-byte transpose (epi_post8:
// store_tile_lds16, vl_gemm_pp.hip, vl_gemm_park.hip) 3, 4, 6 and the epilogues with a second operand of the output's shape act on
// the bf16-ROUNDED values - the rounding points of the reference's autocast (bf16 linear output, then the add / activation).
// Without one (epi_direct4: store_tile and the fp32 transpose) only 4 and 6 do: 3 stores bf16(v) to out2 and applies GELU to the
// fp32 v, and the residual add, ReLU after it, the dGELU product, GEGLU and DGEGLU act on the fp32 v, with ONE rounding at the
// store (at most one bf16 ulp from the other form; the _DSAVE codes the trainers use are the same either way).  The table, and
// the tests that tell the two forms apart: tests/test_hip_gemm_families.py.
//
// A new activation: its arithmetic in vl_common.h (scalar and pair form, a host test that the two agree), its VL_ACT_* code in
// epi_act_code and epi_bf16_family_ok, its branch in epi_act2 and / or epi_post8, in epi_direct4 and in store_tile_lds16's
// runtime dispatch, and one line in each of the two launch tables (vl_gemm_pp_launch, vl_gemm_park_launch).  Then
// tools/kernel_text_diff.py against the parent: how a value is handed to a helper here decides register numbers two screens away.
#pragma once
#include "vl_gemm_common.h"

namespace {

// (epilogue, VL_ACT_* code, out2 given, LayerNorm folded, row statistics wanted) -> template ACT code; -1: no such kernel
constexpr int epi_act_code(int epi, int act, bool out2, bool lnf, bool stats) {
  if (epi == EPI_BF16) {
    int a = 0;                // (an act the epilogue does not take is ignored)
    if (act == VL_ACT_GELU) a = out2 ? 3 : 1;
    else if (act == VL_ACT_RELU || act == VL_ACT_GELU_DSAVE || act == VL_ACT_QGELU || act == VL_ACT_QGELU_DSAVE) a = act;
    if (!lnf) return a;
    return (a == act && a != 2) ? 10 + a : -1;      // folded: none, GELU, QuickGELU and the two _DSAVE codes
  }
  if (epi == EPI_RES_BF16) return stats ? 20 : act == VL_ACT_RELU ? 2 : 0;
  if (epi == EPI_DGELU) return act == VL_ACT_GELU_DSAVE ? 4 : 0;
  return 0;
}

// What vl_gemm_pp.hip and vl_gemm_park.hip both ask of a bf16-output problem (EPI_BF16, EPI_RES_BF16, EPI_DGELU, and park's
// GEGLU pair); tile multiples and the shortest K are each kernel's own
inline bool epi_bf16_family_ok(int epi, const GemmP& p) {
  if ((p.K & 63) || p.M <= 0 || p.N <= 0) return false;
  if (p.res_div != 1) return false;
  if (epi == EPI_RES_BF16 && p.act != 0) return false;
  if (epi == EPI_BF16 && p.out2 && p.act != VL_ACT_GELU && p.act != VL_ACT_GELU_DSAVE && p.act != VL_ACT_QGELU_DSAVE) return false;
  if (epi == EPI_BF16 && (p.act == VL_ACT_GELU_DSAVE || p.act == VL_ACT_QGELU_DSAVE) && !p.out2) return false;
  if (epi == EPI_DGELU && (p.act == VL_ACT_QGELU || p.act == VL_ACT_QGELU_DSAVE)) return false;   // (the dispatcher passes the saved form as 4)
  if (p.ldo & 7) return false;
  // 16-byte accesses on every operand
  if (((uintptr_t)p.A | (uintptr_t)p.W) & 15) return false;
  if (((uintptr_t)p.out | (uintptr_t)p.res | (uintptr_t)p.out2) & 15) return false;
  return true;
}

// ---- the activation of a PAIR of fp32 values in front of the pack (ACT 1, 2, 5; every other (EPI, ACT): nothing), and of four
// (V: f32x4 or float[4]).  QG_PAIRS = false: QuickGELU one value at a time - vl_gemm.hip's kernels, which lost 2-3 % on the c_fc
// shape with qgelu2 (packed instructions take no |x| modifier: a v_and per value and no instruction saved;
// profiles/gemm_epilogue_ab.log).  The same bits either way (tests/test_qgelu_pairs_host.py) ----
template <int EPI, int ACT, bool QG_PAIRS = true>
__device__ __forceinline__ vl_f32x2 epi_act2(vl_f32x2 x) {
  if constexpr (EPI == EPI_BF16 && ACT == 1) return gelu_erf2(x);
  else if constexpr (EPI == EPI_BF16 && ACT == 2) return vl_f32x2{fmaxf(x[0], 0.f), fmaxf(x[1], 0.f)};
  else if constexpr (EPI == EPI_BF16 && ACT == 5 && QG_PAIRS) return qgelu2(x);
  else if constexpr (EPI == EPI_BF16 && ACT == 5) return vl_f32x2{qgelu(x[0]), qgelu(x[1])};
  else return x;
}
template <int EPI, int ACT, bool QG_PAIRS = true, class V>
__device__ __forceinline__ void epi_prepack(V& v) {
  if constexpr (EPI == EPI_BF16 && (ACT == 1 || ACT == 2 || ACT == 5)) {
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
      const vl_f32x2 y = epi_act2<EPI, ACT, QG_PAIRS>(vl_f32x2{v[e], v[e + 1]});
      v[e] = y[0]; v[e + 1] = y[1];
    }
  }
}

// ---- eight bf16 values (w) behind the transpose, with the eight values of the second operand (rr: residual, saved
// pre-activation or saved derivative; read only by EPI_RES_BF16 / EPI_DGELU): w becomes the output, d the derivative that
// ACT 4 / 6 leave in out2 (untouched otherwise; the out2 of ACT 3 is w as it came in: the caller stores it first) ----
template <int EPI, int ACT>
__device__ __forceinline__ void epi_post8(u32x4& w, const u32x4& rr, u32x4& d) {
  if constexpr (EPI == EPI_BF16 && ACT == 3) {
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = pack2bf(gelu_erf2(unpack2bf(w[e])));
  } else if constexpr (EPI == EPI_BF16 && ACT == 4) {              // d = gelu'(pre) for the dX GEMM of the backward
#pragma unroll
    for (int e = 0; e < 4; ++e) { unsigned int y, g; gelu_and_grad_pk(w[e], y, g); w[e] = y; d[e] = g; }
  } else if constexpr (EPI == EPI_BF16 && ACT == 6) {              // d = qgelu'(pre)
#pragma unroll
    for (int e = 0; e < 4; ++e) { unsigned int y, g; qgelu_and_grad_pk(w[e], y, g); w[e] = y; d[e] = g; }
  } else if constexpr (EPI == EPI_RES_BF16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float lo = bf2f((bf16_t)(w[e] & 0xffff)) + bf2f((bf16_t)(rr[e] & 0xffff));
      float hi = bf2f((bf16_t)(w[e] >> 16)) + bf2f((bf16_t)(rr[e] >> 16));
      if constexpr (ACT == 2) { lo = fmaxf(lo, 0.f); hi = fmaxf(hi, 0.f); }
      w[e] = pack2bf(lo, hi);
    }
  } else if constexpr (EPI == EPI_DGELU && ACT == 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = mul_pk_bf16(w[e], rr[e]);     // rr = the derivative saved by the forward
  } else if constexpr (EPI == EPI_DGELU) {
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = pack2bf(unpack2bf(w[e]) * gelu_erf_grad2(unpack2bf(rr[e])));
  }
}

// ---- four consecutive fp32 values v (alpha and bias applied) of row m, columns n .. n + 3, without a 16-byte transpose:
// the whole epilogue of vl_gemm.hip's runtime-act kernels, loads of the second operand and stores included.  EPI_ may be
// EPI_BF16_QG (EPI_BF16 that also carries the QuickGELU codes) ----
template <int EPI_>
__device__ __forceinline__ void epi_direct4(const GemmP& p, float (&v)[4], int m, int n) {
  constexpr int EPI = epi_base(EPI_);
  constexpr bool QG = (EPI_ == EPI_BF16_QG);
  if constexpr (EPI == EPI_BF16) {
    if (p.act == VL_ACT_GELU_DSAVE) {          // GELU of the bf16-rounded pre-activation, out2 = gelu' of the same (bf16)
      unsigned int y0, g0, y1, g1;
      gelu_and_grad_pk(pack2bf(v[0], v[1]), y0, g0);
      gelu_and_grad_pk(pack2bf(v[2], v[3]), y1, g1);
      const u32x2 o = {y0, y1}, d = {g0, g1};
      *(u32x2*)((bf16_t*)p.out2 + (size_t)m * p.ldo + n) = d;
      *(u32x2*)((bf16_t*)p.out + (size_t)m * p.ldo + n) = o;
      return;
    }
    if (QG && p.act == VL_ACT_QGELU_DSAVE) {   // the QuickGELU twin (a block of its own, as it was: folded into the one above, the tail kernel lost 2 %)
      unsigned int y0, g0, y1, g1;
      qgelu_and_grad_pk(pack2bf(v[0], v[1]), y0, g0);
      qgelu_and_grad_pk(pack2bf(v[2], v[3]), y1, g1);
      const u32x2 o = {y0, y1}, d = {g0, g1};
      *(u32x2*)((bf16_t*)p.out2 + (size_t)m * p.ldo + n) = d;
      *(u32x2*)((bf16_t*)p.out + (size_t)m * p.ldo + n) = o;
      return;
    }
    if (p.act == VL_ACT_GELU) {
      if (p.out2) {
        u32x2 o2; o2[0] = pack2bf(v[0], v[1]); o2[1] = pack2bf(v[2], v[3]);
        *(u32x2*)((bf16_t*)p.out2 + (size_t)m * p.ldo + n) = o2;
      }
      epi_prepack<EPI_BF16, 1>(v);
    } else if (p.act == VL_ACT_RELU) {
      epi_prepack<EPI_BF16, 2>(v);
    } else if (QG && p.act == VL_ACT_QGELU) {
      epi_prepack<EPI_BF16, 5, false>(v);
    }
    u32x2 o; o[0] = pack2bf(v[0], v[1]); o[1] = pack2bf(v[2], v[3]);
    *(u32x2*)((bf16_t*)p.out + (size_t)m * p.ldo + n) = o;
  } else if constexpr (EPI == EPI_F32) {
    f32x4 o = {v[0], v[1], v[2], v[3]};
    *(f32x4*)((float*)p.out + (size_t)m * p.ldo + n) = o;
  } else if constexpr (EPI == EPI_RES_F32) {
    const f32x4 r = *(const f32x4*)((const float*)p.res + (size_t)m * p.ldo + n);
    f32x4 o = {v[0] + r[0], v[1] + r[1], v[2] + r[2], v[3] + r[3]};
    *(f32x4*)((float*)p.out + (size_t)m * p.ldo + n) = o;
  } else if constexpr (EPI == EPI_RES_BF16) {
    const u32x2 r = *(const u32x2*)((const bf16_t*)p.res + (size_t)((m + p.m_off) / p.res_div) * p.ldo + n);
    v[0] += bf2f((bf16_t)(r[0] & 0xffff)); v[1] += bf2f((bf16_t)(r[0] >> 16));
    v[2] += bf2f((bf16_t)(r[1] & 0xffff)); v[3] += bf2f((bf16_t)(r[1] >> 16));
    if (p.act == VL_ACT_RELU) epi_prepack<EPI_BF16, 2>(v);
    u32x2 o; o[0] = pack2bf(v[0], v[1]); o[1] = pack2bf(v[2], v[3]);
    *(u32x2*)((bf16_t*)p.out + (size_t)m * p.ldo + n) = o;
  } else if constexpr (EPI == EPI_DGELU) {
    const u32x2 r = *(const u32x2*)((const bf16_t*)p.res + (size_t)m * p.ldo + n);
    const bool saved = p.act == VL_ACT_GELU_DSAVE;      // res = the derivative itself (left by a _DSAVE forward)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const vl_f32x2 u = unpack2bf(r[h]);
      const vl_f32x2 g = saved ? u : gelu_erf_grad2(u);
      v[2 * h] *= g[0]; v[2 * h + 1] *= g[1];
    }
    u32x2 o; o[0] = pack2bf(v[0], v[1]); o[1] = pack2bf(v[2], v[3]);
    *(u32x2*)((bf16_t*)p.out + (size_t)m * p.ldo + n) = o;
  } else if constexpr (EPI == EPI_GEGLU) {
    // interleaved rows: (a_j, gate_j, a_j+1, gate_j+1)
    if (p.out2) {   // pre-activation kept for the backward: bf16 [M, N], row stride 2*ldo
      u32x2 o2; o2[0] = pack2bf(v[0], v[1]); o2[1] = pack2bf(v[2], v[3]);
      *(u32x2*)((bf16_t*)p.out2 + (size_t)m * (2 * p.ldo) + n) = o2;
    }
    const float o0 = v[0] * gelu_erf(v[1]);
    const float o1 = v[2] * gelu_erf(v[3]);
    *(unsigned int*)((bf16_t*)p.out + (size_t)m * p.ldo + (n >> 1)) = pack2bf(o0, o1);
  } else if constexpr (EPI == EPI_DGEGLU) {
    const u32x4 hv = *(const u32x4*)((const bf16_t*)p.res + (size_t)m * p.ldo + 2 * n);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = bf2f((bf16_t)(hv[e] & 0xffff)), g = bf2f((bf16_t)(hv[e] >> 16));
      o[e] = pack2bf(v[e] * gelu_erf(g), v[e] * a * gelu_erf_grad(g));
    }
    *(u32x4*)((bf16_t*)p.out + (size_t)m * p.ldo + 2 * n) = o;
  }
}

}  // namespace
