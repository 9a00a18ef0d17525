// Host build of the QuickGELU helpers of vit-lens_amd/csrc/vl_common.h (tests/test_qgelu_pairs_host.py): the scalar forms
// (qgelu, qgelu_grad), the packed-pair forms (qgelu2, qgelu_grad_from_parts2) and qgelu_and_grad_pk against fp64
// x * sigmoid(1.702 x) and s + 1.702 x s (1 - s) on every finite bf16 value, in both lanes.  The device builtins are replaced by
// their host meanings.  Bound: one bf16 ulp of the fp64 value (the spacing of bf16 at that magnitude; 2^-133 below the normal
// range); no NaN or infinity anywhere; the packed forms equal the scalar forms bit for bit.  Host arithmetic: exp2f and the
// division keep denormals, the device exponential flushes them (from |x| ~ 51 on the device gives -0 / 0 where the true
// magnitudes are below 1e-36).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#define __device__
#define __forceinline__ inline
static inline float vl_host_rcp(float x) { return 1.0f / x; }
static inline float vl_host_med3(float a, float b, float c) { return fminf(fmaxf(a, b), c); }
static inline float __shfl_xor(float v, int, int) { return v; }
#define __builtin_amdgcn_rcpf vl_host_rcp
#define __builtin_amdgcn_exp2f exp2f
#define __builtin_amdgcn_fmed3f vl_host_med3
#include VL_COMMON_HOST_H

static inline uint32_t bits(float f) { return __builtin_bit_cast(uint32_t, f); }

static double ref_s(double x) { return x >= 0 ? 1.0 / (1.0 + exp(-1.702 * x)) : exp(1.702 * x) / (1.0 + exp(1.702 * x)); }
static double ref_y(double x) { return x * ref_s(x); }
static double ref_d(double x) { const double s = ref_s(x), c = x >= 0 ? exp(-1.702 * x) / (1.0 + exp(-1.702 * x)) : 1.0 / (1.0 + exp(1.702 * x)); return s + 1.702 * x * s * c; }
static double ulp_bf16(double v) {
  int e;
  if (v == 0) return ldexp(1.0, -133);
  frexp(fabs(v), &e);                      // |v| = m 2^e, m in [0.5, 1): exponent of the leading bit = e - 1
  e -= 1;
  if (e < -126) e = -126;
  return ldexp(1.0, e - 7);
}
static int within(float got, double want) { return isfinite(got) && fabs((double)got - want) <= ulp_bf16(want); }

int main() {
  long bad = 0, n = 0;
  double worst_y = 0, worst_d = 0;
  for (unsigned lo = 0; lo < 65536; ++lo) {
    const unsigned hi = (lo * 40503u + 12345u) & 0xffff;           // a different value, usually of the other sign, in the high lane
    if (((lo >> 7) & 0xff) == 0xff || ((hi >> 7) & 0xff) == 0xff) continue;     // infinities / NaNs
    const unsigned w = lo | (hi << 16);
    const float a = bf2f((bf16_t)lo), b = bf2f((bf16_t)hi);
    const vl_f32x2 x = {a, b};
    const QGeluParts2 p2 = qgelu_parts2(x);
    const vl_f32x2 y2 = qgelu2(x), g2 = qgelu_grad_from_parts2(x, p2);
    unsigned y, d;
    qgelu_and_grad_pk(w, y, d);
    const float ya = qgelu(a), yb = qgelu(b), da = qgelu_grad(a), db = qgelu_grad(b);
    int ok = bits(y2[0]) == bits(ya) && bits(y2[1]) == bits(yb) && bits(g2[0]) == bits(da) && bits(g2[1]) == bits(db) &&
             y == pack2bf(ya, yb) && d == pack2bf(da, db);
    // against fp64: the fp32 values and the stored bf16 values
    const float sy0 = bf2f((bf16_t)(y & 0xffff)), sy1 = bf2f((bf16_t)(y >> 16)), sd0 = bf2f((bf16_t)(d & 0xffff)), sd1 = bf2f((bf16_t)(d >> 16));
    ok = ok && within(ya, ref_y(a)) && within(yb, ref_y(b)) && within(da, ref_d(a)) && within(db, ref_d(b));
    ok = ok && within(sy0, ref_y(a)) && within(sy1, ref_y(b)) && within(sd0, ref_d(a)) && within(sd1, ref_d(b));
    // the saturated ends: x / 1 at large positive x, (-)0 / 0 at large negative x
    if (a > 60.0f) ok = ok && ya == a && da == 1.0f;
    if (a < -120.0f) ok = ok && ya == 0.0f && da == 0.0f;
    const double ey = fabs((double)sy0 - ref_y(a)) / ulp_bf16(ref_y(a)), ed = fabs((double)sd0 - ref_d(a)) / ulp_bf16(ref_d(a));
    if (ey > worst_y) worst_y = ey;
    if (ed > worst_d) worst_d = ed;
    if (!ok && bad++ < 5) printf("mismatch at w=%08x a=%g: y %g (want %.9g) d %g (want %.9g)\n", w, a, ya, ref_y(a), da, ref_d(a));
    ++n;
  }
  printf("worst stored error in bf16 ulps: qgelu %.3f qgelu' %.3f\n", worst_y, worst_d);
  printf("checked=%ld bad=%ld\n", n, bad);
  return bad != 0;
}
