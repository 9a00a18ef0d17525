// Audio at any sample rate and the training-time transform after the filterbank, on the GPU.
//
//   vl_resample_sinc  = torchaudio.functional.resample at its defaults (sinc_interp_hann, lowpass_filter_width 6,
//                       rolloff 0.99), the resampler every loader of the reference runs when a file is not at 16 kHz
//                       (open_clip/modal_audio/processors/at_processor.py:227-234, 365-369, 877-881).  With o = orig/gcd,
//                       n = new/gcd, base = min(o, n) * 0.99, W = ceil(6 o / base):
//                           out[j] = sum_m x[m] h(m/o - j/n),   h(tau) = sinc(pi t) cos^2(pi t / 12) base/o,  t = clamp(tau base, -6, 6)
//                       with zeros outside the recording and ceil(n len / o) outputs.  In polyphase form (p = j mod n,
//                       i = j div n) the taps of phase p sit at the inputs i o - W .. i o + W + o - 1, but all except one run
//                       of at most 2W of them are zero, so the host (vitlens_hip/audio.py: sinc_resample_table) hands over a
//                       COMPACT table: per phase the first tap's offset and K = 2W + 1 taps - 35 instead of the 475 the dense
//                       convolution multiplies for 44.1 -> 16 kHz.
//   vl_fbank_augment  = the transform of ASTProcessorTrain after the filterbank (:336-362) in one pass: FrequencyMasking /
//                       TimeMasking with 0, Normalize(mean, std), + rand(T, F) * amp, roll along time.  The random draws
//                       of the masks, amp and roll are the host's; the noise field is Philox4x32-10 (Salmon et al., SC'11)
//                       keyed by the sample's seed, counter = element index / 4.
//
// torchaudio is not installed anywhere, so like the filterbank this path is "parity unpinned": restated from the published
// algorithm and checked against a float64 numpy restatement (tests/resample_ref.py), not against the library.
#include "vl_common.h"
#include "vl_philox.h"
#include "vitlens_hip.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_TILE = 2048;        // outputs per workgroup, halved until the input span fits
constexpr int RS_MIN_TILE = 64;
constexpr int RS_SPAN_CAP = 8192;        // floats of input one workgroup stages (32 KiB)
constexpr int RS_TABLE_CAP = 8192;       // n * (K + 1) words up to which the tap table is staged too (32 KiB)

// One workgroup = `tile` consecutive outputs of one row.  The input span they read goes through LDS once (zeros where the
// index is outside the recording: no global read outside [0, n_in)), the tap table too when it fits (TAPS_LDS), else it is
// read through L2.  Every output is K fused multiply-adds in ascending tap order over the same values wherever the tile
// starts, so a window of a recording is bit-identical to the same samples of a whole-file call.
template <bool TAPS_LDS>
__global__ void __launch_bounds__(RS_THREADS) resample_sinc_kernel(const float* in, long in_stride, long n_in, const int* offsets,
                                                                   const float* taps, int o, int n, int K, float* out,
                                                                   long out_stride, long out_first, long n_out, int tile, int span) {
  extern __shared__ float s_rs[];
  float* xs = s_rs;                                        // [span]
  float* ts = xs + span;                                   // [n * K]   (TAPS_LDS)
  int* os = reinterpret_cast<int*>(ts + (TAPS_LDS ? n * K : 0));   // [n]
  const int tid = threadIdx.x, W = (K - 1) / 2;
  const long r0 = (long)blockIdx.x * tile;                 // first output of the tile, relative to out_first
  const long left = n_out - r0;
  const int cnt = left < tile ? (int)left : tile;
  const long j0 = out_first + r0;
  const long i0 = j0 / n;
  const int p0 = (int)(j0 - i0 * n);
  const long m0 = i0 * o - W;                              // input index of xs[0]
  const float* x = in + (size_t)blockIdx.y * in_stride;
  const int need = ((p0 + cnt - 1) / n) * o + 2 * W + o;   // <= span (the host sized span for p0 = n - 1, cnt = tile)
  for (int s = tid; s < need; s += RS_THREADS) {
    const long m = m0 + s;
    xs[s] = (m >= 0 && m < n_in) ? x[m] : 0.f;
  }
  if (TAPS_LDS) {
    for (int s = tid; s < n * K; s += RS_THREADS) ts[s] = taps[s];
    for (int s = tid; s < n; s += RS_THREADS) os[s] = offsets[s];
  }
  __syncthreads();
  float* y = out + (size_t)blockIdx.y * out_stride + r0;
  for (int r = tid; r < cnt; r += RS_THREADS) {
    const int q = p0 + r, di = q / n, p = q - di * n;
    int off = TAPS_LDS ? os[p] : offsets[p];
    off = off < 0 ? 0 : (off > o - 1 ? o - 1 : off);       // the table's contract; keeps every LDS index below `need`
    const float* xp = xs + di * o + off;
    const float* tp = (TAPS_LDS ? ts : taps) + (size_t)p * K;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(xp[k], tp[k], acc);
    y[r] = acc;
  }
}

struct AugParams {             // one per sample, written by the host (vitlens_hip/audio.py: AUGMENT_DTYPE)
  int f0, fw, t0, tw;          // masks [f0, f0 + fw) over mel bins, [t0, t0 + tw) over frames
  float amp;
  int roll;
  unsigned long long seed;
};
static_assert(sizeof(AugParams) == 32, "AugParams is 32 bytes on both sides of the ABI");

__device__ __forceinline__ float aug_value(float x, bool masked, float mean, float std, float amp, uint32_t bits) {
#pragma clang fp contract(off)            // mask, Normalize, + amp * u as the separate roundings torch makes
  const float v = __fdiv_rn(__fsub_rn(masked ? 0.f : x, mean), std);            // mask with 0, then Normalize: a true division
  return __fadd_rn(v, __fmul_rn(amp, (float)(bits >> 8) * 5.9604644775390625e-08f));      // + amp * u,  u = (bits >> 8) 2^-24
}

// One thread = four consecutive elements of a sample's [T, F] plane = one Philox block.  VEC: F % 4 == 0 and 16-byte
// aligned planes, the four sit in one row: one 16-byte load and one 16-byte store.
template <bool VEC>
__global__ void __launch_bounds__(256) fbank_augment_kernel(const float* in, float* out, int T, int F, const AugParams* params,
                                                            float mean, float std) {
  const AugParams P = params[blockIdx.y];
  const long plane = (long)T * F;
  const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= plane) return;
  const float* x = in + (size_t)blockIdx.y * plane;
  float* y = out + (size_t)blockIdx.y * plane;
  const int roll = ((P.roll % T) + T) % T;
  const unsigned long long g = (unsigned long long)(e0 >> 2);
  const U4 rnd = philox4x32_10(U4{(uint32_t)g, (uint32_t)(g >> 32), 0u, 0u}, (uint32_t)P.seed, (uint32_t)(P.seed >> 32));
  const uint32_t bits[4] = {rnd.x, rnd.y, rnd.z, rnd.w};
  if (VEC) {
    const int t = (int)(e0 / F), f = (int)(e0 - (long)t * F);
    const bool tm = t >= P.t0 && t < P.t0 + P.tw;
    const float4 v = *reinterpret_cast<const float4*>(x + e0);
    const float xv[4] = {v.x, v.y, v.z, v.w};
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = aug_value(xv[c], tm || (f + c >= P.f0 && f + c < P.f0 + P.fw), mean, std, P.amp, bits[c]);
    int tr = t + roll;
    tr = tr >= T ? tr - T : tr;
    *reinterpret_cast<float4*>(y + (long)tr * F + f) = float4{r[0], r[1], r[2], r[3]};
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long e = e0 + c;
      if (e >= plane) break;
      const int t = (int)(e / F), f = (int)(e - (long)t * F);
      const bool masked = (t >= P.t0 && t < P.t0 + P.tw) || (f >= P.f0 && f < P.f0 + P.fw);
      int tr = t + roll;
      tr = tr >= T ? tr - T : tr;
      y[(long)tr * F + f] = aug_value(x[e], masked, mean, std, P.amp, bits[c]);
    }
  }
}

}  // namespace

extern "C" int vl_set_error(const char* msg);

extern "C" int vl_resample_sinc(const float* in, long in_stride, int batch, long n_in, const int* offsets, const float* taps, int o,
                                int n, int K, float* out, long out_stride, long out_first, long n_out, hipStream_t stream) {
  if (batch <= 0 || batch > 65535 || n_in <= 0 || o <= 0 || n <= 0 || K <= 0 || !(K & 1) || in_stride < n_in)
    return vl_set_error("vl_resample_sinc: bad shape (batch in [1, 65535], n_in, o, n >= 1, K = 2W + 1, in_stride >= n_in)");
  if (n_in > (0x7fffffffffffffffL - o) / n) return vl_set_error("vl_resample_sinc: n * n_in overflows");
  const long total = (n_in * n + o - 1) / o;                            // ceil(n n_in / o)
  if (out_first < 0 || n_out <= 0 || out_first > total - n_out || out_stride < n_out)
    return vl_set_error("vl_resample_sinc: the output window must lie inside [0, ceil(n * n_in / o)) and out_stride >= n_out");
  const bool taps_lds = (long)n * (K + 1) <= RS_TABLE_CAP;
  int tile = RS_MAX_TILE;
  auto span_of = [&](int t) { return ((long)(n - 1 + t - 1) / n) * o + (K - 1) + o; };
  while (tile > RS_MIN_TILE && span_of(tile) > RS_SPAN_CAP) tile >>= 1;
  if (span_of(tile) > RS_SPAN_CAP)
    return vl_set_error("vl_resample_sinc: the rate ratio is too irregular (o = orig / gcd above a few thousand): the input span of "
                        "one tile does not fit the staging buffer");
  const long tiles = (n_out + tile - 1) / tile;
  if (tiles > 0x7fffffffL) return vl_set_error("vl_resample_sinc: output window too long for one launch");
  const int span = (int)span_of(tile);
  const size_t smem = ((size_t)span + (taps_lds ? (size_t)n * (K + 1) : 0)) * sizeof(float);
  const dim3 grid((unsigned)tiles, (unsigned)batch);
  if (taps_lds)
    hipLaunchKernelGGL(resample_sinc_kernel<true>, grid, dim3(RS_THREADS), smem, stream, in, in_stride, n_in, offsets, taps, o, n, K,
                       out, out_stride, out_first, n_out, tile, span);
  else
    hipLaunchKernelGGL(resample_sinc_kernel<false>, grid, dim3(RS_THREADS), smem, stream, in, in_stride, n_in, offsets, taps, o, n, K,
                       out, out_stride, out_first, n_out, tile, span);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}

extern "C" int vl_fbank_augment(const float* in, float* out, int batch, int T, int F, const void* params, float mean, float std,
                                hipStream_t stream) {
  if (batch <= 0 || batch > 65535 || T <= 0 || F <= 0 || std == 0.f || in == out)
    return vl_set_error("vl_fbank_augment: bad shape (batch in [1, 65535], T, F >= 1, std != 0, out of place: the roll moves rows)");
  const long groups = ((long)T * F + 3) / 4;
  if (groups > 0x7fffffffL * 256L) return vl_set_error("vl_fbank_augment: plane too large");
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)batch);
  const bool vec = F % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(fbank_augment_kernel<true>, grid, dim3(256), 0, stream, in, out, T, F, (const AugParams*)params, mean, std);
  else
    hipLaunchKernelGGL(fbank_augment_kernel<false>, grid, dim3(256), 0, stream, in, out, T, F, (const AugParams*)params, mean, std);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}
