// Audio mix-up (the reference's open_clip/modal_audio/datasets.py:279-326) and the assembly of a batch's training clips on
// the GPU.
//
//   vl_wave_clip_mix  = audio_get_clip (at_processor.py:193-224) for every row of a batch, and for a row with a partner
//                       `mix = lam * wf + (1 - lam) * sec_wf; mix -= mix.mean()` on top, in one launch from recordings that
//                       are already on the device.  A clip is never materialised: cut, repeat and crop are the index
//                           a[c][t] = src[off + c len + (start + t) mod len],   t < n
//                       (doubling a short cut is a periodic extension, and the crop is a shift of it).
//   vl_mix_rows       = the same mix of the two samples' frames (datasets.py:318-321), row by row.
//
// Arithmetic.  torch evaluates `lam * a + mu * b` as three separately rounded float32 operations, so the kernels do: every
// function that forms a product next to a sum is compiled with contraction off, and the library's listing holds no fused
// multiply-add for them.
//
// Summation order of a mean over N = ch * n elements (sum_block).  The elements are taken in flat order e = c n + t, four
// at a time: chunk k = elements 4k .. 4k + 3.  Thread i of the 256 adds the chunks i, i + 256, i + 512, ... in that order into
// four accumulators, one per position in the chunk; then (acc0 + acc1) + (acc2 + acc3); then the 64 lanes of a wave in a
// 6-step butterfly; then the four waves as (w0 + w1) + (w2 + w3).  Nothing depends on timing, so two runs agree bit for
// bit, and an element passes through at most  K = ceil(ceil(N / 4) / 256) + 10  additions
// (vitlens_hip.audio.mix_mean_chain).  The mean is that sum divided by float(N), one true division.
#include "vl_common.h"
#include "vitlens_hip.h"

namespace {

constexpr int MIX_THREADS = 256;

struct MixRec {                // one per output row, written by the host (vitlens_hip/audio.py: MIX_DTYPE)
  int off_a, ch_a, len_a, start_a;     // clip A: ch_a rows of len_a samples at float offset off_a of src, read from start_a
  int off_b, ch_b, len_b, start_b;     // the partner, ch_b = 0: none
  float lam, mu;                       // float32 roundings of lambda and of the double 1 - lambda
};
static_assert(sizeof(MixRec) == 40, "MixRec is 40 bytes on both sides of the ABI");

// Four consecutive samples t0 .. t0 + 3 of one periodic row: one 16-byte load where they do not wrap and sit on a 16-byte
// boundary, scalar loads otherwise (the head and tail of a row that starts off the boundary, every wrap).  No index leaves
// [0, len).
__device__ __forceinline__ void load4(const float* row, unsigned len, unsigned start, unsigned t0, float v[4]) {
  unsigned i0 = start + t0;            // start < len <= 2^31 - 1 and t0 < n <= 2^31 - 1
  if (i0 >= len) i0 %= len;
  if (len - i0 >= 4u && ((uintptr_t)(row + i0) & 15) == 0) {
    const float4 x = *reinterpret_cast<const float4*>(row + i0);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    return;
  }
#pragma unroll
  for (unsigned j = 0; j < 4; ++j) {
    unsigned i = i0 + j;
    if (i >= len) i %= len;
    v[j] = row[i];
  }
}

__device__ __forceinline__ float load1(const float* row, unsigned len, unsigned start, unsigned t) {
  unsigned i = start + t;
  if (i >= len) i %= len;
  return row[i];
}

struct Clip {
  const float* base;                   // src + off
  unsigned ch, len, start;
  __device__ __forceinline__ const float* row(unsigned c) const { return base + (size_t)(ch == 1 ? 0 : c) * len; }   // torch's broadcast
};

// One mixed value: lam a' + mu b' in three roundings, a' = a - mA and b' = b - mB rounded before.
__device__ __forceinline__ float mix_value(float a, float b, float mA, float mB, float lam, float mu) {
#pragma clang fp contract(off)
  const float da = a - mA, db = b - mB;
  const float pa = lam * da, pb = mu * db;
  return pa + pb;
}

// The block's sum of per-thread accumulators, in the order the file comment gives; every thread returns the same value.
__device__ __forceinline__ float sum_block(const float acc[4], float* part) {
#pragma clang fp contract(off)
  float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  s = wave_sum(s);
  __syncthreads();                     // the previous sum's readers are done with `part`
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

// sum over the ch * n elements of a clip in flat order
__device__ __forceinline__ float clip_sum(const Clip& A, unsigned n, float* part) {
  const unsigned N = A.ch * n, chunks = (N + 3u) / 4u;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (unsigned k = threadIdx.x; k < chunks; k += MIX_THREADS) {
    const unsigned e0 = 4u * k, c = e0 / n, t0 = e0 - c * n;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (n - t0 >= 4u) {
      load4(A.row(c), A.len, A.start, t0, v);
    } else {                           // the chunk crosses into the next channel, or ends the clip
#pragma unroll
      for (unsigned j = 0; j < 4; ++j) {
        const unsigned e = e0 + j;
        if (e < N) {
          const unsigned cj = e / n;
          v[j] = load1(A.row(cj), A.len, A.start, e - cj * n);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += v[j];
  }
  return sum_block(acc, part);
}

// sum over the chM * n elements of the mix in flat order
__device__ __forceinline__ float mix_sum(const Clip& A, const Clip& B, unsigned chM, unsigned n, float mA, float mB, float lam, float mu,
                                         float* part) {
  const unsigned N = chM * n, chunks = (N + 3u) / 4u;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (unsigned k = threadIdx.x; k < chunks; k += MIX_THREADS) {
    const unsigned e0 = 4u * k, c = e0 / n, t0 = e0 - c * n;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (n - t0 >= 4u) {
      float a[4], b[4];
      load4(A.row(c), A.len, A.start, t0, a);
      load4(B.row(c), B.len, B.start, t0, b);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = mix_value(a[j], b[j], mA, mB, lam, mu);
    } else {
#pragma unroll
      for (unsigned j = 0; j < 4; ++j) {
        const unsigned e = e0 + j;
        if (e < N) {
          const unsigned cj = e / n, t = e - cj * n;
          v[j] = mix_value(load1(A.row(cj), A.len, A.start, t), load1(B.row(cj), B.len, B.start, t), mA, mB, lam, mu);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += v[j];
  }
  return sum_block(acc, part);
}

__device__ __forceinline__ bool clip_ok(int off, int ch, int len, int start, unsigned n, long src_floats) {
  return off >= 0 && ch >= 1 && len >= 1 && start >= 0 && start < len && (long)off + (long)ch * len <= src_floats &&
         (long)ch * n <= 0x7fffffffL;
}

// One workgroup = one output row: the means first (the row is re-read through L2 for every later pass: a few hundred KB),
// then channel 0 of the result.  A row whose record does not describe clips inside [0, src_floats) writes nothing.
__global__ void __launch_bounds__(MIX_THREADS) wave_clip_mix_kernel(const float* src, long src_floats, const MixRec* recs, float* out,
                                                                    float* means, unsigned n) {
#pragma clang fp contract(off)
  __shared__ float part[MIX_THREADS / 64];
  const MixRec R = recs[blockIdx.x];
  const bool mixed = R.ch_b != 0;
  if (!clip_ok(R.off_a, R.ch_a, R.len_a, R.start_a, n, src_floats)) return;
  if (mixed && (!clip_ok(R.off_b, R.ch_b, R.len_b, R.start_b, n, src_floats) ||
                !(R.ch_a == R.ch_b || R.ch_a == 1 || R.ch_b == 1)))
    return;
  const Clip A{src + R.off_a, (unsigned)R.ch_a, (unsigned)R.len_a, (unsigned)R.start_a};
  float* y = out + (size_t)blockIdx.x * n;
  const float mA = clip_sum(A, n, part) / (float)(A.ch * n);
  float mB = 0.f, mM = 0.f;
  const unsigned chunks = (n + 3u) / 4u;
  if (!mixed) {
    const float* a0 = A.row(0);
    for (unsigned k = threadIdx.x; k < chunks; k += MIX_THREADS) {
      const unsigned t0 = 4u * k;
      if (n - t0 >= 4u) {
        float a[4];
        load4(a0, A.len, A.start, t0, a);
        const float4 r{a[0] - mA, a[1] - mA, a[2] - mA, a[3] - mA};
        if (((uintptr_t)(y + t0) & 15) == 0) {
          *reinterpret_cast<float4*>(y + t0) = r;
        } else {
          y[t0] = r.x; y[t0 + 1] = r.y; y[t0 + 2] = r.z; y[t0 + 3] = r.w;
        }
      } else {
        for (unsigned t = t0; t < n; ++t) y[t] = load1(a0, A.len, A.start, t) - mA;
      }
    }
  } else {
    const Clip B{src + R.off_b, (unsigned)R.ch_b, (unsigned)R.len_b, (unsigned)R.start_b};
    const unsigned chM = A.ch > B.ch ? A.ch : B.ch;
    mB = clip_sum(B, n, part) / (float)(B.ch * n);
    mM = mix_sum(A, B, chM, n, mA, mB, R.lam, R.mu, part) / (float)(chM * n);
    const float* a0 = A.row(0);
    const float* b0 = B.row(0);
    for (unsigned k = threadIdx.x; k < chunks; k += MIX_THREADS) {
      const unsigned t0 = 4u * k;
      if (n - t0 >= 4u) {
        float a[4], b[4], r[4];
        load4(a0, A.len, A.start, t0, a);
        load4(b0, B.len, B.start, t0, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = mix_value(a[j], b[j], mA, mB, R.lam, R.mu) - mM;
        if (((uintptr_t)(y + t0) & 15) == 0) {
          *reinterpret_cast<float4*>(y + t0) = float4{r[0], r[1], r[2], r[3]};
        } else {
          y[t0] = r[0]; y[t0 + 1] = r[1]; y[t0 + 2] = r[2]; y[t0 + 3] = r[3];
        }
      } else {
        for (unsigned t = t0; t < n; ++t)
          y[t] = mix_value(load1(a0, A.len, A.start, t), load1(b0, B.len, B.start, t), mA, mB, R.lam, R.mu) - mM;
      }
    }
  }
  if (means != nullptr && threadIdx.x == 0) {
    float* m = means + (size_t)blockIdx.x * 3;
    m[0] = mA; m[1] = mB; m[2] = mM;
  }
}

// One thread = four consecutive elements of a row.  VEC: n % 4 == 0 and 16-byte aligned operands.
template <bool VEC>
__global__ void __launch_bounds__(256) mix_rows_kernel(const float* a, const float* b, const int* partner, const float* lam_mu,
                                                       float* out, int rows, long n) {
#pragma clang fp contract(off)
  const int r = blockIdx.x;
  const long i0 = ((long)blockIdx.y * 256 + threadIdx.x) * 4;
  if (i0 >= n) return;
  const int p = partner[r];
  if (p >= rows) return;               // no such row of b: the row is left as it was
  const float* x = a + (size_t)r * n;
  float* y = out + (size_t)r * n;
  if (p < 0) {                         // a copy, bit for bit (also of a NaN's payload: no arithmetic touches it)
    if (x == y) return;
    if (VEC) {
      *reinterpret_cast<float4*>(y + i0) = *reinterpret_cast<const float4*>(x + i0);
    } else {
      for (long i = i0; i < n && i < i0 + 4; ++i) y[i] = x[i];
    }
    return;
  }
  const float* z = b + (size_t)p * n;
  const float lam = lam_mu[2 * r], mu = lam_mu[2 * r + 1];
  if (VEC) {
    const float4 u = *reinterpret_cast<const float4*>(x + i0), w = *reinterpret_cast<const float4*>(z + i0);
    float4 o;
    { const float s = lam * u.x, t = mu * w.x; o.x = s + t; }
    { const float s = lam * u.y, t = mu * w.y; o.y = s + t; }
    { const float s = lam * u.z, t = mu * w.z; o.z = s + t; }
    { const float s = lam * u.w, t = mu * w.w; o.w = s + t; }
    *reinterpret_cast<float4*>(y + i0) = o;
  } else {
    for (long i = i0; i < n && i < i0 + 4; ++i) {
      const float s = lam * x[i], t = mu * z[i];
      y[i] = s + t;
    }
  }
}

}  // namespace

extern "C" int vl_set_error(const char* msg);

extern "C" int vl_wave_clip_mix(const float* src, long src_floats, const void* recs, float* out, float* means, int batch, long n,
                                hipStream_t stream) {
  if (src == nullptr || recs == nullptr || out == nullptr)
    return vl_set_error("vl_wave_clip_mix: src, recs and out must not be null");
  if (batch < 1 || n < 1 || n > 0x7fffffffL || src_floats < 1 || src_floats > 0x7fffffffL)
    return vl_set_error("vl_wave_clip_mix: bad shape (batch >= 1, n and src_floats in [1, 2^31 - 1])");
  if (((uintptr_t)recs & 3) != 0) return vl_set_error("vl_wave_clip_mix: recs must be 4-byte aligned");
  hipLaunchKernelGGL(wave_clip_mix_kernel, dim3((unsigned)batch), dim3(MIX_THREADS), 0, stream, src, src_floats, (const MixRec*)recs, out,
                     means, (unsigned)n);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}

extern "C" int vl_mix_rows(const float* a, const float* b, const int* partner, const float* lam_mu, float* out, int rows, long n,
                           hipStream_t stream) {
  if (a == nullptr || b == nullptr || partner == nullptr || lam_mu == nullptr || out == nullptr)
    return vl_set_error("vl_mix_rows: a, b, partner, lam_mu and out must not be null");
  if (rows < 1 || n < 1) return vl_set_error("vl_mix_rows: bad shape (rows, n >= 1)");
  const long col_blocks = (n + 1023) / 1024;
  if (col_blocks > 65535) return vl_set_error("vl_mix_rows: row too long for one launch (n <= 65535 * 1024)");
  if (b == out) return vl_set_error("vl_mix_rows: out may alias a, not b (a row of b is another row's partner)");
  const dim3 grid((unsigned)rows, (unsigned)col_blocks);
  const bool vec = n % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(mix_rows_kernel<true>, grid, dim3(256), 0, stream, a, b, partner, lam_mu, out, rows, n);
  else
    hipLaunchKernelGGL(mix_rows_kernel<false>, grid, dim3(256), 0, stream, a, b, partner, lam_mu, out, rows, n);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}
