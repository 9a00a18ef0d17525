// The packed text tower's front end: which rows a batch of captions needs, and their embedding.
//
// TriCLIP.encode_text pools ONE row per caption, x[b, argmax(text[b])] (open_clip/model.py:539), out of a causal tower
// (transformer.py:870-876): row t depends on rows <= t only, so the rows behind the pooled one are never read.  The plan
// keeps rows 0 .. argmax(ids[b]) of every caption, one caption behind the other:
//   len[b]      = argmax(ids[b]) + 1 (the first maximum, as torch.argmax)
//   start[b]    = len[0] + ... + len[b-1], start[B] = the number of packed rows
//   last_row[b] = start[b] + len[b] - 1, the pooled row (int64: vl_layernorm_fwd's row_index)
//   total       = {start[B], max_b len[b]}
// All of it is integer arithmetic: the result does not depend on the order of the reductions.
#include "vl_common.h"
#include "vitlens_hip.h"

namespace {

// one wave per caption: lane l scans positions l, l + 64, ...; ties go to the smaller position
__global__ void __launch_bounds__(256) text_len_kernel(const int64_t* ids, int* len, int B, int L) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t* row = ids + (long)b * L;
  long long best = 0; int at = L;                       // (at == L: this lane saw no position)
  for (int t = lane; t < L; t += 64) {
    const long long v = row[t];
    if (at == L || v > best) { best = v; at = t; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long ob = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(at, o, 64);
    if (oa < L && (at == L || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
  }
  if (lane == 0) len[b] = at + 1;
}

// one workgroup: thread i owns the captions [i*per, (i+1)*per), the workgroup scans the per-thread sums through LDS
constexpr int SCAN_T = 1024;
__global__ void __launch_bounds__(SCAN_T) text_scan_kernel(const int* len, int* start, int64_t* last_row, int* total, int B) {
  __shared__ int s_sum[SCAN_T];
  __shared__ int s_max[SCAN_T];
  const int tid = threadIdx.x;
  const int per = (B + SCAN_T - 1) / SCAN_T;
  const int b0 = min(tid * per, B), b1 = min(b0 + per, B);
  int sum = 0, mx = 0;
  for (int b = b0; b < b1; ++b) { const int n = len[b]; sum += n; mx = max(mx, n); }
  s_sum[tid] = sum; s_max[tid] = mx;
  __syncthreads();
  for (int o = 1; o < SCAN_T; o <<= 1) {               // inclusive scan of the sums, running maximum beside it
    const int a = tid >= o ? s_sum[tid - o] : 0, m = tid >= o ? s_max[tid - o] : 0;
    __syncthreads();
    s_sum[tid] += a; s_max[tid] = max(s_max[tid], m);
    __syncthreads();
  }
  int run = s_sum[tid] - sum;                           // exclusive
  for (int b = b0; b < b1; ++b) {
    const int n = len[b];
    start[b] = run; last_row[b] = (int64_t)(run + n - 1);
    run += n;
  }
  if (tid == SCAN_T - 1) { start[B] = s_sum[tid]; total[0] = s_sum[tid]; total[1] = s_max[tid]; }
}

// one wave per (caption, position) of the DENSE grid: positions behind the caption's last row leave at once; the waves
// behind the grid zero the rows [rows, rows_pad) (the GEMMs run whole 256-row tiles: their padded rows start finite)
__global__ void __launch_bounds__(256) text_embed_packed_kernel(const int64_t* ids, const int* start, const int* len,
                                                                const float* emb, const float* pos, float* out, int B, int L,
                                                                int D, int vocab, int rows, int rows_pad) {
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long dense = (long)B * L;
  if (w >= dense) {
    const long r = rows + (w - dense);
    if (r >= rows_pad) return;
    for (int i = lane; i < D; i += 64) out[r * D + i] = 0.f;
    return;
  }
  const int b = (int)(w / L), t = (int)(w - (long)b * L);
  if (t >= len[b]) return;
  const long r = (long)start[b] + t;
  if (r >= rows) return;                                // (a plan that disagrees with the host's totals writes nothing out of range)
  long id = ids[w]; id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float* e = emb + id * D;
  const float* ps = pos + (long)t * D;
  for (int i = lane; i < D; i += 64) out[r * D + i] = e[i] + ps[i];
}

}  // namespace

extern "C" int vl_set_error(const char* msg);
#define VL_HIP_OK(e) do { hipError_t _e = (e); if (_e != hipSuccess) return vl_set_error(hipGetErrorString(_e)); } while (0)

extern "C" int vl_text_pack_plan(const int64_t* ids, int* len, int* start, int64_t* last_row, int* total, int B, int L,
                                 hipStream_t stream) {
  if (B <= 0 || L <= 0) return vl_set_error("vl_text_pack_plan: empty problem");
  if ((long)B * L >= (1L << 31)) return vl_set_error("vl_text_pack_plan: B*L must stay below 2^31");
  if (!ids || !len || !start || !last_row || !total) return vl_set_error("vl_text_pack_plan: null argument");
  hipLaunchKernelGGL(text_len_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, ids, len, B, L);
  hipLaunchKernelGGL(text_scan_kernel, dim3(1), dim3(SCAN_T), 0, stream, (const int*)len, start, last_row, total, B);
  VL_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int vl_text_embed_packed(const int64_t* ids, const int* start, const int* len, const float* tok_emb, const float* pos,
                                    float* out, int B, int L, int D, int vocab, int rows, int rows_pad, hipStream_t stream) {
  if (B <= 0 || L <= 0 || D <= 0) return vl_set_error("vl_text_embed_packed: empty problem");
  if ((long)B * L >= (1L << 31)) return vl_set_error("vl_text_embed_packed: B*L must stay below 2^31");
  if (!ids || !start || !len || !tok_emb || !pos || !out) return vl_set_error("vl_text_embed_packed: null argument");
  if (rows < B || rows > (long)B * L || rows_pad < rows) return vl_set_error("vl_text_embed_packed: need B <= rows <= B*L and rows_pad >= rows");
  const long waves = (long)B * L + (rows_pad - rows);
  hipLaunchKernelGGL(text_embed_packed_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, ids, start, len, tok_emb, pos,
                     out, B, L, D, vocab, rows, rows_pad);
  VL_HIP_OK(hipGetLastError());
  return 0;
}
