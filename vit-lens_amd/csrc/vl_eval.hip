// Evaluation metrics on the device (training/zero_shot.py's drivers; open_clip/metrics/map.py): integer counts only, and for
// the average precision fp64 ratios of integer counts added in a fixed order - no floating-point atomics, two calls on the same
// input agree bit for bit.
//
//   vl_eval_hits          vl_topk_hits (csrc/vl_linprobe.hip) with three additions: a class map (cond_acc: the classes folded
//                         into "others" count as one), per-class counters (the 3D evaluation's per-class top-1 / top-5 rates) and
//                         the arg-max.  One wave per row, two passes over the row: the best member of the target's group and the
//                         row's arg-max (a (value, index) wave reduction), then the rank of that member (integer wave sum).  The
//                         second pass reads the row from the cache; C is a few thousand at most.
//   vl_clip_mean_normalize  the audio drivers' mean over a sample's clips followed by F.normalize, one wave per sample.
//   vl_average_precision  scikit-learn's average_precision_score(average=None) from its integer form
//                             AP_c = (1 / P) sum_{positive i} #{positive j: s_j >= s_i} / #{j: s_j >= s_i}
//                         A workgroup owns 256 rows x 16 classes: it lists the positives of that tile, and each thread takes one
//                         of them and counts both numbers while the N x 16 strip streams through LDS in tiles of 256 rows (64-byte
//                         row segments: coalesced; the 16 classes share every line that a single column would touch alone).  The
//                         ratios are written back by cell, added per class in a fixed order, and the row tiles' partial sums go
//                         through a workspace to a second launch that adds them in tile order.  Cost O(P N) per class - about
//                         1.2e9 comparisons for AudioSet's evaluation set (20 000 x 527, 0.5 % positives) - and O(N^2) for a
//                         class where half the samples are positive: with every class that dense, 527 x 1e4 x 2e4 = 1e11.
#include "vl_common.h"
#include "vitlens_hip.h"

#include <limits.h>
#include <math.h>

namespace {

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the larger of two (key, index) pairs, the lower index on equal keys; keys are never NaN (eval_key)
struct Best { float key; int idx; };
__device__ __forceinline__ Best best_of(Best a, Best b) {
  return (b.key > a.key || (b.key == a.key && b.idx < a.idx)) ? b : a;
}
__device__ __forceinline__ Best wave_best(Best v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best w;
    w.key = __shfl_xor(v.key, o, 64);
    w.idx = __shfl_xor(v.idx, o, 64);
    v = best_of(v, w);
  }
  return v;
}
// a NaN logit is never "the largest": it orders as -inf when the best member and the arg-max are chosen
__device__ __forceinline__ float eval_key(float x) { return x != x ? -INFINITY : x; }

__global__ void __launch_bounds__(256) eval_hits_kernel(const float* logits, long ld, const int64_t* target, const int* class_map,
                                                        int B, int C, int k0, int k1, int* hits, int* cls_count, int* cls_hit0,
                                                        int* cls_hit1, int* pred) {
  __shared__ int sh[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long b = (long)blockIdx.x * 4 + wave;
  int h0 = 0, h1 = 0;
  if (b < B) {
    const float* row = logits + (size_t)b * ld;
    const int64_t t = target[b];
    const bool bad = t < 0 || t >= C;
    const int tc = bad ? 0 : (int)t;                     // clamped before any read
    const int g = class_map ? class_map[tc] : tc;
    Best m = {-INFINITY, INT_MAX}, top = {-INFINITY, INT_MAX};
    for (int c = lane; c < C; c += 64) {
      const Best x = {eval_key(row[c]), c};
      top = best_of(top, x);
      if ((class_map ? class_map[c] : c) == g) m = best_of(m, x);
    }
    m = wave_best(m);                                    // the group holds tc: never empty
    top = wave_best(top);
    const float v = row[m.idx];
    int rank = 0;
    for (int c = lane; c < C; c += 64) {
      const float x = row[c];
      rank += (x > v) || (x == v && c < m.idx);          // a NaN compares false both ways
    }
    rank = wave_sum_i(rank);
    h0 = !bad && rank < k0;
    h1 = !bad && rank < k1;
    if (lane == 0) {
      if (pred) pred[b] = top.idx;
      if (!bad) {
        if (cls_count) atomicAdd(cls_count + tc, 1);
        if (cls_hit0 && h0) atomicAdd(cls_hit0 + tc, 1);
        if (cls_hit1 && h1) atomicAdd(cls_hit1 + tc, 1);
      }
    }
  }
  if (lane == 0) { sh[wave][0] = h0; sh[wave][1] = h1; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int s = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
    if (s) atomicAdd(hits + threadIdx.x, s);
  }
}

// ---- average precision --------------------------------------------------------------------------------------------------
constexpr int AP_ROWS = 256, AP_COLS = 16, AP_CELLS = AP_ROWS * AP_COLS;          // cell = row * 16 + class: cell & 15 = class

// rows j0 .. j0+255 x classes c0 .. c0+15 into LDS; a cell outside the matrix holds a NaN score (never >= anything) and no flag
__device__ __forceinline__ void ap_load_tile(const float* scores, long ld, const float* targets, long ldt, int N, int C, int j0,
                                             int c0, float* st, uint8_t* tt) {
  for (int e = threadIdx.x; e < AP_CELLS; e += 256) {
    const long j = (long)j0 + (e >> 4);
    const int c = c0 + (e & 15);
    const bool in = j < N && c < C;
    st[e] = in ? scores[(size_t)j * ld + c] : NAN;
    tt[e] = in && targets[(size_t)j * ldt + c] > 0.0f;
  }
}

__global__ void __launch_bounds__(256) ap_partial_kernel(const float* scores, long ld, const float* targets, long ldt, int N, int C,
                                                         double* part, int* pcnt) {
  __shared__ float st[AP_CELLS];
  __shared__ uint8_t tt[AP_CELLS];
  __shared__ uint16_t list[AP_CELLS];                    // the own tile's positive cells, in any order
  __shared__ double ratio[AP_CELLS];                     // per cell: the positive's score until its thread has run, then its ratio
  __shared__ double red[16][AP_COLS];
  __shared__ int redn[16][AP_COLS];
  __shared__ int nlist;
  const int t = threadIdx.x;
  const int i0 = blockIdx.x * AP_ROWS, c0 = blockIdx.y * AP_COLS;
  if (t == 0) nlist = 0;
  ap_load_tile(scores, ld, targets, ldt, N, C, i0, c0, st, tt);
  __syncthreads();
  int mine = 0;                                          // positives among this thread's 16 cells: all of class t & 15
  for (int e = t; e < AP_CELLS; e += 256) {
    const bool pos = tt[e];
    ratio[e] = pos ? (double)st[e] : 0.0;
    if (pos) { list[atomicAdd(&nlist, 1)] = (uint16_t)e; ++mine; }
  }
  __syncthreads();
  const int n = nlist;
  for (int first = 0; first < n; first += 256) {
    const bool act = first + t < n;
    const int cell = act ? list[first + t] : 0;
    const int k = cell & 15;
    const float s = act ? (float)ratio[cell] : NAN;      // (exact: the double holds a float)
    int ge = 0, gep = 0;
    for (int j0 = 0; j0 < N; j0 += AP_ROWS) {
      __syncthreads();                                   // the previous tile has been read
      ap_load_tile(scores, ld, targets, ldt, N, C, j0, c0, st, tt);
      __syncthreads();
      if (act) {
#pragma unroll 8
        for (int r = 0; r < AP_ROWS; ++r) {
          const int above = st[r * AP_COLS + k] >= s;
          ge += above;
          gep += above & (int)tt[r * AP_COLS + k];
        }
      }
    }
    if (act) ratio[cell] = (double)gep / (double)ge;     // ge >= 1: the positive itself (0 / 0 = NaN for a NaN score)
  }
  __syncthreads();
  // per class: this thread's 16 cells in row order, then the 16 row groups in order
  double acc = 0.0;
  for (int e = t; e < AP_CELLS; e += 256) acc += ratio[e];
  red[t >> 4][t & 15] = acc;
  redn[t >> 4][t & 15] = mine;
  __syncthreads();
  if (t < AP_COLS && c0 + t < C) {
    double a = 0.0;
    int p = 0;
    for (int g = 0; g < 16; ++g) { a += red[g][t]; p += redn[g][t]; }
    part[(size_t)blockIdx.x * C + c0 + t] = a;
    pcnt[(size_t)blockIdx.x * C + c0 + t] = p;
  }
}

__global__ void __launch_bounds__(256) ap_final_kernel(const double* part, const int* pcnt, int tiles, int C, double* ap) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double a = 0.0;
  long p = 0;
  for (int r = 0; r < tiles; ++r) { a += part[(size_t)r * C + c]; p += pcnt[(size_t)r * C + c]; }
  ap[c] = p > 0 ? a / (double)p : 0.0;
}

// ---- mean over the clips of a sample, then F.normalize -------------------------------------------------------------------
// one wave per sample: x[(b * n_clip + i), :] added in clip order, divided by n_clip (torch.mean's order), then l2norm_kernel's
// arithmetic (csrc/vl_rows.hip) on the mean, which is kept in the output row between the two passes
__global__ void __launch_bounds__(256) clip_mean_normalize_kernel(const float* x, long ldx, int B, int n_clip, int D, float eps,
                                                                  float* out) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* xr = x + (size_t)b * n_clip * ldx;
  float* yr = out + (size_t)b * D;
  float s = 0.f;
  for (int e = lane; e < D; e += 64) {
    float a = xr[e];
    for (int i = 1; i < n_clip; ++i) a += xr[(size_t)i * ldx + e];
    const float v = a / (float)n_clip;
    yr[e] = v;                                           // read back below by the lane that wrote it
    s = fmaf(v, v, s);
  }
  const float inv = 1.0f / fmaxf(sqrtf(wave_sum(s)), eps);
  for (int e = lane; e < D; e += 64) yr[e] *= inv;
}

}  // namespace

extern "C" int vl_set_error(const char* msg);

static int launched(void) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vl_set_error(hipGetErrorString(e));
}

extern "C" int vl_eval_hits(const float* logits, long ld, const int64_t* target, const int* class_map, int B, int C, int k0, int k1,
                            int* hits, int* cls_count, int* cls_hit0, int* cls_hit1, int* pred, hipStream_t stream) {
  if (B < 1 || C < 1) return vl_set_error("vl_eval_hits: bad shape (B >= 1, C >= 1)");
  if (!logits || !target || !hits) return vl_set_error("vl_eval_hits: logits, target and hits are required");
  if (ld < C) return vl_set_error("vl_eval_hits: ld must be >= C");
  if (k0 < 1 || k1 < 1) return vl_set_error("vl_eval_hits: k counts from 1");
  hipLaunchKernelGGL(eval_hits_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, logits, ld, target, class_map, B, C, k0,
                     k1, hits, cls_count, cls_hit0, cls_hit1, pred);
  return launched();
}

extern "C" long vl_average_precision_ws_bytes(int N, int C) {
  if (N < 1 || C < 1) return 0;
  return (long)((N + AP_ROWS - 1) / AP_ROWS) * C * 12L;          // per row tile and class: one double, one int
}

extern "C" int vl_average_precision(const float* scores, long ld, const float* targets, long ldt, int N, int C, double* ap, void* ws,
                                    hipStream_t stream) {
  if (N < 1 || C < 1) return vl_set_error("vl_average_precision: bad shape (N >= 1, C >= 1)");
  if (!scores || !targets || !ap) return vl_set_error("vl_average_precision: scores, targets and ap are required");
  if (ld < C || ldt < C) return vl_set_error("vl_average_precision: ld and ldt must be >= C");
  if (!ws || ((uintptr_t)ws & 7))
    return vl_set_error("vl_average_precision: a workspace of vl_average_precision_ws_bytes(N, C) bytes, 8-byte aligned, is required");
  const int tiles = (N + AP_ROWS - 1) / AP_ROWS, strips = (C + AP_COLS - 1) / AP_COLS;
  if (strips > 65535) return vl_set_error("vl_average_precision: C beyond 65535 * 16 classes");
  double* part = (double*)ws;
  int* pcnt = (int*)(part + (size_t)tiles * C);
  hipLaunchKernelGGL(ap_partial_kernel, dim3((unsigned)tiles, (unsigned)strips), dim3(256), 0, stream, scores, ld, targets, ldt, N, C,
                     part, pcnt);
  hipLaunchKernelGGL(ap_final_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, part, pcnt, tiles, C, ap);
  return launched();
}

extern "C" int vl_clip_mean_normalize(const float* x, long ldx, int B, int n_clip, int D, float eps, float* out, hipStream_t stream) {
  if (B < 1 || n_clip < 1 || D < 1) return vl_set_error("vl_clip_mean_normalize: bad shape (B >= 1, n_clip >= 1, D >= 1)");
  if (!x || !out) return vl_set_error("vl_clip_mean_normalize: x and out are required");
  if (x == out) return vl_set_error("vl_clip_mean_normalize: out must not be x");
  if (ldx < D) return vl_set_error("vl_clip_mean_normalize: ldx must be >= D");
  hipLaunchKernelGGL(clip_mean_normalize_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, x, ldx, B, n_clip, D, eps, out);
  return launched();
}
