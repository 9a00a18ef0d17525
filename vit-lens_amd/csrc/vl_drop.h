// Perceiver dropout's mask: a pure function of (seed, sample, sub-layer, element) that the forward, the backward and any
// recompute evaluate alike (vl_lens_drop.hip has the definition; tests/perceiver_drop_ref.py is the numpy restatement).
// Shared by the forward / FeedForward kernels of vl_lens_drop.hip and the attention backward of vl_attn_bwd.hip.
#pragma once
#include <math.h>
#include <stdio.h>
#include "vl_philox.h"

extern "C" int vl_set_error(const char* msg);

namespace vldrop {

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

// host: p -> threshold and scale; 0 on success
inline int drop_args(const char* who, double p, uint64_t seed, int64_t sample0, int sublayer, uint64_t groups, uint32_t kg4,
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

}  // namespace vldrop
