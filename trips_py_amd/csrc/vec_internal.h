// vec_internal.h — what the four vector-kernel sources share (vecops.hip, cgls_update.hip, gemv.hip, wgram.hip) and nobody else
// includes: other sources define an NT of their own.
#pragma once
#include "trk_internal.h"

namespace {

constexpr int NT = 256;

// grid for a streaming kernel over n floats: one float4 per thread until the chip is covered 4x (<= kMaxPartialBlocks
// blocks so a reduction leaves at most that many partials), then grid-stride
inline int stream_grid(int64_t n) {
  int64_t want = (n + (int64_t)NT * 4 - 1) / ((int64_t)NT * 4);
  int64_t cap = (int64_t)trk::cu_count() * 4;
  if (cap > trk::kMaxPartialBlocks) cap = trk::kMaxPartialBlocks;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  return (int)want;
}

__device__ __forceinline__ float4 ld4(const float* p, int64_t i4) { return reinterpret_cast<const float4*>(p)[i4]; }
__device__ __forceinline__ void st4(float* p, int64_t i4, float4 v) { reinterpret_cast<float4*>(p)[i4] = v; }
// non-temporal accesses for vectors that are not re-read soon (which ones and from which size: stream_nontemporal())
typedef float f4nt __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4_nt(const float* p, int64_t i4) {
  const f4nt v = __builtin_nontemporal_load(reinterpret_cast<const f4nt*>(p) + i4);
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void st4_nt(float* p, int64_t i4, float4 v) {
  __builtin_nontemporal_store((f4nt){v.x, v.y, v.z, v.w}, reinterpret_cast<f4nt*>(p) + i4);
}

}  // namespace

namespace trk {
// gemv.hip: h[j] = sum_i wt(i) V[j][i] r[i] (wpow 0: wt = 1, 1: w, 2: w^2), k_gemv_t and its finalize; xrow: one more row, its dot in *h_x
int launch_gemv_t(const float* V, int64_t ld, int k, int64_t n, const float* r, const float* w, int wpow, double* h, hipStream_t s,
                  const float* xrow = nullptr, double* h_x = nullptr);
}  // namespace trk
