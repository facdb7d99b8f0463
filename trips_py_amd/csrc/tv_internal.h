// tv_internal.h — what the two sources with column-thread first-difference kernels share (tvops.hip: the operators and the MM forms;
// pdhg_tv.hip: PDHG's fused forms) and nobody else includes: the block shape, the two grids, the gather of L^T y and the geometry
// of a handle.
#pragma once
#include "trk_internal.h"

namespace {

constexpr int NT = 256;
constexpr int RB = 4;              // image rows per thread and batch
constexpr int kTvMaxBlocks = 4096;  // cap on the blocks (= block partials) per frame of the kernels that reduce

// The 2-D stencils run one thread per image COLUMN over batches of RB rows: every load of a batch is issued before the
// first use (the kernels are latency-, then HBM-bound: memory-level parallelism is what fills the pipe), the vertical
// neighbours of the batch are loaded once, row offsets are running sums (no integer division) and every load/store of a
// wavefront is one contiguous row segment.  grid = (ceil(N/NT), row batches (grid-strided when capped), frames).
struct Grid2 {
  dim3 g;
  int per_frame;  // blocks (= block partials) per frame
};
inline Grid2 grid2(int N, int frames, bool capped) {
  const int gx = (N + NT - 1) / NT;
  int gy = (N + RB - 1) / RB;
  if (capped) {
    const int cap = kTvMaxBlocks / gx;
    if (gy > cap) gy = cap < 1 ? 1 : cap;
  }
  return {dim3(gx, gy, frames), gx * gy};
}

// ONE launch over every frame whose blocks all leave partials: the row batches strided so that the launch has at most
// max(kTvMaxBlocks, column blocks x frames) blocks — a partial buffer costs 64 bytes per block and iteration.
inline dim3 grid3(int N, int frames) {
  const int gx = (N + NT - 1) / NT;
  int gy = (N + RB - 1) / RB;
  const int64_t cap = kTvMaxBlocks / ((int64_t)gx * frames);
  if (gy > cap) gy = cap < 1 ? 1 : (int)cap;
  return dim3(gx, gy, frames);
}

// The gather (L^T y)[i][j] = H[i][j] - H[i][j-1] + V[i][j] - V[i-1][j] (+ T_t[i][j] - T_{t-1}[i][j]) for the rows i0 .. i0 + RB - 1
// of column j of one frame, ONE definition for k_d2_adj and PDHG's fused primal: fused = unfused bit for bit rests on the order of
// the sum.  load: every load of the batch, before the first use.  yh, yv: the frame's H and V rows; tc, tp: T_t and T_{t-1}, NULL
// where the row does not exist.  sum: + hc - hp + v[t+1] - v[t] + a - b, a term outside the index range left out.
template <bool TEMPORAL>
struct AdjGather {
  float hc[RB], hp[RB], v[RB + 1], a[RB], b[RB];
  bool hr, hl, has_c, has_p;

  __device__ __forceinline__ void load(const float* __restrict__ yh, const float* __restrict__ yv, const float* __restrict__ tc,
                                       const float* __restrict__ tp, int N, int i0, int j) {
    const int64_t o0 = (int64_t)i0 * N + j;
    const int64_t h0 = (int64_t)i0 * (N - 1) + j;
    hr = j < N - 1;
    hl = j > 0;
    has_c = TEMPORAL && tc;
    has_p = TEMPORAL && tp;
#pragma unroll
    for (int t = 0; t <= RB; ++t) {      // v[t] = yv[i0 + t - 1][j]
      const int i = i0 + t - 1;
      v[t] = (i >= 0 && i < N - 1) ? yv[o0 + (int64_t)(t - 1) * N] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < RB; ++t) {
      const bool in = i0 + t < N;
      hc[t] = (in && hr) ? yh[h0 + (int64_t)t * (N - 1)] : 0.f;
      hp[t] = (in && hl) ? yh[h0 + (int64_t)t * (N - 1) - 1] : 0.f;
      if (TEMPORAL) {
        a[t] = (in && has_c) ? tc[o0 + (int64_t)t * N] : 0.f;
        b[t] = (in && has_p) ? tp[o0 + (int64_t)t * N] : 0.f;
      }
    }
  }

  // row i = i0 + t < N of the batch
  __device__ __forceinline__ float sum(int t, int i, int N) const {
    float acc = 0.f;
    if (hr) acc += hc[t];
    if (hl) acc -= hp[t];
    if (i < N - 1) acc += v[t + 1];
    if (i > 0) acc -= v[t];
    if (TEMPORAL) {
      if (has_c) acc += a[t];
      if (has_p) acc -= b[t];
    }
    return acc;
  }
};

}  // namespace

namespace trk {
// tvops.hip: N and the frame count of a first-difference handle whose frames all lie on this rank.  Returns the handle's kind — 3: the
// 2-D operator (frames = 1), 4: the space-time operator — and 0 for any other handle (a time-sharded one among them).
int tv_geometry_of(const trk_op* L, int* N, int* frames);
}  // namespace trk
