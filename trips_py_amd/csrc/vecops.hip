// vecops.hip — the vector algebra inside the Krylov loops, HBM-bound streaming kernels:
// 16-byte-per-lane coalesced loads, grid-stride, fp32 storage, fp64 accumulation, wave64 __shfl reductions,
// one double of block partial per workgroup, summed in a fixed order by core.hip's finalize kernel.
// (The CGLS updates: cgls_update.hip; the sweeps over a tall-skinny basis: gemv.hip; the weighted Gram matrices: wgram.hip.)
#include "vec_internal.h"

using namespace trk;

namespace {

// ------------------------------------------------------------------ dot / nrm2 / diff-nrm2
// MODE 0: sum x*y   1: sum x*x   2: sum (x-y)^2
template <int MODE, bool VEC>
__global__ __launch_bounds__(NT) void k_reduce2(const float* __restrict__ x, const float* __restrict__ y, int64_t n,
                                                double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  double acc = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  if (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 a = ld4(x, i);
      if (MODE == 1) {
        acc += (double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z + (double)a.w * a.w;
      } else {
        float4 b = ld4(y, i);
        if (MODE == 0) {
          acc += (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z + (double)a.w * b.w;
        } else {
          double d0 = (double)a.x - b.x, d1 = (double)a.y - b.y, d2 = (double)a.z - b.z, d3 = (double)a.w - b.w;
          acc += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
        }
      }
    }
    for (int64_t i = (n4 << 2) + tid; i < n; i += nth) {
      double a = x[i], b = (MODE == 1) ? a : (double)y[i];
      acc += (MODE == 2) ? (a - b) * (a - b) : a * b;
    }
  } else {
    for (int64_t i = tid; i < n; i += nth) {
      double a = x[i], b = (MODE == 1) ? a : (double)y[i];
      acc += (MODE == 2) ? (a - b) * (a - b) : a * b;
    }
  }
  acc = block_sum<NT>(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

template <int MODE>
int launch_reduce2(const float* x, const float* y, int64_t n, double* out, hipStream_t s) {
  const int grid = stream_grid(n);
  double* part = nullptr;
  if (int rc = scratch_doubles(s, grid, &part)) return rc;
  const bool vec = aligned16(x) && (MODE == 1 || aligned16(y));
  with_bools([&](auto VEC) { hipLaunchKernelGGL((k_reduce2<MODE, VEC>), dim3(grid), dim3(NT), 0, s, x, y, n, part); }, vec);
  TRK_LAUNCH_CHECK();
  return finalize_sums(part, grid, 1, 1, out, s);
}

// ------------------------------------------------------------------ out = A*x + B*y (+ sum out^2)
template <bool HAS_Y, bool SUMSQ, bool VEC>
__global__ __launch_bounds__(NT) void k_axpby(int64_t n, Coef ca, const float* x, Coef cb, const float* y, float* out,
                                              double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  const float a = (float)coef_eval(ca);
  const float b = HAS_Y ? (float)coef_eval(cb) : 0.f;
  double acc = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 v = ld4(x, i), o;
      if (HAS_Y) {
        float4 w = ld4(y, i);
        o.x = fmaf(a, v.x, b * w.x);
        o.y = fmaf(a, v.y, b * w.y);
        o.z = fmaf(a, v.z, b * w.z);
        o.w = fmaf(a, v.w, b * w.w);
      } else {
        o.x = a * v.x;
        o.y = a * v.y;
        o.z = a * v.z;
        o.w = a * v.w;
      }
      st4(out, i, o);
      if (SUMSQ) acc += (double)o.x * o.x + (double)o.y * o.y + (double)o.z * o.z + (double)o.w * o.w;
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) {
    float o = HAS_Y ? fmaf(a, x[i], b * y[i]) : a * x[i];
    out[i] = o;
    if (SUMSQ) acc += (double)o * o;
  }
  if (SUMSQ) {
    acc = block_sum<NT>(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
  }
}

// ------------------------------------------------------------------ out = a*x with <out, z> (the new basis vector and c_j = v_j . A^T b)
template <bool VEC>
__global__ __launch_bounds__(NT) void k_scale_dot(int64_t n, Coef ca, const float* x, float* out, const float* __restrict__ z,
                                                  double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  const float a = (float)coef_eval(ca);
  double acc = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 v = ld4(x, i), w = ld4(z, i);
      float4 o;
      o.x = a * v.x;
      o.y = a * v.y;
      o.z = a * v.z;
      o.w = a * v.w;
      st4(out, i, o);
      acc += (double)o.x * w.x + (double)o.y * w.y + (double)o.z * w.z + (double)o.w * w.w;
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) {
    const float o = a * x[i];
    out[i] = o;
    acc += (double)o * z[i];
  }
  acc = block_sum<NT>(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// ------------------------------------------------------------------ out = x*y ; MM weights
template <bool VEC>
__global__ __launch_bounds__(NT) void k_mul(int64_t n, const float* x, const float* y, float* out) {
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 a = ld4(x, i), b = ld4(y, i);
      st4(out, i, make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w));
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) out[i] = x[i] * y[i];
}

// out = w * (x - y)
template <bool VEC>
__global__ __launch_bounds__(NT) void k_mul_diff(int64_t n, const float* w, const float* x, const float* y, float* out) {
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 c = ld4(w, i), a = ld4(x, i), b = ld4(y, i);
      st4(out, i, make_float4(c.x * (a.x - b.x), c.y * (a.y - b.y), c.z * (a.z - b.z), c.w * (a.w - b.w)));
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) out[i] = w[i] * (x[i] - y[i]);
}

template <bool HAS_Y, bool VEC>
__global__ __launch_bounds__(NT) void k_mm_weights(int64_t n, const float* x, const float* y, float eps2, float e,
                                                   int special, float* out) {
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 a = ld4(x, i);
      if (HAS_Y) {
        float4 b = ld4(y, i);
        a.x -= b.x;
        a.y -= b.y;
        a.z -= b.z;
        a.w -= b.w;
      }
      st4(out, i, make_float4(mm_w(a.x, eps2, e, special), mm_w(a.y, eps2, e, special), mm_w(a.z, eps2, e, special),
                              mm_w(a.w, eps2, e, special)));
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) {
    float v = HAS_Y ? x[i] - y[i] : x[i];
    out[i] = mm_w(v, eps2, e, special);
  }
}

// ------------------------------------------------------------------ group-sparsity weights (MMGKS.py:86-90)
// out[c*groups + i] = (sum_t d[i*len + t]^2 + add)^expo for c < copies: one weight per group of `len` consecutive
// entries (the nt entries of a row of Ls X), repeated `copies` times (np.kron(ones(nt), wr)).
__global__ __launch_bounds__(NT) void k_group_weights(const float* __restrict__ d, int64_t groups, int len, double add,
                                                      double expo, int copies, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= groups) return;
  const float* g = d + i * len;
  double s = 0.0;
  for (int t = 0; t < len; ++t) s += (double)g[t] * (double)g[t];
  const float w = (float)pow(s + add, expo);
  for (int c = 0; c < copies; ++c) out[(int64_t)c * groups + i] = w;
}

// ------------------------------------------------------------------ isotropic-TV weights (MMGKS.py:61-77, weights.py:29-40)
// The flat iterate is viewed as X[i][j][t] (N x N x nt, t fastest: x.reshape(nx**2, nt) in C order, :71).  With the centered
// 3-point derivative of operators_old.py:22-45 (zero first / last row per axis):
//   g1 = (X[i][j+1][t] - X[i][j-1][t]) / 2  (0 at j = 0, N-1),   g2 = (X[i+1][j][t] - X[i-1][j][t]) / 2  (0 at i = 0, N-1)
//   w  = (g1^2 + g2^2 + eps^2)^e,  written to out[idx] and out[N*N*nt + idx]  (:75-76), idx = (i*N + j)*nt + t;
// behind them the temporal weights  out[2*N*N*nt + k] = (u_tail[k]^2 + eps^2)^e  (:77).  One pass: 4 B read (neighbours hit
// in L1/L2) + 8 B written per element.
__global__ __launch_bounds__(NT) void k_isotv_weights(const float* __restrict__ x, int N, int nt, const float* __restrict__ u_tail,
                                                      int64_t n_tail, float eps2, float e, int special, float* __restrict__ out) {
  const int64_t ns = (int64_t)N * N * nt;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  const int64_t sj = nt, si = (int64_t)N * nt;
  for (int64_t idx = tid; idx < ns; idx += nth) {
    const int64_t r = idx / nt;
    const int i = (int)(r / N), j = (int)(r - (int64_t)i * N);
    const float g1 = (j > 0 && j < N - 1) ? 0.5f * x[idx + sj] - 0.5f * x[idx - sj] : 0.f;
    const float g2 = (i > 0 && i < N - 1) ? 0.5f * x[idx + si] - 0.5f * x[idx - si] : 0.f;
    const float t = fmaf(g1, g1, fmaf(g2, g2, eps2));
    const float w = special == 1 ? 1.0f : special == 2 ? 1.0f / sqrtf(t) : special == 3 ? 1.0f / sqrtf(sqrtf(t)) : powf(t, e);
    out[idx] = w;
    out[ns + idx] = w;
  }
  for (int64_t k = tid; k < n_tail; k += nth) {
    const float t = fmaf(u_tail[k], u_tail[k], eps2);
    out[2 * ns + k] = special == 1 ? 1.0f : special == 2 ? 1.0f / sqrtf(t) : special == 3 ? 1.0f / sqrtf(sqrtf(t)) : powf(t, e);
  }
}

}  // namespace

// ======================================================================================= C ABI
extern "C" {

int trk_dot(const float* x, const float* y, int64_t n, double* out, trk_stream st) {
  TRK_REQUIRE(out && n >= 0 && ((x && y) || n == 0), "trk_dot: NULL argument or n < 0");
  return launch_reduce2<0>(x, y, n, out, (hipStream_t)st);
}

int trk_nrm2sq(const float* x, int64_t n, double* out, trk_stream st) {
  TRK_REQUIRE(out && n >= 0 && (x || n == 0), "trk_nrm2sq: NULL argument or n < 0");
  return launch_reduce2<1>(x, x, n, out, (hipStream_t)st);
}

int trk_diff_nrm2sq(const float* x, const float* y, int64_t n, double* out, trk_stream st) {
  TRK_REQUIRE(out && n >= 0 && ((x && y) || n == 0), "trk_diff_nrm2sq: NULL argument or n < 0");
  return launch_reduce2<2>(x, y, n, out, (hipStream_t)st);
}

int trk_axpby(int64_t n, double ca, const double* a_num, const double* a_den, int a_flags, const float* x, double cb,
              const double* b_num, const double* b_den, int b_flags, const float* y, float* out, double* sumsq,
              trk_stream st) {
  TRK_REQUIRE(x && out && n >= 0, "trk_axpby: NULL x/out or n < 0");
  hipStream_t s = (hipStream_t)st;
  const Coef A{ca, a_num, a_den, a_flags}, B{cb, b_num, b_den, b_flags};
  const int grid = stream_grid(n);
  double* part = nullptr;
  if (sumsq)
    if (int rc = scratch_doubles(s, grid, &part)) return rc;
  const bool vec = aligned16(x) && aligned16(out) && (!y || aligned16(y));
  with_bools([&](auto HAS_Y, auto SUMSQ, auto VEC) {
    hipLaunchKernelGGL((k_axpby<HAS_Y, SUMSQ, VEC>), dim3(grid), dim3(NT), 0, s, n, A, x, B, y, out, part);
  }, y != nullptr, sumsq != nullptr, vec);
  TRK_LAUNCH_CHECK();
  if (sumsq) return finalize_sums(part, grid, 1, 1, sumsq, s);
  return TRK_OK;
}

int trk_scale_dot(int64_t n, double ca, const double* a_num, const double* a_den, int a_flags, const float* x, float* out,
                  const float* z, double* dot_out, trk_stream st) {
  TRK_REQUIRE(x && out && z && dot_out && n >= 0, "trk_scale_dot: NULL argument or n < 0");
  hipStream_t s = (hipStream_t)st;
  const Coef A{ca, a_num, a_den, a_flags};
  const int grid = stream_grid(n);
  double* part = nullptr;
  if (int rc = scratch_doubles(s, grid, &part)) return rc;
  with_bools([&](auto VEC) { hipLaunchKernelGGL((k_scale_dot<VEC>), dim3(grid), dim3(NT), 0, s, n, A, x, out, z, part); },
             aligned16(x) && aligned16(out) && aligned16(z));
  TRK_LAUNCH_CHECK();
  return finalize_sums(part, grid, 1, 1, dot_out, s);
}

int trk_mul(int64_t n, const float* x, const float* y, float* out, trk_stream st) {
  TRK_REQUIRE(x && y && out && n >= 0, "trk_mul: NULL argument or n < 0");
  const int grid = stream_grid(n);
  with_bools([&](auto VEC) { hipLaunchKernelGGL((k_mul<VEC>), dim3(grid), dim3(NT), 0, (hipStream_t)st, n, x, y, out); },
             aligned16(x) && aligned16(y) && aligned16(out));
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_mul_diff(int64_t n, const float* w, const float* x, const float* y, float* out, trk_stream st) {
  TRK_REQUIRE(w && x && y && out && n >= 0, "trk_mul_diff: NULL argument or n < 0");
  const int grid = stream_grid(n);
  with_bools([&](auto VEC) { hipLaunchKernelGGL((k_mul_diff<VEC>), dim3(grid), dim3(NT), 0, (hipStream_t)st, n, w, x, y, out); },
             aligned16(w) && aligned16(x) && aligned16(y) && aligned16(out));
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_mm_weights(int64_t n, const float* x, const float* y, double eps, double p, float* out, trk_stream st) {
  TRK_REQUIRE(x && out && n >= 0, "trk_mm_weights: NULL argument or n < 0");
  const float e = (float)(p / 2.0 - 1.0), eps2 = (float)(eps * eps);
  const int special = (p == 2.0) ? 1 : (p == 1.0) ? 2 : 0;
  const int grid = stream_grid(n);
  const bool vec = aligned16(x) && aligned16(out) && (!y || aligned16(y));
  hipStream_t s = (hipStream_t)st;
  with_bools([&](auto HAS_Y, auto VEC) {
    hipLaunchKernelGGL((k_mm_weights<HAS_Y, VEC>), dim3(grid), dim3(NT), 0, s, n, x, y, eps2, e, special, out);
  }, y != nullptr, vec);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_group_weights(const float* d, int64_t groups, int group_len, double add, double expo, int copies, float* out,
                      trk_stream st) {
  TRK_REQUIRE(d && out && groups >= 0 && group_len >= 1 && copies >= 1, "trk_group_weights: bad argument");
  if (groups == 0) return TRK_OK;
  hipLaunchKernelGGL(k_group_weights, dim3(ceil_div(groups, NT)), dim3(NT), 0, (hipStream_t)st, d, groups, group_len, add, expo,
                     copies, out);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_isotv_weights(const float* x, int N, int nt, const float* u_tail, int64_t n_tail, double eps, double q, float* out,
                      trk_stream st) {
  TRK_REQUIRE(x && out && N >= 1 && nt >= 1 && n_tail >= 0 && (u_tail || n_tail == 0), "trk_isotv_weights: bad argument");
  const double ed = (q - 2.0) / 4.0;                                   // sic: (q-2)/4 (MMGKS.py:75,77)
  const int special = (ed == 0.0) ? 1 : (ed == -0.5) ? 2 : (ed == -0.25) ? 3 : 0;
  const int64_t ns = (int64_t)N * N * nt;
  hipLaunchKernelGGL(k_isotv_weights, dim3(stream_grid(ns > n_tail ? ns : n_tail)), dim3(NT), 0, (hipStream_t)st, x, N, nt,
                     u_tail, n_tail, (float)(eps * eps), (float)ed, special, out);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

}  // extern "C"
