// gemv.hip — sweeps over a tall-skinny basis V (k rows of n floats, k << n): the k dots V r, the combinations V^T y, their fusions
// for the projected solvers (GKS, Hybrid-GMRES, MMGKS) and the damped-LSQR iterate; streaming kernels in the style of vecops.hip.
#include "vec_internal.h"
#include <algorithm>

using namespace trk;

namespace {


// Workgroups of `kernel` (NT threads, no dynamic LDS) that one CU holds at a time.
template <class K>
inline int resident_blocks_per_cu(K kernel) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, NT, 0) != hipSuccess || nb < 1) nb = 4;
  return nb;
}

// Grid of the one-pass k-dot kernels (k_gemv_t / _t2 / _tr): x = shares of the vector, y = row tiles.  All workgroups take the
// same time, so the grid is EXACTLY one resident round — occupancy x CUs workgroups in all, rounded DOWN to whole x-columns.
// Measured (4096^2, k = 18, three tiles): 683 x 3 = 2049 workgroups, one more than the chip holds, ran 290 us; 1024 x 3 (two
// rounds) 222 us; a single full round is what every basis size gets now (tools/gemv_micro.py, profiles/r03/gemv_micro.txt).
inline int tiled_dot_grid_x(int64_t n, int ntile, int blocks_per_cu) {
  const int64_t total = (int64_t)cu_count() * blocks_per_cu;
  int64_t bx = total / ntile;
  // float4s of a row per thread at least: two on short vectors (512^2: one float4 per thread and row left a workgroup little but its
  // reduction to do; Hybrid-GMRES 17.0 -> 17.4 k iterations/s, four: 17.0)
  const int per_thread = n <= ((int64_t)1 << 20) ? 2 : 1;
  const int64_t chunk = (int64_t)NT * 4 * per_thread;
  const int64_t want = (n + chunk - 1) / chunk;
  if (bx > want) bx = want;
  if (bx > kMaxPartialBlocks) bx = kMaxPartialBlocks;
  return bx < 1 ? 1 : (int)bx;
}

// ------------------------------------------------------------------ h[j] = sum_i wt(i) V[j][i] r[i]   (k dots, one pass)
// grid = (bx, ceil(k/JT)); a block sweeps its share of i for JT rows; partials [bx][k].
// WPOW: 0 no weight, 1 multiply by w, 2 multiply by w^2.
constexpr int JT = 8;

template <int WPOW, bool VEC>
__global__ __launch_bounds__(NT) void k_gemv_t(const float* __restrict__ V, int64_t ld, int kv, int64_t n,
                                               const float* __restrict__ r, const float* __restrict__ w,
                                               double* __restrict__ partials, int nt, const float* __restrict__ xrow = nullptr) {
  __shared__ double lds[(NT / 64) * JT];
  // xrow: one more row that is not part of the basis (trk_gemv_t_x: the right-hand side b next to the images A v_j), row index kv
  const int k = kv + (xrow ? 1 : 0);
  // row tiles of equal height: ceil(k / tiles) <= JT rows each (k = 18: 6 + 6 + 6, not 8 + 8 + 2 — the short tile's workgroups
  // read the right-hand sides for a quarter of the work)
  const int jb = (k + (int)gridDim.y - 1) / (int)gridDim.y;
  const int j0 = blockIdx.y * jb;
  const int jn = (k - j0 < jb) ? (k - j0 < 0 ? 0 : k - j0) : jb;
  auto row = [&](int j) -> const float* { return (j0 + j < kv) ? V + (int64_t)(j0 + j) * ld : xrow; };
  double acc[JT];
#pragma unroll
  for (int j = 0; j < JT; ++j) acc[j] = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 rv = ld4(r, i);
      if (WPOW) {
        float4 wv = ld4(w, i);
        if (WPOW == 2) {
          wv.x *= wv.x;
          wv.y *= wv.y;
          wv.z *= wv.z;
          wv.w *= wv.w;
        }
        rv.x *= wv.x;
        rv.y *= wv.y;
        rv.z *= wv.z;
        rv.w *= wv.w;
      }
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        if (j < jn) {
          float4 v = (nt & 64) ? ld4_nt(row(j), i) : ld4(row(j), i);
          acc[j] += (double)v.x * rv.x + (double)v.y * rv.y + (double)v.z * rv.z + (double)v.w * rv.w;
        }
      }
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) {
    float rv = r[i];
    if (WPOW) {
      float wv = w[i];
      rv *= (WPOW == 2) ? wv * wv : wv;
    }
#pragma unroll
    for (int j = 0; j < JT; ++j)
      if (j < jn) acc[j] += (double)row(j)[i] * rv;
  }
  // (one exchange for the JT sums: with a block_sum each, the 2 JT barriers of a workgroup were a visible part of the kernel on
  // short vectors — dynamic problems, n = 2 M)
  const double t = block_sum_many<NT, JT>(acc, lds);
  if ((int)threadIdx.x < jn) partials[(size_t)blockIdx.x * k + j0 + threadIdx.x] = t;
}

// Two right-hand sides in one sweep over the basis: h[j] = V[j] . r and g[j] = V[j] . r2 (partials [bx][2k]).  What the
// Gram-matrix form of the repeated Gram-Schmidt sweeps needs: the coefficients of the new direction AND the Gram row of the
// vector appended last time, for the price of reading the basis once.
template <bool VEC>
__global__ __launch_bounds__(NT) void k_gemv_t2(const float* __restrict__ V, int64_t ld, int k, int64_t n,
                                                const float* __restrict__ r, const float* __restrict__ r2,
                                                double* __restrict__ partials, int nt) {
  __shared__ double lds[(NT / 64) * 2 * JT];
  // row tiles of equal height: ceil(k / tiles) <= JT rows each (k = 18: 6 + 6 + 6, not 8 + 8 + 2 — the short tile's workgroups
  // read the right-hand sides for a quarter of the work)
  const int jb = (k + (int)gridDim.y - 1) / (int)gridDim.y;
  const int j0 = blockIdx.y * jb;
  const int jn = (k - j0 < jb) ? (k - j0 < 0 ? 0 : k - j0) : jb;
  double acc[JT], acc2[JT];
#pragma unroll
  for (int j = 0; j < JT; ++j) acc[j] = acc2[j] = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 rv = ld4(r, i), sv = ld4(r2, i);
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        if (j < jn) {
          float4 v = (nt & 64) ? ld4_nt(V + (int64_t)(j0 + j) * ld, i) : ld4(V + (int64_t)(j0 + j) * ld, i);
          acc[j] += (double)v.x * rv.x + (double)v.y * rv.y + (double)v.z * rv.z + (double)v.w * rv.w;
          acc2[j] += (double)v.x * sv.x + (double)v.y * sv.y + (double)v.z * sv.z + (double)v.w * sv.w;
        }
      }
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) {
    const float rv = r[i], sv = r2[i];
#pragma unroll
    for (int j = 0; j < JT; ++j)
      if (j < jn) {
        const double v = (double)V[(int64_t)(j0 + j) * ld + i];
        acc[j] += v * rv;
        acc2[j] += v * sv;
      }
  }
  double both[2 * JT];
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    both[j] = acc[j];
    both[JT + j] = acc2[j];
  }
  const double t = block_sum_many<NT, 2 * JT>(both, lds);      // value i in thread i
  const int q = threadIdx.x / JT, j = threadIdx.x % JT;
  if (threadIdx.x < 2 * JT && j < jn) partials[(size_t)blockIdx.x * 2 * k + (size_t)q * k + j0 + j] = t;
}

// The same with R right-hand sides (R = 3, 4): out[q k + j] = V[j] . rhs[q].  GKS rides the Gram rows of its NEXT basis vector on
// the sweep that orthogonalises it (krylov.GramSchmidtByGram.sweep, solvers/GKS.py): V^T (A^T A r) and V^T (L^T L r) next to V^T r
// and the newest vector's row of V^T V — one pass over the basis instead of two.
struct RhsSet {
  const float* p[4];
};
template <bool VEC, int R>
__global__ __launch_bounds__(NT) void k_gemv_tr(const float* __restrict__ V, int64_t ld, int k, int64_t n, RhsSet rhs,
                                                double* __restrict__ partials, int nt) {
  __shared__ double lds[(NT / 64) * R * JT];
  // row tiles of equal height: ceil(k / tiles) <= JT rows each (k = 18: 6 + 6 + 6, not 8 + 8 + 2 — the short tile's workgroups
  // read the right-hand sides for a quarter of the work)
  const int jb = (k + (int)gridDim.y - 1) / (int)gridDim.y;
  const int j0 = blockIdx.y * jb;
  const int jn = (k - j0 < jb) ? (k - j0 < 0 ? 0 : k - j0) : jb;
  double acc[R][JT];
#pragma unroll
  for (int q = 0; q < R; ++q)
#pragma unroll
    for (int j = 0; j < JT; ++j) acc[q][j] = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 rv[R];
#pragma unroll
      for (int q = 0; q < R; ++q) rv[q] = ld4(rhs.p[q], i);
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        if (j < jn) {
          const float4 v = (nt & 64) ? ld4_nt(V + (int64_t)(j0 + j) * ld, i) : ld4(V + (int64_t)(j0 + j) * ld, i);
#pragma unroll
          for (int q = 0; q < R; ++q)
            acc[q][j] += (double)v.x * rv[q].x + (double)v.y * rv[q].y + (double)v.z * rv[q].z + (double)v.w * rv[q].w;
        }
      }
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) {
    float rv[R];
#pragma unroll
    for (int q = 0; q < R; ++q) rv[q] = rhs.p[q][i];
#pragma unroll
    for (int j = 0; j < JT; ++j)
      if (j < jn) {
        const double v = (double)V[(int64_t)(j0 + j) * ld + i];
#pragma unroll
        for (int q = 0; q < R; ++q) acc[q][j] += v * rv[q];
      }
  }
  double all[R * JT];
#pragma unroll
  for (int q = 0; q < R; ++q)
#pragma unroll
    for (int j = 0; j < JT; ++j) all[q * JT + j] = acc[q][j];
  const double t = block_sum_many<NT, R * JT>(all, lds);        // value i in thread i
  const int q = threadIdx.x / JT, j = threadIdx.x % JT;
  if (threadIdx.x < R * JT && j < jn) partials[(size_t)blockIdx.x * R * k + (size_t)q * k + j0 + j] = t;
}

// ------------------------------------------------------------------ out = a*base + s * sum_j y[j] V[j]   (+ sum out^2)
constexpr int KMAX_LDS = 1024;  // coefficients staged in LDS as doubles

// HAS_REF: the partials are those of sum (out - ref)^2 instead of sum out^2 (the error norm against x_true)
// where the k coefficients come from: device memory, or the launch's own arguments (values the HOST holds — the projected solution
// of a hybrid solver whose lambda was chosen there — ride in the dispatch packet: no upload, no kernel that computes them)
struct YPtr {
  const double* p;
  __device__ __forceinline__ double at(int j) const { return p[j]; }
};
constexpr int YARG_MAX = 128;
struct YArg {
  double v[YARG_MAX];
  // read where the dispatch put them — the kernel-argument segment, of which this struct is the FIRST member (k_gemv_n) — and not
  // through `v`: indexing a by-value aggregate with the thread index makes every thread copy all of it to scratch first
  __device__ __forceinline__ double at(int j) const {
    return ((const __attribute__((address_space(4))) double*)__builtin_amdgcn_kernarg_segment_ptr())[j];
  }
};

template <bool HAS_BASE, bool SUMSQ, bool VEC, bool HAS_REF = false, class YS = YPtr>
__global__ __launch_bounds__(NT) void k_gemv_n(const YS y, const float* __restrict__ V, int64_t ld, int k, int64_t n,
                                               double a, const float* base, double sc,
                                               float* out, double* __restrict__ partials,
                                               const float* __restrict__ ref = nullptr, int nt = 0) {
  __shared__ double ys[KMAX_LDS];
  __shared__ double lds[NT / 64];
  for (int j = threadIdx.x; j < k; j += NT) ys[j] = sc * y.at(j);
  __syncthreads();
  double acc2 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      double o0 = 0, o1 = 0, o2 = 0, o3 = 0;
      if (HAS_BASE) {
        float4 b = ld4(base, i);
        o0 = a * b.x;
        o1 = a * b.y;
        o2 = a * b.z;
        o3 = a * b.w;
      }
      // rows of the basis are requested in groups — 8, then 4 — before the first of a group is used (the compiler's own unrolling
      // of the plain loop kept 4 in flight; measured, tools/gemv_micro.py: 4 -> 5.4-5.8 TB/s, 8 (+ 8 workgroups per CU) -> 6.2-6.4)
      int j = 0;
      auto group = [&](auto width) {
        constexpr int W = decltype(width)::value;
        float4 v[W];
#pragma unroll
        for (int u = 0; u < W; ++u) v[u] = (nt & 128) ? ld4_nt(V + (int64_t)(j + u) * ld, i) : ld4(V + (int64_t)(j + u) * ld, i);
#pragma unroll
        for (int u = 0; u < W; ++u) {
          const double c = ys[j + u];
          o0 = fma(c, (double)v[u].x, o0);
          o1 = fma(c, (double)v[u].y, o1);
          o2 = fma(c, (double)v[u].z, o2);
          o3 = fma(c, (double)v[u].w, o3);
        }
        j += W;
      };
      while (j + 8 <= k) group(std::integral_constant<int, 8>{});
      if (j + 4 <= k) group(std::integral_constant<int, 4>{});
      while (j < k) group(std::integral_constant<int, 1>{});
      float4 o = make_float4((float)o0, (float)o1, (float)o2, (float)o3);
      st4(out, i, o);
      if (SUMSQ && HAS_REF) {
        const float4 t = ld4(ref, i);
        const double e0 = (double)o.x - t.x, e1 = (double)o.y - t.y, e2 = (double)o.z - t.z, e3 = (double)o.w - t.w;
        acc2 += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
      } else if (SUMSQ) {
        acc2 += (double)o.x * o.x + (double)o.y * o.y + (double)o.z * o.z + (double)o.w * o.w;
      }
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) {
    double o = HAS_BASE ? a * base[i] : 0.0;
    for (int j = 0; j < k; ++j) o = fma(ys[j], (double)V[(int64_t)j * ld + i], o);
    const float of = (float)o;
    out[i] = of;
    if (SUMSQ && HAS_REF) {
      const double e = (double)of - ref[i];
      acc2 += e * e;
    } else if (SUMSQ) {
      acc2 += (double)of * of;
    }
  }
  if (SUMSQ) {
    acc2 = block_sum<NT>(acc2, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc2;
  }
}

// ------------------------------------------------------------------ out = (a*base + s * sum_j y[j] V[j]) [/ sqrt(*den2)] for SHORT vectors
// k_gemv_n gives a thread one 16-byte column of the basis and walks the k rows eight loads at a time: with m-length images of a
// projector (dynamic tomography, C5: m = 122 880 floats against n = 2 M) the grid is 30 workgroups and every thread waits for k / 8
// dependent round trips — 11.5 us for k = 40 rows of half a megabyte each.  Here the four waves of a workgroup share 64 columns and take
// a quarter of the rows each; their partial sums meet in LDS in wave order ((0 + 1) + (2 + 3)).  16-byte aligned operands, n % 4 == 0.
template <bool HAS_BASE>
__global__ __launch_bounds__(NT) void k_gemv_n_split(const double* __restrict__ y, const float* __restrict__ V, int64_t ld, int k,
                                                     int64_t n4, double a, const float* __restrict__ base, double sc, float* out,
                                                     const double* __restrict__ den2) {
  __shared__ double ys[KMAX_LDS];
  __shared__ double part[NT / 64][64][4];
  for (int j = threadIdx.x; j < k; j += NT) ys[j] = sc * y[j];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + lane;
  const int kq = (k + NT / 64 - 1) / (NT / 64);
  const int j0 = wv * kq, j1 = (j0 + kq < k) ? j0 + kq : k;
  double o0 = 0, o1 = 0, o2 = 0, o3 = 0;
  if (i < n4) {
    int j = j0;
    auto group = [&](auto width) {
      constexpr int W = decltype(width)::value;
      float4 v[W];
#pragma unroll
      for (int u = 0; u < W; ++u) v[u] = ld4(V + (int64_t)(j + u) * ld, i);
#pragma unroll
      for (int u = 0; u < W; ++u) {
        const double c = ys[j + u];
        o0 = fma(c, (double)v[u].x, o0);
        o1 = fma(c, (double)v[u].y, o1);
        o2 = fma(c, (double)v[u].z, o2);
        o3 = fma(c, (double)v[u].w, o3);
      }
      j += W;
    };
    while (j + 8 <= j1) group(std::integral_constant<int, 8>{});
    if (j + 4 <= j1) group(std::integral_constant<int, 4>{});
    while (j < j1) group(std::integral_constant<int, 1>{});
  }
  part[wv][lane][0] = o0;
  part[wv][lane][1] = o1;
  part[wv][lane][2] = o2;
  part[wv][lane][3] = o3;
  __syncthreads();
  if (wv != 0 || i >= n4) return;
  double t[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) t[q] = (part[0][lane][q] + part[1][lane][q]) + (part[2][lane][q] + part[3][lane][q]);
  if (HAS_BASE) {
    const float4 b = ld4(base, i);
    t[0] = fma(a, (double)b.x, t[0]);
    t[1] = fma(a, (double)b.y, t[1]);
    t[2] = fma(a, (double)b.z, t[2]);
    t[3] = fma(a, (double)b.w, t[3]);
  }
  if (den2) {
    const double inv = 1.0 / sqrt(*den2);
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] *= inv;
  }
  st4(out, i, make_float4((float)t[0], (float)t[1], (float)t[2], (float)t[3]));
}
// whether the short-vector form serves a call (no fused norm, aligned, few columns, enough rows to be worth splitting)
static bool gemv_n_split_serves(int64_t n, int k, bool vec) {
  return vec && (n % 4) == 0 && n > 0 && (n >> 2) <= (int64_t)64 * 4 * cu_count() && k >= 12 && k <= KMAX_LDS;
}

// ------------------------------------------------------------------ the new basis vector AND the next iterate in ONE pass over the basis
// GKS / MMGKS pass over V three / four times per iteration: x = V y (GKS.py:76), h = V^T r, r - V c (:86-88) [+ the re-weighted Gram].
// The iterate of the NEXT iteration is x' = V y'[0..k) + y'[k] v_k with v_k = (r - V c) / rho the vector this sweep produces — and y'
// needs nothing of v_k but its Gram rows, which follow from the products of the h-sweep (trk_gram_row_from_sweep), and rho, which
// follows from them too (trk_cgs_coeffs_rho: rho^2 = r.r - 2 c.h + c.G c; r is the residual of the projected normal equations, h
// and c are of rounding size, nothing cancels).  So the projected problem of the next iteration is solved BEFORE this pass and the
// pass leaves both vectors: one read of the basis less per iteration.
//   vn = (w - sum_j c[j] V[j]) / sqrt(*rho2)        — the sums of k_gemv_n<HAS_BASE> in its order, ONE rounding to fp32 (after the scaling)
//   x  = sum_{j<k} y[j] V[j] + y[k] vn              — k_gemv_n's sum over the k + 1 stored vectors, term for term (vn as stored)
// HAS_REF: block partials of ||x - ref||^2 (trk_gemv_n_err's); chk != nullptr: block partials of ||w - V c||^2 as computed (float64,
// before the scaling) — what rho^2 stands for, for callers who want to see the two agree.
template <bool VEC, bool HAS_X, bool HAS_REF>
__global__ __launch_bounds__(NT) void k_gemv_orth_iter(const float* __restrict__ V, int64_t ld, int k, int64_t n,
                                                       const float* __restrict__ w, const double* __restrict__ c,
                                                       const double* __restrict__ rho2, const double* __restrict__ y, float* vn, float* x,
                                                       const float* __restrict__ ref, double* __restrict__ partials,
                                                       double* __restrict__ chk, int nt) {
  __shared__ double2 cy[KMAX_LDS];      // (-c[j], y[j])
  __shared__ double lds[NT / 64];
  for (int j = threadIdx.x; j < k; j += NT) cy[j] = make_double2(-c[j], HAS_X ? y[j] : 0.0);
  const double inv = 1.0 / sqrt(*rho2);
  const double yk = HAS_X ? y[k] : 0.0;
  __syncthreads();
  double acc2 = 0.0, accc = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 b = ld4(w, i);
      double o0 = 1.0 * b.x, o1 = 1.0 * b.y, o2 = 1.0 * b.z, o3 = 1.0 * b.w;
      double x0 = 0, x1 = 0, x2 = 0, x3 = 0;
      int j = 0;
      auto group = [&](auto width) {
        constexpr int W = decltype(width)::value;
        float4 v[W];
#pragma unroll
        for (int u = 0; u < W; ++u) v[u] = (nt & 128) ? ld4_nt(V + (int64_t)(j + u) * ld, i) : ld4(V + (int64_t)(j + u) * ld, i);
#pragma unroll
        for (int u = 0; u < W; ++u) {
          const double2 q = cy[j + u];
          o0 = fma(q.x, (double)v[u].x, o0);
          o1 = fma(q.x, (double)v[u].y, o1);
          o2 = fma(q.x, (double)v[u].z, o2);
          o3 = fma(q.x, (double)v[u].w, o3);
          if (HAS_X) {
            x0 = fma(q.y, (double)v[u].x, x0);
            x1 = fma(q.y, (double)v[u].y, x1);
            x2 = fma(q.y, (double)v[u].z, x2);
            x3 = fma(q.y, (double)v[u].w, x3);
          }
        }
        j += W;
      };
      while (j + 8 <= k) group(std::integral_constant<int, 8>{});
      if (j + 4 <= k) group(std::integral_constant<int, 4>{});
      while (j < k) group(std::integral_constant<int, 1>{});
      if (chk) accc += (o0 * o0 + o1 * o1) + (o2 * o2 + o3 * o3);
      const float4 vo = make_float4((float)(o0 * inv), (float)(o1 * inv), (float)(o2 * inv), (float)(o3 * inv));
      st4(vn, i, vo);
      if (HAS_X) {
        const float4 xo = make_float4((float)fma(yk, (double)vo.x, x0), (float)fma(yk, (double)vo.y, x1), (float)fma(yk, (double)vo.z, x2),
                                      (float)fma(yk, (double)vo.w, x3));
        st4(x, i, xo);
        if (HAS_REF) {
          const float4 t = ld4(ref, i);
          const double e0 = (double)xo.x - t.x, e1 = (double)xo.y - t.y, e2 = (double)xo.z - t.z, e3 = (double)xo.w - t.w;
          acc2 += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
        }
      }
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) {
    double o = 1.0 * w[i], xs = 0.0;
    for (int j = 0; j < k; ++j) {
      const double v = (double)V[(int64_t)j * ld + i];
      o = fma(cy[j].x, v, o);
      if (HAS_X) xs = fma(cy[j].y, v, xs);
    }
    if (chk) accc += o * o;
    const float vo = (float)(o * inv);
    vn[i] = vo;
    if (HAS_X) {
      const float xo = (float)fma(yk, (double)vo, xs);
      x[i] = xo;
      if (HAS_REF) {
        const double e = (double)xo - ref[i];
        acc2 += e * e;
      }
    }
  }
  if (HAS_X && HAS_REF) {
    acc2 = block_sum<NT>(acc2, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc2;
  }
  if (chk) {                                                      // uniform over the grid
    __syncthreads();
    accc = block_sum<NT>(accc, lds);
    if (threadIdx.x == 0) chk[blockIdx.x] = accc;
  }
}

// ------------------------------------------------------------------ damped-LSQR iterate by its short recurrence
// x_k = V_k y_k with y_k = argmin || [B_k; damp I] y - beta_1 e_1 ||  (Hybrid_LSQR.py:104-105 with a FIXED lambda, damp =
// sqrt(lambda)) is Paige & Saunders' damped LSQR iterate, which obeys  w_k = v_k - (theta_k / rho_{k-1}) w_{k-1},
// x_k = x_{k-1} + (phi_k / rho_k) w_k  — an algebraic identity in B_k (no orthogonality of V is used), so the k-term
// combination per iterate (4 k n bytes) becomes one pass over three vectors.  The plane rotations (two per step: one against
// the damping, one against beta_{k+1}) are recomputed by thread 0 of every workgroup from alpha_k^2, beta_{k+1}^2 and the
// four doubles the previous step left in st_in = {cs, sn, rho, phibar}; workgroup 0 leaves this step's in st_out (the caller
// alternates two slots).  vk is alpha_k v_k as GKState(normalized=False) stores it.
// Templated on the element type T of the vectors (float: the product; double: the float64 instrument of ref64.hip — the same
// statements with one type changed); VEC (16-byte accesses) exists for float only.
template <class T, bool VEC>
__global__ __launch_bounds__(NT) void k_lsqr_damped_update(const T* __restrict__ vk, T* w, const T* x_in, T* x_out,
                                                           const T* __restrict__ ref, double* __restrict__ err_part, int64_t n,
                                                           const double* __restrict__ a2, const double* __restrict__ b2,
                                                           const double* __restrict__ beta0_sq, double damp,
                                                           const double* __restrict__ st_in, double* __restrict__ st_out, int first) {
  __shared__ double cf[3];
  __shared__ double lds[NT / 64];
  if (threadIdx.x == 0) {
    const double alpha = sqrt(*a2), beta = sqrt(*b2);
    double rhobar, phibar, tw = 0.0;
    if (first) {
      rhobar = alpha;
      phibar = sqrt(*beta0_sq);
    } else {
      rhobar = -st_in[0] * alpha;
      tw = st_in[1] * alpha / st_in[2];
      phibar = st_in[3];
    }
    const double rhobar1 = sqrt(rhobar * rhobar + damp * damp);
    phibar *= rhobar / rhobar1;
    const double rho = sqrt(rhobar1 * rhobar1 + beta * beta);
    const double cs = rhobar1 / rho, sn = beta / rho;
    cf[0] = 1.0 / alpha;
    cf[1] = tw;
    cf[2] = cs * phibar / rho;
    if (blockIdx.x == 0) {
      st_out[0] = cs;
      st_out[1] = sn;
      st_out[2] = rho;
      st_out[3] = sn * phibar;
    }
  }
  __syncthreads();
  const double ia = cf[0], tw = cf[1], px = cf[2];
  double acc = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  auto one = [&](T v, T wo, T xo, T& wn, T& xn) {
    wn = (T)(ia * (double)v - (first ? 0.0 : tw * (double)wo));
    xn = (T)((x_in ? (double)xo : 0.0) + px * (double)wn);
  };
  int64_t tail0 = 0;
  if constexpr (VEC) {
    static_assert(std::is_same<T, float>::value, "16-byte accesses: float only");
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 v = ld4(vk, i);
      const float4 wo = first ? make_float4(0.f, 0.f, 0.f, 0.f) : ld4(w, i);
      const float4 xo = x_in ? ld4(x_in, i) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 wn, xn;
      one(v.x, wo.x, xo.x, wn.x, xn.x);
      one(v.y, wo.y, xo.y, wn.y, xn.y);
      one(v.z, wo.z, xo.z, wn.z, xn.z);
      one(v.w, wo.w, xo.w, wn.w, xn.w);
      st4(w, i, wn);
      st4(x_out, i, xn);
      if (ref) {
        const float4 t = ld4(ref, i);
        const double e0 = (double)xn.x - t.x, e1 = (double)xn.y - t.y, e2 = (double)xn.z - t.z, e3 = (double)xn.w - t.w;
        acc += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
      }
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) {
    T wn, xn;
    one(vk[i], first ? (T)0 : w[i], x_in ? x_in[i] : (T)0, wn, xn);
    w[i] = wn;
    x_out[i] = xn;
    if (ref) {
      const double e = (double)xn - (double)ref[i];
      acc += e * e;
    }
  }
  if (ref) {
    acc = block_sum<NT>(acc, lds);
    if (threadIdx.x == 0) err_part[blockIdx.x] = acc;
  }
}

// ------------------------------------------------------------------ fused reorthogonalisation step
// w_out = w_in - sum_j h[j] V[j]   AND   g[j] = sum_i V[j][i] w_out[i]   with ONE pass over the k basis rows:
// the middle step of repeated classical Gram-Schmidt  r -= V (V^T r)  (GKS.py:86-88 three times, MMGKS.py:119-120 twice,
// Arnoldi): the update with the previous pass's coefficients and the next pass's dot products read the same rows, so a
// thread keeps its k float4 of a column group in registers between the two uses (k <= KB = 8 / 16).
// Element formulas are those of k_gemv_n (fp64 accumulation of the combination, rounded once) and k_gemv_t.
template <int KB, bool VEC>
__global__ __launch_bounds__(NT, 2) void k_gemv_nt(const float* __restrict__ V, int64_t ld, int k, int64_t n,
                                                   const double* __restrict__ h, const float* w_in, float* w_out,
                                                   double* __restrict__ partials) {
  __shared__ double hs[KB];
  __shared__ double lds[NT / 64];
  if (threadIdx.x < KB) hs[threadIdx.x] = threadIdx.x < k ? h[threadIdx.x] : 0.0;
  __syncthreads();
  double acc[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) acc[j] = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 wv = ld4(w_in, i);
      float4 v[KB];
#pragma unroll
      for (int j = 0; j < KB; ++j) v[j] = (j < k) ? ld4(V + (int64_t)j * ld, i) : make_float4(0.f, 0.f, 0.f, 0.f);
      double o0 = (double)wv.x, o1 = (double)wv.y, o2 = (double)wv.z, o3 = (double)wv.w;
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        if (j < k) {
          const double c = -hs[j];
          o0 = fma(c, (double)v[j].x, o0);
          o1 = fma(c, (double)v[j].y, o1);
          o2 = fma(c, (double)v[j].z, o2);
          o3 = fma(c, (double)v[j].w, o3);
        }
      }
      const float4 o = make_float4((float)o0, (float)o1, (float)o2, (float)o3);
      st4(w_out, i, o);
#pragma unroll
      for (int j = 0; j < KB; ++j)
        if (j < k) acc[j] += (double)v[j].x * o.x + (double)v[j].y * o.y + (double)v[j].z * o.z + (double)v[j].w * o.w;
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) {
    float v[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) v[j] = (j < k) ? V[(int64_t)j * ld + i] : 0.f;
    double o0 = (double)w_in[i];
#pragma unroll
    for (int j = 0; j < KB; ++j)
      if (j < k) o0 = fma(-hs[j], (double)v[j], o0);
    const float o = (float)o0;
    w_out[i] = o;
#pragma unroll
    for (int j = 0; j < KB; ++j)
      if (j < k) acc[j] += (double)v[j] * o;
  }
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    if (j < k) {                                                // uniform
      const double t = block_sum<NT>(acc[j], lds);
      if (threadIdx.x == 0) partials[(size_t)blockIdx.x * k + j] = t;
    }
  }
}

}  // namespace

// out = x / sqrt(S), S = the sum of nblk block partials added up by every workgroup as k_finalize would (finalize_block_256: the same
// bits as the finalize launch + trk_axpby(1 / sqrt(*S)) pair it replaces); workgroup 0 leaves S in *sum_out and carries the mailbox
// post, if any (PostReq: its scalars are final here — *sum_out is the last one).
// DOT: the pass also takes <out, dotv> (Hybrid-GMRES with the discrepancy principle wants V_{k+1}^T b, one new entry per step): block
// partials stored write-through, a ticket per workgroup, and the workgroup that draws the LAST one adds them up (k_finalize's order, loads
// past the caches), stores the sum in *dot_out and carries the post instead of workgroup 0 — the dot travels with it (PostReq::sum_host).
template <bool VEC, bool DOT>
__global__ __launch_bounds__(NT) void k_scale_fin(int64_t n, const double* __restrict__ part, int nblk, const float* x, float* out,
                                                  double* sum_out, const PostReq pq, const float* __restrict__ dotv, double* dot_part,
                                                  unsigned* cnt, double* dot_out) {
  __shared__ double lds[NT / 64];
  __shared__ double bc, bd;
  __shared__ unsigned ticket;
  const double S = finalize_block_256(part, nblk, 1, lds);
  if (threadIdx.x == 0) {
    bc = S;
    if (blockIdx.x == 0) *sum_out = S;
  }
  __syncthreads();
  double cv = 1.0;
  cv /= sqrt(bc);                                        // coef_eval(Coef{1.0, nullptr, S, TRK_SQRT_DEN})
  const float a = (float)cv;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  double acc = 0.0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 v = ld4(x, i), o;
      o.x = a * v.x;
      o.y = a * v.y;
      o.z = a * v.z;
      o.w = a * v.w;
      st4(out, i, o);
      if (DOT) {
        const float4 bv = ld4(dotv, i);
        acc += (double)o.x * bv.x + (double)o.y * bv.y + (double)o.z * bv.z + (double)o.w * bv.w;
      }
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) {
    const float o = a * x[i];
    out[i] = o;
    if (DOT) acc += (double)o * dotv[i];
  }
  bool poster = blockIdx.x == 0;
  if (DOT) {
    acc = block_sum<NT>(acc, lds);
    if (threadIdx.x == 0) {
      asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" ::"v"(dot_part + blockIdx.x), "v"(acc) : "memory");
      ticket = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    poster = ticket == gridDim.x - 1;
    if (!poster) return;
    if (threadIdx.x == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // for the next launch
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;        // finalize_block_256's association, the partials loaded past the caches
    auto ldp = [&](int bb) -> double {
      double t;
      asm volatile("global_load_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(t) : "v"(dot_part + bb) : "memory");
      return t;
    };
    int bb = threadIdx.x;
    const int nb = (int)gridDim.x;
    for (; bb + 768 < nb; bb += 1024) {
      v0 += ldp(bb);
      v1 += ldp(bb + 256);
      v2 += ldp(bb + 512);
      v3 += ldp(bb + 768);
    }
    for (; bb < nb; bb += 256) v0 += ldp(bb);
    const double D = block_sum<NT>((v0 + v1) + (v2 + v3), lds);
    if (threadIdx.x == 0) {
      bd = D;
      *dot_out = D;
    }
    __syncthreads();
  }
  if (pq.on && poster && threadIdx.x < 64) {                    // one wave: its lanes move in step, the publication follows the copies
    for (int c = threadIdx.x; c < pq.count; c += 64) {
      const double* sp = pq.src + c;
      pq.dst[c] = (sp == sum_out) ? bc : *sp;
    }
    if (DOT && pq.sum_host && threadIdx.x == 0) *pq.sum_host = bd;       // the dot: its own place on the host (PostReq::sum_host)
    __threadfence_system();
    if (threadIdx.x == 0) __hip_atomic_store(pq.seq, pq.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ======================================================================================= host side that other sources call (namespace trk)
int trk::launch_gemv_t(const float* V, int64_t ld, int k, int64_t n, const float* r, const float* w, int wpow, double* h,
                  hipStream_t s, const float* xrow, double* h_x) {
  const int kt = k + (xrow ? 1 : 0);
  const int ntile = ceil_div(kt, JT);
  static const int occ = resident_blocks_per_cu(k_gemv_t<0, true>);
  const int bx = tiled_dot_grid_x(n, ntile, occ);
  double* part = nullptr;
  if (int rc = scratch_doubles(s, (size_t)bx * kt, &part)) return rc;
  const bool vec = aligned16(V) && aligned16(r) && (ld % 4 == 0) && (!wpow || aligned16(w)) && (!xrow || aligned16(xrow));
  dim3 grid(bx, ntile);
  with_bools([&](auto VEC) {
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(NT), 0, s, V, ld, k, n, r, w, part, stream_nontemporal(n), xrow); };
    if (wpow == 0) launch(k_gemv_t<0, VEC>);
    else if (wpow == 1) launch(k_gemv_t<1, VEC>);
    else launch(k_gemv_t<2, VEC>);
  }, vec);
  TRK_LAUNCH_CHECK();
  if (xrow) return finalize_sums_split(part, bx, kt, kt, h, k, h_x, s);
  return finalize_sums(part, bx, k, k, h, s);
}

int trk::gemv_t2_partials(const float* V, int64_t ld, int k, int64_t n, const float* r, const float* r2, double** part_out, int* nblk,
                          hipStream_t s) {
  TRK_REQUIRE(V && r && r2, "trk_gemv_t2: NULL argument");
  TRK_REQUIRE(k >= 1 && n >= 0 && ld >= n, "trk_gemv_t2: need k >= 1, n >= 0, ld >= n");
  const int ntile = ceil_div(k, JT);
  static const int occ = resident_blocks_per_cu(k_gemv_t2<true>);
  const int bx = tiled_dot_grid_x(n, ntile, occ);
  double* part = nullptr;
  if (int rc = scratch_doubles(s, (size_t)bx * 2 * k, &part)) return rc;
  const bool vec = aligned16(V) && aligned16(r) && aligned16(r2) && (ld % 4 == 0);
  dim3 grid(bx, ntile);
  with_bools([&](auto VEC) { hipLaunchKernelGGL((k_gemv_t2<VEC>), grid, dim3(NT), 0, s, V, ld, k, n, r, r2, part, stream_nontemporal(n)); }, vec);
  TRK_LAUNCH_CHECK();
  *part_out = part;
  *nblk = bx;
  return TRK_OK;
}

int trk::gemv_n_partials(const float* V, int64_t ld, int k, int64_t n, const double* y, double a, const float* base, double sc,
                         float* out, double** part_out, int* nblk, hipStream_t s) {
  TRK_REQUIRE(V && y && out, "trk_gemv_n: NULL argument");
  TRK_REQUIRE(k >= 1 && k <= KMAX_LDS && n >= 0 && ld >= n, "trk_gemv_n: need 1 <= k <= %d, n >= 0, ld >= n", KMAX_LDS);
  const bool sumsq = part_out != nullptr;
  const int grid = stream_grid(n);
  double* part = nullptr;
  const bool vec = aligned16(V) && aligned16(out) && (ld % 4 == 0) && (!base || aligned16(base));
  // short vectors WITH a base (the residual (AV) y - b of a projector's images): rows split over the waves.  The plain combination
  // x = V y stays with k_gemv_n at every size: trk_gemv_n_err and trk_gemv_orth_iterate are its sum term for term (tested bit for bit)
  if (!sumsq && base && gemv_n_split_serves(n, k, vec)) {
    const int64_t n4 = n >> 2;
    const unsigned g = (unsigned)((n4 + 63) / 64);
    hipLaunchKernelGGL((k_gemv_n_split<true>), dim3(g), dim3(NT), 0, s, y, V, ld, k, n4, a, base, sc, out, (const double*)nullptr);
    TRK_LAUNCH_CHECK();
    *nblk = 0;
    return TRK_OK;
  }
  // 8 workgroups per CU (tools/gemv_micro.py); one workgroup for n = 0 (nothing to write, *sumsq = 0)
  const int grid_n = (int)std::max<int64_t>(1, std::min<int64_t>((n + (int64_t)NT * 4 - 1) / ((int64_t)NT * 4), (int64_t)cu_count() * 8));
  if (sumsq)                                                     // one partial per workgroup of the grid actually launched
    if (int rc = scratch_doubles(s, (size_t)(grid_n > grid ? grid_n : grid), &part)) return rc;
  with_bools([&](auto HAS_BASE, auto SUMSQ, auto VEC) {
    hipLaunchKernelGGL((k_gemv_n<HAS_BASE, SUMSQ, VEC>), dim3(grid_n), dim3(NT), 0, s, YPtr{y}, V, ld, k, n, a, base, sc, out, part,
                       (const float*)nullptr, stream_nontemporal(n));
  }, base != nullptr, sumsq, vec);
  TRK_LAUNCH_CHECK();
  if (sumsq) *part_out = part;
  *nblk = grid_n;
  return TRK_OK;
}

int trk::scale_by_partials(int64_t n, const double* part, int nblk, const float* x, float* out, double* sum_out, const PostReq& post,
                           hipStream_t s, const float* dotv, double* dot_out) {
  TRK_REQUIRE(part && nblk >= 1 && x && out && sum_out && n >= 0 && (!dotv || dot_out), "scale_by_partials: bad argument");
  const int grid = stream_grid(n);
  const bool vec = aligned16(x) && aligned16(out) && (!dotv || aligned16(dotv));
  unsigned* cnt = nullptr;
  double* dpart = nullptr;
  if (dotv) {
    if (int rc = stream_ticket(s, &cnt)) return rc;
    // the dot's partials behind the norm's in the stream's scratch (`part` is its start: gemv_n_partials left nblk doubles there)
    double* base = nullptr;
    if (int rc = scratch_doubles(s, (size_t)nblk + (size_t)grid, &base)) return rc;
    TRK_REQUIRE(base == part, "scale_by_partials: the norm's partials are not at the start of the stream's scratch");
    dpart = base + nblk;
  }
  with_bools([&](auto VEC, auto DOT) {                             // without the dot its four arguments are null
    hipLaunchKernelGGL((k_scale_fin<VEC, DOT>), dim3(grid), dim3(NT), 0, s, n, part, nblk, x, out, sum_out, post, dotv, dpart, cnt,
                       DOT ? dot_out : (double*)nullptr);
  }, vec, dotv != nullptr);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

// the damped-LSQR update on float or double vectors (ref64.hip's chain): the scalar-access instantiation of the production template
int trk::lsqr_damped_update_any(size_t elem_bytes, const void* vk, void* w, const void* x_in, void* x_out, int64_t n, const double* alpha_sq,
                           const double* beta_next_sq, const double* beta0_sq, double damp, const double* state_in, double* state_out,
                           int first, hipStream_t s) {
  const int grid = stream_grid(n);
  if (elem_bytes == 8)
    hipLaunchKernelGGL((k_lsqr_damped_update<double, false>), dim3(grid), dim3(NT), 0, s, (const double*)vk, (double*)w, (const double*)x_in,
                       (double*)x_out, (const double*)nullptr, (double*)nullptr, n, alpha_sq, beta_next_sq, beta0_sq, damp, state_in,
                       state_out, first);
  else
    hipLaunchKernelGGL((k_lsqr_damped_update<float, false>), dim3(grid), dim3(NT), 0, s, (const float*)vk, (float*)w, (const float*)x_in,
                       (float*)x_out, (const float*)nullptr, (double*)nullptr, n, alpha_sq, beta_next_sq, beta0_sq, damp, state_in,
                       state_out, first);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

// ======================================================================================= C ABI
extern "C" {

int trk_gemv_t(const float* V, int64_t ld, int k, int64_t n, const float* r, const float* w2, double* h, trk_stream st) {
  TRK_REQUIRE(V && r && h, "trk_gemv_t: NULL argument");
  TRK_REQUIRE(k >= 1 && n >= 0 && ld >= n, "trk_gemv_t: need k >= 1, n >= 0, ld >= n");
  return launch_gemv_t(V, ld, k, n, r, w2, w2 ? 1 : 0, h, (hipStream_t)st);
}

int trk_gemv_nt(const float* V, int64_t ld, int k, int64_t n, const double* h, const float* w_in, float* w_out,
                double* g, trk_stream st) {
  TRK_REQUIRE(V && h && w_in && w_out && g, "trk_gemv_nt: NULL argument");
  TRK_REQUIRE(k >= 1 && k <= 16 && n >= 0 && ld >= n, "trk_gemv_nt: need 1 <= k <= 16, n >= 0, ld >= n");
  hipStream_t s = (hipStream_t)st;
  int bx = stream_grid(n);
  double* part = nullptr;
  if (int rc = scratch_doubles(s, (size_t)bx * k, &part)) return rc;
  const bool vec = aligned16(V) && aligned16(w_in) && aligned16(w_out) && (ld % 4 == 0);
  with_bools([&](auto VEC) {
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(bx), dim3(NT), 0, s, V, ld, k, n, h, w_in, w_out, part); };
    if (k <= 8) launch(k_gemv_nt<8, VEC>);
    else launch(k_gemv_nt<16, VEC>);
  }, vec);
  TRK_LAUNCH_CHECK();
  return finalize_sums(part, bx, k, k, g, s);
}

int trk_gemv_t_x(const float* V, int64_t ld, int k, int64_t n, const float* r, const float* xrow, double* h, double* h_x,
                 trk_stream st) {
  TRK_REQUIRE(V && r && h && xrow && h_x, "trk_gemv_t_x: NULL argument");
  TRK_REQUIRE(k >= 1 && n >= 0 && ld >= n, "trk_gemv_t_x: need k >= 1, n >= 0, ld >= n");
  return launch_gemv_t(V, ld, k, n, r, nullptr, 0, h, (hipStream_t)st, xrow, h_x);
}

int trk_gemv_t2(const float* V, int64_t ld, int k, int64_t n, const float* r, const float* r2, double* h2k, trk_stream st) {
  TRK_REQUIRE(h2k, "trk_gemv_t2: NULL argument");
  double* part = nullptr;
  int bx = 0;
  if (int rc = gemv_t2_partials(V, ld, k, n, r, r2, &part, &bx, (hipStream_t)st)) return rc;
  return finalize_sums(part, bx, 2 * k, 2 * k, h2k, (hipStream_t)st);
}

int trk_gemv_n(const float* V, int64_t ld, int k, int64_t n, const double* y, double a, const float* base, double sc,
               float* out, double* sumsq, trk_stream st) {
  double* part = nullptr;
  int nblk = 0;
  if (int rc = gemv_n_partials(V, ld, k, n, y, a, base, sc, out, sumsq ? &part : nullptr, &nblk, (hipStream_t)st)) return rc;
  if (sumsq) return finalize_sums(part, nblk, 1, 1, sumsq, (hipStream_t)st);
  return TRK_OK;
}

int trk_gemv_n_err(const float* V, int64_t ld, int k, int64_t n, const double* y, float* out, const float* ref,
                   double* err_partials, int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(V && y && out && ref && err_partials && n_blocks, "trk_gemv_n_err: NULL argument");
  TRK_REQUIRE(k >= 1 && k <= KMAX_LDS && n >= 0 && ld >= n, "trk_gemv_n_err: need 1 <= k <= %d, n >= 0, ld >= n", KMAX_LDS);
  // the launch shape of trk_gemv_n (8 workgroups per CU: tools/gemv_micro.py) when the caller's buffer has room for its partials
  int grid = stream_grid(n);
  const int g8 = (int)std::min<int64_t>((n + (int64_t)NT * 4 - 1) / ((int64_t)NT * 4), (int64_t)cu_count() * 8);
  if (g8 >= 1 && g8 <= capacity_blocks) grid = g8;
  TRK_REQUIRE(grid <= capacity_blocks, "trk_gemv_n_err: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  hipStream_t s = (hipStream_t)st;
  const float* nobase = nullptr;
  with_bools([&](auto VEC) {
    hipLaunchKernelGGL((k_gemv_n<false, true, VEC, true>), dim3(grid), dim3(NT), 0, s, YPtr{y}, V, ld, k, n, 1.0, nobase, 1.0, out, err_partials,
                       ref, stream_nontemporal(n));
  }, aligned16(V) && aligned16(out) && aligned16(ref) && (ld % 4 == 0));
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_gemv_orth_iterate(const float* V, int64_t ld, int k, int64_t n, const float* w, const double* c, const double* rho2,
                          const double* y_next, float* vn, float* x_next, const float* ref, double* err_partials, int capacity_blocks,
                          int* n_blocks, double* chk_sumsq, trk_stream st) {
  TRK_REQUIRE(V && w && c && rho2 && vn, "trk_gemv_orth_iterate: NULL argument");
  TRK_REQUIRE((y_next != nullptr) == (x_next != nullptr), "trk_gemv_orth_iterate: y_next and x_next come together");
  TRK_REQUIRE(!ref || (x_next && err_partials && n_blocks), "trk_gemv_orth_iterate: ref needs x_next and room for the partials");
  TRK_REQUIRE(k >= 1 && k < KMAX_LDS && n >= 0 && ld >= n, "trk_gemv_orth_iterate: need 1 <= k < %d, n >= 0, ld >= n", KMAX_LDS);
  TRK_REQUIRE(vn != w && x_next != w && x_next != vn, "trk_gemv_orth_iterate: the outputs must not alias w or each other");
  int grid = stream_grid(n);                                     // trk_gemv_n_err's launch shape
  const int g8 = (int)std::min<int64_t>((n + (int64_t)NT * 4 - 1) / ((int64_t)NT * 4), (int64_t)cu_count() * 8);
  if (g8 >= 1 && (!ref || g8 <= capacity_blocks)) grid = g8;
  if (ref) {
    TRK_REQUIRE(grid <= capacity_blocks, "trk_gemv_orth_iterate: partial buffer too small (%d blocks needed)", grid);
    *n_blocks = grid;
  }
  hipStream_t s = (hipStream_t)st;
  double* chk = nullptr;
  if (chk_sumsq)
    if (int rc = scratch_doubles(s, (size_t)grid, &chk)) return rc;
  const bool vec = aligned16(V) && aligned16(w) && aligned16(vn) && (!x_next || aligned16(x_next)) && (!ref || aligned16(ref)) && (ld % 4 == 0);
  if (!x_next && !chk_sumsq && gemv_n_split_serves(n, k, vec)) {  // the image of the new vector, A v_k = (A r - AV c) / rho: short rows
    const int64_t n4 = n >> 2;
    hipLaunchKernelGGL((k_gemv_n_split<true>), dim3((unsigned)((n4 + 63) / 64)), dim3(NT), 0, s, c, V, ld, k, n4, 1.0, w, -1.0, vn, rho2);
    TRK_LAUNCH_CHECK();
    return TRK_OK;
  }
  const int nt = stream_nontemporal(n);
  with_bools([&](auto VEC) {                                     // HAS_X, HAS_REF: three of the four (no ref without x_next)
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), 0, s, V, ld, k, n, w, c, rho2, y_next, vn, x_next, ref, err_partials, chk, nt);
    };
    if (!x_next) launch(k_gemv_orth_iter<VEC, false, false>);
    else if (ref) launch(k_gemv_orth_iter<VEC, true, true>);
    else launch(k_gemv_orth_iter<VEC, true, false>);
  }, vec);
  TRK_LAUNCH_CHECK();
  if (chk_sumsq) return finalize_sums(chk, grid, 1, 1, chk_sumsq, s);
  return TRK_OK;
}

int trk_gemv_n_hosty(const float* V, int64_t ld, int k, int64_t n, const double* y_host, float* out, const float* ref,
                     double* err_partials, int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(V && y_host && out, "trk_gemv_n_hosty: NULL argument");
  TRK_REQUIRE(!ref || (err_partials && n_blocks), "trk_gemv_n_hosty: ref given but no room for the partials");
  TRK_REQUIRE(k >= 1 && n >= 0 && ld >= n, "trk_gemv_n_hosty: need k >= 1, n >= 0, ld >= n");
  const int grid = stream_grid(n);
  if (ref) {
    TRK_REQUIRE(grid <= capacity_blocks, "trk_gemv_n_hosty: partial buffer too small (%d blocks needed)", grid);
    *n_blocks = grid;
  }
  hipStream_t s = (hipStream_t)st;
  const bool vec = aligned16(V) && aligned16(out) && (!ref || aligned16(ref)) && (ld % 4 == 0);
  // YARG_MAX coefficients per launch; further groups of rows add to what the launches before them left in `out` (rounded to
  // fp32 in between: one rounding more per 128 terms), the last one carries the error norm
  for (int j0 = 0; j0 < k; j0 += YARG_MAX) {
    const int kk = std::min(YARG_MAX, k - j0);
    const bool last = j0 + kk == k, first = j0 == 0;
    YArg ya;
    for (int j = 0; j < kk; ++j) ya.v[j] = y_host[j0 + j];
    for (int j = kk; j < YARG_MAX; ++j) ya.v[j] = 0.0;
    const float* Vj = V + (int64_t)j0 * ld;
    const float* base = first ? nullptr : out;
    double* part = (last && ref) ? err_partials : nullptr;
    with_bools([&](auto HAS_BASE, auto ERR, auto VEC) {          // ERR: the error norm, SUMSQ and HAS_REF together
      hipLaunchKernelGGL((k_gemv_n<HAS_BASE, ERR, VEC, ERR, YArg>), dim3(grid), dim3(NT), 0, s, ya, Vj, ld, kk, n, 1.0, base, 1.0, out, part,
                         ref, 0);
    }, !first, part != nullptr, vec);
  }
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_lsqr_damped_update(const float* vk, float* w, const float* x_in, float* x_out, int64_t n, const float* ref,
                           double* err_partials, int capacity_blocks, int* n_blocks, const double* alpha_sq,
                           const double* beta_next_sq, const double* beta0_sq, double damp, const double* state_in,
                           double* state_out, int first, trk_stream st) {
  TRK_REQUIRE(vk && w && x_out && alpha_sq && beta_next_sq && state_out, "trk_lsqr_damped_update: NULL argument");
  TRK_REQUIRE(first ? beta0_sq != nullptr : (state_in != nullptr && x_in != nullptr),
              "trk_lsqr_damped_update: the first step needs beta0_sq, later ones state_in and x_in");
  TRK_REQUIRE(!ref || (err_partials && n_blocks), "trk_lsqr_damped_update: ref given but no room for the partials");
  TRK_REQUIRE(n >= 0 && damp >= 0.0, "trk_lsqr_damped_update: need n >= 0, damp >= 0");
  const int grid = stream_grid(n);
  if (ref) {
    TRK_REQUIRE(grid <= capacity_blocks, "trk_lsqr_damped_update: partial buffer too small (%d blocks needed)", grid);
    *n_blocks = grid;
  }
  hipStream_t s = (hipStream_t)st;
  const bool vec = aligned16(vk) && aligned16(w) && aligned16(x_out) && (!x_in || aligned16(x_in)) && (!ref || aligned16(ref));
  with_bools([&](auto VEC) {
    hipLaunchKernelGGL((k_lsqr_damped_update<float, VEC>), dim3(grid), dim3(NT), 0, s, vk, w, x_in, x_out, ref, err_partials, n, alpha_sq,
                       beta_next_sq, beta0_sq, damp, state_in, state_out, first);
  }, vec);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_gemv_tn(const float* V, int64_t ld, int k, int64_t n, const float* const* rhs, int n_rhs, double* out, trk_stream st) {
  TRK_REQUIRE(V && rhs && out, "trk_gemv_tn: NULL argument");
  TRK_REQUIRE(n_rhs == 3 || n_rhs == 4, "trk_gemv_tn: 3 or 4 right-hand sides (1: trk_gemv_t, 2: trk_gemv_t2)");
  TRK_REQUIRE(k >= 1 && n >= 0 && ld >= n, "trk_gemv_tn: need k >= 1, n >= 0, ld >= n");
  RhsSet rs{};
  bool vec = aligned16(V) && (ld % 4 == 0);
  for (int q = 0; q < n_rhs; ++q) {
    TRK_REQUIRE(rhs[q], "trk_gemv_tn: NULL right-hand side");
    rs.p[q] = rhs[q];
    vec = vec && aligned16(rhs[q]);
  }
  hipStream_t s = (hipStream_t)st;
  const int ntile = ceil_div(k, JT);
  static const int occ3 = resident_blocks_per_cu(k_gemv_tr<true, 3>), occ4 = resident_blocks_per_cu(k_gemv_tr<true, 4>);
  const int bx = tiled_dot_grid_x(n, ntile, n_rhs == 3 ? occ3 : occ4);
  double* part = nullptr;
  if (int rc = scratch_doubles(s, (size_t)bx * n_rhs * k, &part)) return rc;
  dim3 grid(bx, ntile);
  const int nt = stream_nontemporal(n);
  with_bools([&](auto VEC) {
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(NT), 0, s, V, ld, k, n, rs, part, nt); };
    if (n_rhs == 3) launch(k_gemv_tr<VEC, 3>);
    else launch(k_gemv_tr<VEC, 4>);
  }, vec);
  TRK_LAUNCH_CHECK();
  return finalize_sums(part, bx, n_rhs * k, n_rhs * k, out, s);
}

}  // extern "C"
