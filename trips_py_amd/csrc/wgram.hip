// wgram.hip — weighted Gram matrices of a tall-skinny basis on the matrix cores: G = (w W)(w W)^T over stored rows (trk_wgram), and
// the Gram matrix of L V for the 2-D first-difference L formed from V on the fly (trk_wgram_tv, trk_wgram_tv_z).
#include "vec_internal.h"

using namespace trk;

namespace {

// ------------------------------------------------------------------ weighted Gram, tile pairs (TG x TG)
// G[a][b] = sum_i w_i^2 W[a][i] W[b][i].  grid = (bx, npairs): pair p -> (ta <= tb).  partials [bx][k*k] (upper blocks).
constexpr int TG = 4;

template <bool HAS_W, bool VEC>
__global__ __launch_bounds__(NT) void k_wgram(const float* __restrict__ W, int64_t ld, int k, int64_t m,
                                              const float* __restrict__ w, int ntile,
                                              double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  // blockIdx.y enumerates tile pairs (ta <= tb) row by row
  int ta = 0, rem = blockIdx.y;
  while (rem >= ntile - ta) {
    rem -= ntile - ta;
    ++ta;
  }
  const int a0 = ta * TG, b0 = (ta + rem) * TG;
  double acc[TG][TG];
#pragma unroll
  for (int a = 0; a < TG; ++a)
#pragma unroll
    for (int b = 0; b < TG; ++b) acc[a][b] = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t m4 = m >> 2;
    tail0 = m4 << 2;
    for (int64_t i = tid; i < m4; i += nth) {
      float4 ra[TG], rb[TG];
      float4 ww = make_float4(1.f, 1.f, 1.f, 1.f);
      if (HAS_W) {
        ww = ld4(w, i);
        ww.x *= ww.x;
        ww.y *= ww.y;
        ww.z *= ww.z;
        ww.w *= ww.w;
      }
#pragma unroll
      for (int a = 0; a < TG; ++a) {
        const int ja = (a0 + a < k) ? a0 + a : k - 1;  // clamp: out-of-range rows are computed and discarded
        ra[a] = ld4(W + (int64_t)ja * ld, i);
        if (HAS_W) {
          ra[a].x *= ww.x;
          ra[a].y *= ww.y;
          ra[a].z *= ww.z;
          ra[a].w *= ww.w;
        }
      }
#pragma unroll
      for (int b = 0; b < TG; ++b) {
        const int jb = (b0 + b < k) ? b0 + b : k - 1;
        rb[b] = ld4(W + (int64_t)jb * ld, i);
      }
#pragma unroll
      for (int a = 0; a < TG; ++a)
#pragma unroll
        for (int b = 0; b < TG; ++b)
          acc[a][b] += (double)ra[a].x * rb[b].x + (double)ra[a].y * rb[b].y + (double)ra[a].z * rb[b].z +
                       (double)ra[a].w * rb[b].w;
    }
  }
  for (int64_t i = tail0 + tid; i < m; i += nth) {
    float ww = 1.f;
    if (HAS_W) {
      ww = w[i];
      ww *= ww;
    }
#pragma unroll
    for (int a = 0; a < TG; ++a) {
      const int ja = (a0 + a < k) ? a0 + a : k - 1;
      const float va = W[(int64_t)ja * ld + i] * ww;
#pragma unroll
      for (int b = 0; b < TG; ++b) {
        const int jb = (b0 + b < k) ? b0 + b : k - 1;
        acc[a][b] += (double)va * W[(int64_t)jb * ld + i];
      }
    }
  }
#pragma unroll
  for (int a = 0; a < TG; ++a)
#pragma unroll
    for (int b = 0; b < TG; ++b) {
      double t = block_sum<NT>(acc[a][b], lds);
      if (threadIdx.x == 0 && a0 + a < k && b0 + b < k) {
        partials[(size_t)blockIdx.x * k * k + (size_t)(a0 + a) * k + (b0 + b)] = t;
        partials[(size_t)blockIdx.x * k * k + (size_t)(b0 + b) * k + (a0 + a)] = t;
      }
    }
}


// ------------------------------------------------------------------ weighted Gram on the matrix cores
// The one GEMM-shaped contraction of the path (SYRK: G = R R^T, R = the <= 64 augmented rows, m up to 3e7 long) runs on
// v_mfma_f32_32x32x2_f32: a wave feeds lane l with R[row l&31][element slot l>>5] as BOTH operands (A[i][k] = R_i[e_k],
// B[k][j] = R_j[e_k]), so one instruction adds two elements to a full 32 x 32 tile of G.  Products are exact fp32 FMAs;
// the fp32 tile is flushed into fp64 accumulators after every 32 elements (per wave), so the long sum is fp64.
// Rows are staged per 128-element chunk through LDS with coalesced 16-byte loads (row stride 129 floats: the 32 rows a
// wave reads at one element fall on 32 different banks).  NTILE = 1: KA <= 32 rows (1 tile); NTILE = 2: KA <= 64 (3 tiles).
typedef float f16v __attribute__((ext_vector_type(16)));

template <int NTILE, bool HAS_W, bool HAS_B>
__global__ __launch_bounds__(NT) void k_wgram_mfma(const float* __restrict__ W, int64_t ld, int k, int64_t m,
                                                   const float* __restrict__ w, const float* __restrict__ bvec,
                                                   double* __restrict__ partials) {
  constexpr int KP = 32 * NTILE, CH = 128, RS = CH + 1, CH4 = CH / 4;
  constexpr int NPAIR = NTILE * (NTILE + 1) / 2;
  __shared__ float tile[KP * RS];
  __shared__ double red[3][16][64];
  const int KA = k + (HAS_B ? 2 : 0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  double accd[NPAIR][16];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p)
#pragma unroll
    for (int q = 0; q < 16; ++q) accd[p][q] = 0.0;
  const bool vec_ok = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(W) & 15u) == 0) &&
                      (!HAS_W || (reinterpret_cast<uintptr_t>(w) & 15u) == 0) &&
                      (!HAS_B || (reinterpret_cast<uintptr_t>(bvec) & 15u) == 0);
  const int64_t nchunk = (m + CH - 1) / CH;
  for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
    const int64_t e0 = c * CH;
    const bool full = vec_ok && (e0 + CH <= m);
    if (full) {
      for (int idx = threadIdx.x; idx < KP * CH4; idx += NT) {
        const int row = idx / CH4, q = idx - row * CH4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < KA) {
          float4 wv = make_float4(1.f, 1.f, 1.f, 1.f);
          if (HAS_W && row != k) wv = ld4(w + e0, q);
          if (row < k) v = ld4(W + (int64_t)row * ld + e0, q);
          else v = ld4(bvec + e0, q);
          v.x *= wv.x;
          v.y *= wv.y;
          v.z *= wv.z;
          v.w *= wv.w;
        }
        float* d = &tile[row * RS + 4 * q];
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
      }
    } else {
      for (int idx = threadIdx.x; idx < KP * CH; idx += NT) {
        const int row = idx / CH, e = idx - row * CH;
        float v = 0.f;
        if (row < KA && e0 + e < m) {
          const float wv = (HAS_W && row != k) ? w[e0 + e] : 1.f;
          v = ((row < k) ? W[(int64_t)row * ld + e0 + e] : bvec[e0 + e]) * wv;
        }
        tile[row * RS + e] = v;
      }
    }
    __syncthreads();
    f16v acc[NPAIR];
#pragma unroll
    for (int p = 0; p < NPAIR; ++p)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[p][q] = 0.f;
    const int ebase = wave * 32 + h * 16;       // this wave's 32 elements: slot h takes one half
#pragma unroll 4
    for (int sidx = 0; sidx < 16; ++sidx) {
      const float a0 = tile[r * RS + ebase + sidx];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, a0, acc[0], 0, 0, 0);
      if (NTILE == 2) {
        const float a1 = tile[(32 + r) * RS + ebase + sidx];
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, a1, acc[1], 0, 0, 0);   // rows of tile 0 x rows of tile 1
        acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, a1, acc[2], 0, 0, 0);
      }
    }
#pragma unroll
    for (int p = 0; p < NPAIR; ++p)
#pragma unroll
      for (int q = 0; q < 16; ++q) accd[p][q] += (double)acc[p][q];
    __syncthreads();
  }
  // combine the 4 waves (fixed order) and write the block partial in matrix order
  double* __restrict__ out = partials + (size_t)blockIdx.x * KA * KA;
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) {
    if (wave > 0) {
#pragma unroll
      for (int q = 0; q < 16; ++q) red[wave - 1][q][lane] = accd[p][q];
    }
    __syncthreads();
    if (wave == 0) {
      const int ti = (p == 2) ? 1 : 0, tj = (p == 0) ? 0 : 1;     // pair 0: (0,0)  1: (0,1)  2: (1,1)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const double t = ((accd[p][q] + red[0][q][lane]) + red[1][q][lane]) + red[2][q][lane];
        const int row = ti * 32 + (q & 3) + 8 * (q >> 2) + 4 * h, col = tj * 32 + r;   // MFMA 32x32 C/D map
        if (row < KA && col < KA) {
          out[(size_t)row * KA + col] = t;
          if (ti != tj) out[(size_t)col * KA + row] = t;
        }
      }
    }
    __syncthreads();
  }
}

// Register-direct variant on v_mfma_f32_16x16x4_f32 for KA <= 64 and 16-byte aligned rows: no LDS staging, no block
// barriers inside the stream, and only the T(T+1)/2 upper 16 x 16 tiles of the symmetric Gram are computed (T = ceil(KA/16)).
// Why: the 32 x 32 kernel above is bound by the fp32 matrix pipe, not by HBM — 64 cycles per instruction = 16 B/clk/CU of
// input (measured 0.97 ms per pass over 33.5 M elements whatever k <= 30 is); one 32 x 32 tile costs 128 cycles per 4
// elements, the 16 x 16 tiles cost 32 (T = 1), 96 (T = 2), 192 (T = 3), 320 (T = 4), which puts the pipe at or above
// the HBM rate for every KA <= 64.
// A wave owns groups of 32 U consecutive elements (U = 1).  Lane (r = l & 15, s = l >> 4) loads, for
// each 16-row tile t, 2 U float4 of row 16 t + r at element offsets 16 j + 4 s (j < 2 U): the four s-lanes of a row read 64 contiguous bytes per
// instruction.  Component c of float4 j feeds MFMA number 4 j + c of every tile pair (element slots s = 0..3 then hold
// elements 16 j + 4 s + c).  The next group's loads are issued before the current group's MFMAs; the fp32 tiles are
// flushed into fp64 accumulators after every group, so the long sum is fp64.
typedef float f4v __attribute__((ext_vector_type(4)));

template <int T, bool HAS_W, bool HAS_B>
__global__ __launch_bounds__(NT, 2) void k_wgram_t16(const float* __restrict__ W, int64_t ld, int k, int64_t m,
                                                  const float* __restrict__ w, const float* __restrict__ bvec,
                                                  double* __restrict__ partials) {
  constexpr int NP = T * (T + 1) / 2;
  constexpr int U = 1;                                         // a group is 32 U elements: 2 U float4 per lane and tile (U = 4, 2 measured slower)
  constexpr int GE = 32 * U;
  __shared__ double red[3][4][64];
  const int KA = k + (HAS_B ? 2 : 0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, sl = lane >> 4;
  // every lane loads unconditionally (no divergent branches, so all loads of a group are in flight together): lanes
  // beyond the last row read row 0 and multiply by 0; `one[t]` is the factor of an unweighted live row
  const float* rowp[T];
  bool live[T], wtd[T];
  float one[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int rr = 16 * t + r;
    live[t] = rr < KA;
    wtd[t] = HAS_W && live[t] && rr != k;                      // row k is the plain b; rows < k and row k+1 carry w
    one[t] = live[t] ? 1.f : 0.f;
    rowp[t] = (rr < k) ? W + (int64_t)rr * ld : (HAS_B && live[t] ? bvec : W);
  }
  double accd[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) accd[p][q] = 0.0;
  const int64_t ngroup = m / GE;                               // full groups; the tail (< GE elements) is done below
  const int64_t g0 = (int64_t)blockIdx.x * (NT / 64) + wave, gs = (int64_t)gridDim.x * (NT / 64);
  float4 v[2][T][2 * U];
  auto load = [&](int buf, int64_t g) {
    const int64_t e = g * GE + 4 * sl;
#pragma unroll
    for (int j = 0; j < 2 * U; ++j) {
      float4 wv = make_float4(1.f, 1.f, 1.f, 1.f);
      if (HAS_W) wv = *reinterpret_cast<const float4*>(w + e + 16 * j);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        float4 x = *reinterpret_cast<const float4*>(rowp[t] + e + 16 * j);
        x.x *= wtd[t] ? wv.x : one[t];
        x.y *= wtd[t] ? wv.y : one[t];
        x.z *= wtd[t] ? wv.z : one[t];
        x.w *= wtd[t] ? wv.w : one[t];
        v[buf][t][j] = x;
      }
    }
  };
  auto consume = [&](int buf) {
    int p = 0;
#pragma unroll
    for (int ta = 0; ta < T; ++ta)
#pragma unroll
      for (int tb = ta; tb < T; ++tb, ++p) {
        f4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 2 * U; ++j) {
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v[buf][ta][j].x, v[buf][tb][j].x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v[buf][ta][j].y, v[buf][tb][j].y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v[buf][ta][j].z, v[buf][tb][j].z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v[buf][ta][j].w, v[buf][tb][j].w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) accd[p][q] += (double)acc[q];
      }
  };
  if (g0 < ngroup) {
    load(0, g0);
    int64_t g = g0;
    for (; g + 2 * gs < ngroup; g += 2 * gs) {                 // two groups per trip: buffer indices stay compile-time
      load(1, g + gs);
      consume(0);
      load(0, g + 2 * gs);
      consume(1);
    }
    if (g + gs < ngroup) {
      load(1, g + gs);
      consume(0);
      consume(1);
    } else {
      consume(0);
    }
  }
  // tail elements [GE * ngroup, m): one wave, scalar predicated loads; element slot sl of step i holds element 4 i + sl
  if (blockIdx.x == 0 && wave == 0 && (m % GE)) {
    const int64_t e0 = ngroup * GE;
    for (int i = 0; i < 8 * U; ++i) {
      const int64_t e = e0 + 4 * i + sl;
      float a[T];
#pragma unroll
      for (int t = 0; t < T; ++t) a[t] = (live[t] && e < m) ? rowp[t][e] * (wtd[t] ? w[e] : 1.f) : 0.f;
      int p = 0;
#pragma unroll
      for (int ta = 0; ta < T; ++ta)
#pragma unroll
        for (int tb = ta; tb < T; ++tb, ++p) {
          f4v acc = {0.f, 0.f, 0.f, 0.f};
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ta], a[tb], acc, 0, 0, 0);
#pragma unroll
          for (int q = 0; q < 4; ++q) accd[p][q] += (double)acc[q];
        }
    }
  }
  // combine the 4 waves (fixed order) and write the block partial in matrix order (16x16 C/D map: lane (r, sl), register q
  // holds D[4 sl + q][r])
  double* __restrict__ out = partials + (size_t)blockIdx.x * KA * KA;
  int p = 0;
#pragma unroll
  for (int ta = 0; ta < T; ++ta)
#pragma unroll
    for (int tb = ta; tb < T; ++tb, ++p) {
      if (wave > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave - 1][q][lane] = accd[p][q];
      }
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double t = ((accd[p][q] + red[0][q][lane]) + red[1][q][lane]) + red[2][q][lane];
          const int row = 16 * ta + 4 * sl + q, col = 16 * tb + r;
          if (row < KA && col < KA) {
            out[(size_t)row * KA + col] = t;
            if (ta != tb) out[(size_t)col * KA + row] = t;
          }
        }
      }
      __syncthreads();
    }
}

// ------------------------------------------------------------------ weighted Gram of L V for the 2-D first-difference L, from V
// G[a][b] = sum over the rows e of L of  w_e^2 (L v_a)_e (L v_b)_e,   L = [D_h; D_v]  (MMGKS.py:94-95: the R factor of wr * (L V)
// enters the projected problem only through this Gram matrix).  k_wgram_t16 reads the stored images L v_j — 2 n floats
// per basis vector; here a wave forms them on the fly from V (n floats per vector: HALF the bytes, and L V is never written or
// kept).  A wave owns a strip of 32 image columns and marches down a band of rows: lane (r = l & 15, sl = l >> 4) holds, per
// 16-row tile t of V, the 8 pixels at columns 32 strip + 8 sl .. + 7 of row 16 t + r of V, for the current and the next image row
// — every element of V is loaded ONCE (the row below is the next step's current row).  The pixel right of a lane's eight comes
// from lane l + 16 (ds_bpermute; the last quarter takes the next strip's first pixel, one dword load per tile and step); the 64
// weights of a step (32 horizontal, 32 vertical) are ONE coalesced dword load per wave, spread to the lanes through LDS.  (First
// version: per-lane loads of the weights and of the right neighbours — as many L2 requests again as the rows themselves; 2 TB/s.)
// Per step 64 weighted differences go through the same v_mfma_f32_16x16x4_f32 tile pairs as in k_wgram_t16, flushed into fp64
// every step.  Rows are loaded two steps ahead.  w = [w_h: N rows of N-1 | w_v: N-1 rows of N] (trk_tv_weights).  N % 32 == 0.
template <int T>
struct TvRow {
  float4 x[T][2];      // 8 consecutive pixels of the image row, per tile
  float nx[T];         // the first pixel of the next strip (used by the lanes sl == 3 only)
  float w;             // lane l < 32: w_h of column 32 strip + l ; l >= 32: w_v of column 32 strip + l - 32
  float z;             // (Z) lane l: z of column 32 strip + (l & 31)
};

// Z: the pass also takes h[j] = V[j] . z for one more image z (MMGKS: the Gram row V^T (A^T A v_new) of the vector appended last,
// which needs the same sweep over V — trk_wgram_tv_z): fp64 products as in k_gemv_t, z spread to the lanes like the weights.
// Block partials: [k*k Gram | k dots] per workgroup.
// D: image rows held per wave (the current one, the next, D - 2 in flight).  D = 3 is what is instantiated: with one workgroup per
// CU and D = 6 (four rows in flight, 320-380 VGPRs) k = 32 went from 689 to 716 us — latency is not what that case waits for; for
// k <= 24 the kernel sits at the fp32 matrix pipe's rate already (48 MFMAs per 32 pixels at two tiles).
// BF (round 4): the products of the Gram tiles through the bf16 matrix pipe, each operand split into two bf16 halves and ALL FOUR
// partial products taken — (a_hi + a_lo)(b_hi + b_lo) exactly; what is lost is each operand's third piece, 2^-17 of it, of either
// sign (dropping a_lo b_lo instead would bias every diagonal entry low by ~1e-6: the squares of the roundings do not cancel).
// v_mfma_f32_16x16x32_bf16 takes a lane's eight weighted differences of a step in ONE instruction: 4 x 16 cycles per tile pair and
// direction where eight v_mfma_f32_16x16x4_f32 took 256 — the fp32 matrix pipe, at the vector unit's own rate, was this kernel's
// bound at two tiles (k = 17 .. 32: 0.51-0.57 ms whatever k; 48 MFMAs x 32 cycles per 32 pixels), now the rows' traffic is.
// The verdict of trk_wgram_tv's 'auto' arithmetic (the probe is further down: k_wgram_tv_probe): sums = the probe's 2 x 10 finished
// sums {S_ab, S'_ab}; worst = max_ab |S' - S| / sqrt(S_aa S_bb); verdict = worst > threshold.  Every workgroup of the Gram launch
// evaluates it (20 scalar loads, the same bits everywhere); the first one also records it in `record`.
struct ProbeGate {
  const double* sums;     // NULL: no probe ('auto' not chosen)
  double threshold;
  double* record;         // {verdict, worst} for trk_wgram_tv_last_probe
  int groups = 1;         // sets of four sampled basis vectors: 2 x 10 sums each (k_wgram_tv_probe)
};
__device__ __forceinline__ int probe_verdict(const ProbeGate& pg, bool record) {
  constexpr int PV = 4, PP = 10;
  double worst = 0.0;
  for (int g = 0; g < pg.groups; ++g) {
    const double* __restrict__ S = pg.sums + g * 2 * PP;
    int q = 0;
#pragma unroll
    for (int a = 0; a < PV; ++a)
#pragma unroll
      for (int b = a; b < PV; ++b, ++q) {
        // (the diagonal entries of the upper-triangle order: a = 0 -> 0, 1 -> 4, 2 -> 7, 3 -> 9)
        const int qa = a == 0 ? 0 : a == 1 ? 4 : a == 2 ? 7 : 9, qb = b == 0 ? 0 : b == 1 ? 4 : b == 2 ? 7 : 9;
        const double sc = sqrt(fabs(S[qa] * S[qb]));
        if (sc > 0.0) worst = fmax(worst, fabs(S[PP + q] - S[q]) / sc);
      }
  }
  const int verdict = worst > pg.threshold ? 1 : 0;
  if (record && pg.record) {
    pg.record[0] = (double)verdict;
    pg.record[1] = worst;
  }
  return verdict;
}
typedef __bf16 bf8v __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void bf16_split8(const float (&d)[8], bf8v& hi, bf8v& lo) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    hi[c] = (__bf16)d[c];
    lo[c] = (__bf16)(d[c] - (float)hi[c]);
  }
}
// BF = 3 (round 5): THREE bf16 pieces per operand — hi + mid + lo is the fp32 value exactly — and the six partial products down to
// 2^-16 of the largest (hi hi, hi mid, mid hi, mid mid, hi lo, lo hi; what is dropped is 2^-24 and below, the fp32 accumulator's own
// resolution).  Two pieces lose up to 2^-16 of EACH operand; on noisy data the residuals average out (measured 5e-9 against the
// fp32-pipe Gram), on piecewise-constant or repeated values they are all the same number and do not: a Gram entry was then off by
// up to 3e-5 of itself (tests/test_gpu_kernels.py::test_wgram_tv_split_products_on_adversarial_images).
__device__ __forceinline__ void bf16_split8x3(const float (&d)[8], bf8v& hi, bf8v& mid, bf8v& lo) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    hi[c] = (__bf16)d[c];
    const float r1 = d[c] - (float)hi[c];
    mid[c] = (__bf16)r1;
    lo[c] = (__bf16)(r1 - (float)mid[c]);
  }
}
// The arithmetic of one image row of a 32-column strip (k_wgram_tv and k_wgram_tv_lds): lane (r, sl) holds, per 16-vector tile t, the eight
// pixels Px[t] of image row i and Qx[t] of the row below, nbr[t] = the pixel right of the strip (used by the last quarter only), and the
// row's weights for its eight columns; the weighted differences' tile products in the arithmetic AR (0 fp32 pipe, 2 / 3 bf16 pieces),
// flushed into the float64 accumulators.
template <int T, int AR>
__device__ __forceinline__ void tv_row_products(const float4 (&Px)[T][2], const float4 (&Qx)[T][2], const float (&nbr)[T], int up16, int sl,
                                                const float4& wh0, const float4& wh1, const float4& wv0, const float4& wv1,
                                                double (&accd)[T * (T + 1) / 2][4]) {
  constexpr int NP = T * (T + 1) / 2;
    f4v acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = (f4v){0.f, 0.f, 0.f, 0.f};
    float dh[T][8], dv[T][8];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const float4 a = Px[t][0], b = Px[t][1], c = Qx[t][0], d = Qx[t][1];
      // the pixel right of this lane's eight: lane l + 16 holds it as its first, the last quarter takes the next strip's
      float right = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(up16, __builtin_bit_cast(int, a.x)));
      right = sl == 3 ? nbr[t] : right;
      dh[t][0] = (a.x - a.y) * wh0.x;
      dh[t][1] = (a.y - a.z) * wh0.y;
      dh[t][2] = (a.z - a.w) * wh0.z;
      dh[t][3] = (a.w - b.x) * wh0.w;
      dh[t][4] = (b.x - b.y) * wh1.x;
      dh[t][5] = (b.y - b.z) * wh1.y;
      dh[t][6] = (b.z - b.w) * wh1.z;
      dh[t][7] = (b.w - right) * wh1.w;
      dv[t][0] = (a.x - c.x) * wv0.x;
      dv[t][1] = (a.y - c.y) * wv0.y;
      dv[t][2] = (a.z - c.z) * wv0.z;
      dv[t][3] = (a.w - c.w) * wv0.w;
      dv[t][4] = (b.x - d.x) * wv1.x;
      dv[t][5] = (b.y - d.y) * wv1.y;
      dv[t][6] = (b.z - d.z) * wv1.z;
      dv[t][7] = (b.w - d.w) * wv1.w;
    }
    if constexpr (AR == 3) {
      // one direction at a time (its three pieces die before the other direction's are made: the register file is the limit here)
      auto dir = [&](const float (&dd)[T][8]) {
        bf8v ph[T], pm[T], pl[T];
#pragma unroll
        for (int t = 0; t < T; ++t) bf16_split8x3(dd[t], ph[t], pm[t], pl[t]);
        int pp = 0;
#pragma unroll
        for (int ta = 0; ta < T; ++ta)
#pragma unroll
          for (int tb = ta; tb < T; ++tb, ++pp) {
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph[ta], pl[tb], acc[pp], 0, 0, 0);      // smallest terms first
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pl[ta], ph[tb], acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pm[ta], pm[tb], acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph[ta], pm[tb], acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pm[ta], ph[tb], acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph[ta], ph[tb], acc[pp], 0, 0, 0);
          }
      };
      dir(dh);
      dir(dv);
    } else {
      auto two_pieces = [&]() {
        bf8v hh[T], hl[T], vh[T], vl[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
          bf16_split8(dh[t], hh[t], hl[t]);
          bf16_split8(dv[t], vh[t], vl[t]);
        }
        int pp = 0;
#pragma unroll
        for (int ta = 0; ta < T; ++ta)
#pragma unroll
          for (int tb = ta; tb < T; ++tb, ++pp) {
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hl[ta], hl[tb], acc[pp], 0, 0, 0);      // smallest terms first
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vl[ta], vl[tb], acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hh[ta], hl[tb], acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hl[ta], hh[tb], acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh[ta], vl[tb], acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vl[ta], vh[tb], acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hh[ta], hh[tb], acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh[ta], vh[tb], acc[pp], 0, 0, 0);
          }
      };
      auto fp32_pipe = [&]() {
        int pp = 0;
#pragma unroll
        for (int ta = 0; ta < T; ++ta)
#pragma unroll
          for (int tb = ta; tb < T; ++tb, ++pp) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
              acc[pp] = __builtin_amdgcn_mfma_f32_16x16x4f32(dh[ta][c], dh[tb][c], acc[pp], 0, 0, 0);
              acc[pp] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[ta][c], dv[tb][c], acc[pp], 0, 0, 0);
            }
          }
      };
      if constexpr (AR == 2) two_pieces();
      else fp32_pipe();
    }
#pragma unroll
    for (int p2 = 0; p2 < NP; ++p2)
#pragma unroll
      for (int q = 0; q < 4; ++q) accd[p2][q] += (double)acc[p2][q];
}

// MINB: two tiles, three pieces: 256 registers (no spills) at 2 workgroups per CU is the faster form (532 / 605 us at k = 17 / 32
// against 648 / 781 with 32 spilled registers at 3: profiles/r05/wgram_tv_pieces.txt)
template <int T, bool Z, int D, int BF = 3, int MINB = (D > 3 ? 1 : T == 1 ? 4 : (T == 2 && !Z && BF != 3) ? 3 : 2)>
__global__ __launch_bounds__(NT, MINB) void k_wgram_tv(const float* __restrict__ V, int64_t ld, int k, int N,
                                                    const float* __restrict__ w, int nbands, int band_rows,
                                                    double* __restrict__ partials, const float* __restrict__ z, int lockstep,
                                                    ProbeGate pg) {
  // 'auto' arithmetic (trk_wgram_tv_precision), BF == 4: ONE launch holds both arithmetics — two bf16 pieces / the fp32 pipe — and
  // the probe's verdict (worked out by every workgroup from the probe's 20 finished sums: no launch for it) picks per launch
  // (uniform branch in the step)
  bool use_f32 = false;
  if constexpr (BF == 4) use_f32 = pg.sums && probe_verdict(pg, blockIdx.x == 0 && threadIdx.x == 0) != 0;
  constexpr int NP = T * (T + 1) / 2;
  __shared__ double red[3][4][64];
  __shared__ __attribute__((aligned(16))) float wl[NT / 64][Z ? 96 : 64];
  // lockstep (the launcher's choice when the workgroup's four waves always own four neighbouring strips of one band): the pixel
  // right of a strip is the first pixel of the next wave's strip, which that wave holds in registers — it is handed over through
  // LDS, one row ahead, behind the one barrier per image row that keeps the four waves together.  Only the workgroup's last wave
  // still fetches its neighbour column from memory.  (Every wave fetching it cost 25-40 % more HBM traffic than the operands: the
  // column is a sector of a line that the neighbouring strip's wave fetches again at some other time;
  // profiles/r03/traffic_bench_c4.txt.)
  __shared__ float nxs[2][NT / 64][T][16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, sl = lane >> 4;
  const float* __restrict__ wh = w;
  const float* __restrict__ wv = w + (int64_t)N * (N - 1);
  const float* rowp[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int rr = 16 * t + r;
    rowp[t] = V + (int64_t)(rr < k ? rr : 0) * ld;              // rows beyond the basis read row 0: their Gram entries are never stored
  }
  double accd[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) accd[p][q] = 0.0;
  double accz[T];                                                // (the dots V[j] . z stay float64 FMAs: through the matrix pipe as
#pragma unroll                                                   //  well — split operands, four products — they cost what they cost here)
  for (int t = 0; t < T; ++t) accz[t] = 0.0;
  const int strips = N / 32;
  const int64_t units = (int64_t)strips * nbands;
  const int64_t gw = (int64_t)blockIdx.x * (NT / 64) + wave, nw = (int64_t)gridDim.x * (NT / 64);
  float* __restrict__ my = wl[wave];
  const int up16 = ((lane + 16) & 63) << 2;                      // ds_bpermute address of lane l + 16

  // Which XCD's L2 meets which strips (round 4).  The pixel right of a workgroup's four strips is one dword of a line that the
  // workgroup owning the next four strips fetches as its own data: with workgroups dealt round-robin to the eight XCDs the two
  // sit behind different L2s and the line crosses the fabric twice — 1.33 x the operand bytes at 4096^2 (FETCH_SIZE,
  // profiles/r04/traffic_c4_before_xcd_map.txt).  Workgroups b and b + 8 share an XCD (placement is speed only, never correctness),
  // so each XCD is given a CONTIGUOUS eighth of every band's strip groups: the neighbour line is then in its own L2 except at the
  // eight seams.  Needs the groups of a band to divide by 8 (N a multiple of 1024) and a grid that is a multiple of 8.
  const int groups = strips / (NT / 64);
  const bool xcd_map = strips % (NT / 64) == 0 && (groups & 7) == 0 && (gridDim.x & 7) == 0;   // (uniform)
  // The whole sweep once per arithmetic AR (0 fp32 pipe, 2 / 3 bf16 pieces).  BF == 4 ('auto') instantiates it twice under ONE uniform
  // branch on the probe's verdict: both forms in one launch, each with its own register allocation (a branch inside the step made
  // the allocator keep both forms' operands live: 34-99 spilled registers).
  auto run = [&](auto arith_tag) {
  constexpr int AR = decltype(arith_tag)::value;
  for (int64_t it = 0;; ++it) {
    int64_t u;
    if (xcd_map) {
      const int64_t U = (int64_t)blockIdx.x + it * gridDim.x;
      if (U >= units / (NT / 64)) break;
      const int per = groups >> 3;
      const int64_t q = U >> 3;
      const int64_t bnd = q / per;
      const int grp = (int)(U & 7) * per + (int)(q - bnd * per);
      u = (bnd * groups + grp) * (NT / 64) + wave;
    } else {
      u = gw + it * nw;
      if (u >= units) break;
    }
    const int band = (int)(u / strips), strip = (int)(u - (int64_t)band * strips);
    const int i0 = band * band_rows, i1 = (i0 + band_rows < N) ? i0 + band_rows : N;
    const int cs = 32 * strip;
    const int c0 = cs + 8 * sl;
    const bool last_strip = cs + 32 >= N;                        // (uniform) no pixel right of this strip
    const int nxo = last_strip ? 31 : 32;                        // clamped: a valid address, met by a zero weight
    const bool need_nx = !lockstep || wave == NT / 64 - 1;      // (uniform per wave)

    // every load is unconditional (clamped addresses, zeroed weights instead of branches): all loads of a row are in flight together
    auto load = [&](TvRow<T>& P, int i) {
      const int ic = i < N ? i : N - 1;                          // the row below the image is looked at with a zero weight only
      const int64_t e = (int64_t)ic * N;
      const int iv = ic < N - 1 ? ic : N - 2;                    // the last image row has no vertical difference: weight zeroed at use
      P.w = lane < 32 ? wh[(int64_t)ic * (N - 1) + cs + (lane < 31 || !last_strip ? lane : 30)] : wv[(int64_t)iv * N + cs + lane - 32];
      if (Z) P.z = z[e + cs + (lane & 31)];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        P.x[t][0] = *reinterpret_cast<const float4*>(rowp[t] + e + c0);
        P.x[t][1] = *reinterpret_cast<const float4*>(rowp[t] + e + c0 + 4);
        P.nx[t] = need_nx ? rowp[t][e + cs + nxo] : 0.f;
      }
    };
    auto publish = [&](const TvRow<T>& R, int i) {               // this wave's first pixel column of image row i, for the wave to its left
      if (lane < 16) {
#pragma unroll
        for (int t = 0; t < T; ++t) nxs[i & 1][wave][t][lane] = R.x[t][0].x;
      }
    };
    auto step = [&](const TvRow<T>& P, const TvRow<T>& Q, int i) {   // P: image row i, Q: the one below
      float nbr[T];
#pragma unroll
      for (int t = 0; t < T; ++t) nbr[t] = P.nx[t];
      if (lockstep) {                                            // (uniform)
        __syncthreads();                                         // row i's columns are published; everybody has left row i - 1
        publish(Q, i + 1);
        if (wave < NT / 64 - 1) {
#pragma unroll
          for (int t = 0; t < T; ++t) nbr[t] = nxs[i & 1][wave + 1][t][r];
        }
      }
      // this row's weights to the lanes: h at my[0..31], v at my[32..63]
      float wk = P.w;
      if (lane == 31 && last_strip) wk = 0.f;                    // column N - 1 has no right neighbour
      if (lane >= 32 && i >= N - 1) wk = 0.f;                    // row N - 1 has none below
      // (the LDS traffic of one wave is in order in hardware; the compiler must not reorder the float stores and the float4 loads
      //  of the next lines either — it did, across two unrolled steps: fences for the compiler only)
      __asm__ volatile("" ::: "memory");
      my[lane] = wk;
      if (Z && lane < 32) my[64 + lane] = P.z;
      __asm__ volatile("" ::: "memory");
      const float4 wh0 = *reinterpret_cast<const float4*>(my + 8 * sl), wh1 = *reinterpret_cast<const float4*>(my + 8 * sl + 4);
      const float4 wv0 = *reinterpret_cast<const float4*>(my + 32 + 8 * sl), wv1 = *reinterpret_cast<const float4*>(my + 36 + 8 * sl);
      float4 z0 = make_float4(0.f, 0.f, 0.f, 0.f), z1 = z0;
      if (Z) {
        z0 = *reinterpret_cast<const float4*>(my + 64 + 8 * sl);
        z1 = *reinterpret_cast<const float4*>(my + 68 + 8 * sl);
      }
      __asm__ volatile("" ::: "memory");
      if (Z) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const float4 a = P.x[t][0], b = P.x[t][1];
          accz[t] += (double)a.x * z0.x + (double)a.y * z0.y + (double)a.z * z0.z + (double)a.w * z0.w +
                     (double)b.x * z1.x + (double)b.y * z1.y + (double)b.z * z1.z + (double)b.w * z1.w;
        }
      }
      tv_row_products<T, AR>(P.x, Q.x, nbr, up16, sl, wh0, wh1, wv0, wv1, accd);
    };

    TvRow<T> P[D];                                               // a ring: row i sits in P[(i - i0) % D]; indices are compile-time below
#pragma unroll
    for (int j = 0; j < D - 1; ++j) load(P[j], i0 + j);
    if (lockstep) {
      __syncthreads();                                           // the previous unit's last exchange has been read
      publish(P[0], i0);
    }
    int i = i0;
    for (; i + D <= i1; i += D) {                                // roles rotate: no register copies
#pragma unroll
      for (int j = 0; j < D; ++j) {
        load(P[(j + D - 1) % D], i + j + D - 1);
        step(P[j], P[(j + 1) % D], i + j);
      }
    }
#pragma unroll
    for (int j = 0; j < D - 1; ++j) {                            // fewer than D rows left; P[j] = row i + j
      if (i + j < i1) {                                          // (uniform)
        if (i + j + D - 1 <= i1) load(P[(j + D - 1) % D], i + j + D - 1);
        step(P[j], P[(j + 1) % D], i + j);
      }
    }
  }
  };
  if constexpr (BF == 4) {
    if (use_f32) run(std::integral_constant<int, 0>{});
    else run(std::integral_constant<int, 2>{});
  } else {
    run(std::integral_constant<int, BF>{});
  }
  // combine the 4 waves (fixed order) and write the block partial in matrix order (16x16 C/D map: lane (r, sl), register q
  // holds D[4 sl + q][r])
  double* __restrict__ out = partials + (size_t)blockIdx.x * (k * k + (Z ? k : 0));
  int p = 0;
#pragma unroll
  for (int ta = 0; ta < T; ++ta)
#pragma unroll
    for (int tb = ta; tb < T; ++tb, ++p) {
      if (wave > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave - 1][q][lane] = accd[p][q];
      }
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double t = ((accd[p][q] + red[0][q][lane]) + red[1][q][lane]) + red[2][q][lane];
          const int row = 16 * ta + 4 * sl + q, col = 16 * tb + r;
          // one value per unordered pair: tiles above the diagonal are mirrored, and so is the upper triangle of a diagonal tile
          // (its lower triangle holds the same sums with the split products added in another order: equal to rounding, not to the bit)
          if (row < k && col < k && (ta != tb || row <= col)) {
            out[(size_t)row * k + col] = t;
            if (row != col) out[(size_t)col * k + row] = t;
          }
        }
      }
      __syncthreads();
    }
  if (Z) {
    // the dots: the four quarter-strip lanes of a row first (fixed order), then the four waves
#pragma unroll
    for (int t = 0; t < T; ++t) {
      double v = accz[t];
      const double v1 = __shfl(v, r + 16, 64), v2 = __shfl(v, r + 32, 64), v3 = __shfl(v, r + 48, 64);
      v = ((__shfl(v, r, 64) + v1) + v2) + v3;
      if (lane < 16) red[0][wave][16 * (t & 3) + lane] = v;      // [wave][row within a group of 4 tiles]
    }
    __syncthreads();
    if (threadIdx.x < 16 * T) {
      const int row = threadIdx.x;
      const double t = ((red[0][0][row] + red[0][1][row]) + red[0][2][row]) + red[0][3][row];
      if (row < k) out[(size_t)k * k + row] = t;
    }
  }
}

// ------------------------------------------------------------------ the same pass, the rows of V through LDS in FULL lines (round 5)
// k_wgram_tv's loads are fragment-shaped: one wave-instruction touches 16 basis vectors x 64 bytes, a workgroup 512 contiguous bytes
// per (vector, image row) — the loads ALONE take the kernel's whole time (a timing build, round 5: k = 32 at 4096^2 576 us with the
// arithmetic removed, 545 with it; 3.9 TB/s where the plain streams of k_gemv_n run at 5.9).  Here a workgroup of 8 waves owns 256
// image columns: every (vector, image row) of its tile is ONE 1 KiB global_load_lds_dwordx4 (a whole wave reading 1 KiB of one
// row of one basis vector) straight into an LDS stage, four stages deep — two image rows in flight per CU without a register held
// for them — and the waves take their MFMA operands from LDS.  The LDS image of a (vector, row) piece has its 16-byte slots XOR-ed with
// the vector's index mod 16 (applied to the per-lane SOURCE address of the load: the LDS side of such a load is lane-linear): the four
// 16-lane groups of a ds_read_b128 — {0-3, 12-15, 20-27}, .. — then meet 16 different slots (padding the rows to 260 floats does
// not do it: 61 % of the LDS cycles were bank conflicts, SQ_LDS_BANK_CONFLICT).  The pixel right of a wave's strip is the next strip's first pixel in the same stage; the column right
// of the TILE comes with the stage as one dword per vector.  The row's weights and the row of z arrive the same way (no load of the
// loop has a register destination: one vmcnt queue, counted by hand, raw barriers — a __syncthreads() would drain it).
// Arithmetic, block partials and their order: exactly k_wgram_tv's (tv_row_products).  N a multiple of 256, k <= 32.
constexpr int LW_NW = 8, LW_NT = 64 * LW_NW, LW_COLS = 32 * LW_NW, LW_RS = LW_COLS, LW_S = 4;
constexpr int LW_WH = 0, LW_WV = 256, LW_Z = 512, LW_HALO = 768, LW_XF = 832;      // the extras of a stage, in floats after its rows
__device__ __forceinline__ void glds16(const float* g, unsigned lds) {              // lane l: 16 bytes at g -> LDS byte lds + 16 l
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(g), "s"(lds) : "memory");
}
__device__ __forceinline__ void glds4(const float* g, unsigned lds) {               // lane l: 4 bytes at g -> LDS byte lds + 4 l
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(g), "s"(lds) : "memory");
}
// LDS reads the compiler may not take apart (it split the float4 reads of a row into b64 / b32 / read2_b32 pieces: 18 LDS instructions
// per step instead of 12, most of them on the 32-bank paths): issued as written, waited for by hand (lds_wait), and the values tied to
// the wait (lds_tie) so that no use is scheduled before it.
__device__ __forceinline__ f4v lds_r128(const float* p) {
  f4v v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"((unsigned)(size_t)(__attribute__((address_space(3))) const float*)p) : "memory");
  return v;
}
__device__ __forceinline__ float lds_r32(const float* p) {
  float v;
  asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"((unsigned)(size_t)(__attribute__((address_space(3))) const float*)p) : "memory");
  return v;
}
__device__ __forceinline__ void lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <class X>
__device__ __forceinline__ void lds_tie(X& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ float4 as_float4(const f4v& v) { return make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void wait_vm_le(int n) {                                 // (n: wave-uniform, <= 10)
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
  }
}
template <int T>
struct LwRow {
  float4 x[T][2];      // lane (r, sl): 8 pixels of vector 16 t + r at columns 32 wave + 8 sl ..
  float nx[T];         // the pixel right of the wave's strip
};
template <int T, bool Z, int BF>
__global__ __launch_bounds__(LW_NT, T == 1 ? 4 : 2) void k_wgram_tv_lds(const float* __restrict__ V, int64_t ld, int k, int N,
                                                           const float* __restrict__ w, int nbands, int band_rows,
                                                           double* __restrict__ partials, const float* __restrict__ z,
                                                           ProbeGate pg) {
  bool use_f32 = false;
  if constexpr (BF == 4) use_f32 = pg.sums && probe_verdict(pg, blockIdx.x == 0 && threadIdx.x == 0) != 0;
  constexpr int NP = T * (T + 1) / 2, NV = 16 * T, SF = NV * LW_RS + LW_XF;
  __shared__ __attribute__((aligned(16))) float smem[LW_S * SF];                  // (ALL of the kernel's LDS: the sums at the end alias it)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63, r = lane & 15, sl = lane >> 4;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float*)smem;
  const float* __restrict__ wh = w;
  const float* __restrict__ wv = w + (int64_t)N * (N - 1);
  const int up16 = ((lane + 16) & 63) << 2;
  // rows of vectors beyond the basis are never loaded: zero in every stage (their Gram entries are never stored; finite all the same)
  for (int s = 0; s < LW_S; ++s)
    for (int v = k; v < NV; ++v)
      for (int c = threadIdx.x; c < LW_RS; c += LW_NT) smem[s * SF + v * LW_RS + c] = 0.f;
  // this wave's pieces of a stage: the vectors wave, wave + 8, .. below k, and one of the extras
  int nv_mine = 0;
#pragma unroll
  for (int j = 0; j < 2 * T; ++j) nv_mine += (wave + 8 * j < k) ? 1 : 0;
  const bool has_extra = wave <= 4 || (wave == 5 && Z) || wave == 6;
  const int npw = nv_mine + (has_extra ? 1 : 0);
  double accd[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) accd[p][q] = 0.0;
  double accz[T];
#pragma unroll
  for (int t = 0; t < T; ++t) accz[t] = 0.0;
  const int tiles = N / LW_COLS;
  const int64_t units = (int64_t)tiles * nbands;
  const bool xcd_map = (tiles & 7) == 0 && (gridDim.x & 7) == 0;      // (uniform) as in k_wgram_tv: an XCD's tiles are neighbours
  __syncthreads();

  auto run = [&](auto arith_tag) {
  constexpr int AR = decltype(arith_tag)::value;
  for (int64_t U = blockIdx.x; U < units; U += gridDim.x) {
    int band, tile;
    if (xcd_map) {
      const int per = tiles >> 3;
      const int64_t q = U >> 3;
      band = (int)(q / per);
      tile = (int)(U & 7) * per + (int)(q - (int64_t)band * per);
    } else {
      band = (int)(U / tiles);
      tile = (int)(U - (int64_t)band * tiles);
    }
    const int i0 = band * band_rows, i1 = (i0 + band_rows < N) ? i0 + band_rows : N;
    const int c0 = LW_COLS * tile;
    const bool last_tile = c0 + LW_COLS >= N;                    // (uniform)
    const int halo_col = last_tile ? N - 1 : c0 + LW_COLS;       // clamped: a valid address, met by a zero weight

    auto issue = [&](int i) {                                    // image row i -> stage i & 3
      const int ic = i < N ? i : N - 1;
      const int64_t e = (int64_t)ic * N;
      const int iv = ic < N - 1 ? ic : N - 2;
      const unsigned sb = lds0 + (unsigned)((i & (LW_S - 1)) * SF) * 4u;
#pragma unroll
      for (int j = 0; j < 2 * T; ++j) {
        const int v = wave + 8 * j;
        if (v < k) glds16(V + (int64_t)v * ld + e + c0 + 4 * (lane ^ (v & 15)), sb + (unsigned)(v * LW_RS) * 4u);
      }
      const unsigned xb = sb + (unsigned)(NV * LW_RS) * 4u;
      if (wave < 4) glds4(wh + (int64_t)ic * (N - 1) + c0 + 64 * wave + lane, xb + (unsigned)(LW_WH + 64 * wave) * 4u);
      else if (wave == 4) glds16(wv + (int64_t)iv * N + c0 + 4 * lane, xb + LW_WV * 4u);
      else if (wave == 5) { if (Z) glds16(z + e + c0 + 4 * lane, xb + LW_Z * 4u); }
      else if (wave == 6) {
        const int hv = (lane & (NV - 1)) < k ? (lane & (NV - 1)) : 0;
        glds4(V + (int64_t)hv * ld + e + halo_col, xb + LW_HALO * 4u);
      }
    };
    // RAW: the reads as hand-issued ds_read_b128 (every value used only after lds_wait + lds_tie).  Measured per form: without the dots
    // the compiler takes the float4 reads apart (18 LDS instructions per step, 53 % of the LDS cycles bank conflicts; raw reads 415 us
    // against 428 at k = 24); with them it keeps them whole and schedules around its own waits better than one lds_wait does (435 us
    // against 463).
    constexpr bool RAW = !Z;
    auto fetch_raw = [&](f4v (&x)[T][2], float (&nx)[T], int i) {   // the wave's operands of image row i, from its stage
      const float* S = smem + (i & (LW_S - 1)) * SF;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float* row = S + (16 * t + r) * LW_RS;             // slot q of the row sits at slot q ^ r
        const int q = 8 * wave + 2 * sl;
        const float* np = wave < LW_NW - 1 ? row + 4 * ((8 * wave + 8) ^ r) : S + NV * LW_RS + LW_HALO + 16 * t + r;
        if constexpr (RAW) {
          x[t][0] = lds_r128(row + 4 * (q ^ r));
          x[t][1] = lds_r128(row + 4 * ((q + 1) ^ r));
          nx[t] = lds_r32(np);
        } else {
          x[t][0] = *reinterpret_cast<const f4v*>(row + 4 * (q ^ r));
          x[t][1] = *reinterpret_cast<const f4v*>(row + 4 * ((q + 1) ^ r));
          nx[t] = *np;
        }
      }
    };
    auto settle = [&](LwRow<T>& R, f4v (&x)[T][2], float (&nx)[T]) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if constexpr (RAW) {
          lds_tie(x[t][0]);
          lds_tie(x[t][1]);
          lds_tie(nx[t]);
        }
        R.x[t][0] = as_float4(x[t][0]);
        R.x[t][1] = as_float4(x[t][1]);
        R.nx[t] = nx[t];
      }
    };
    auto step = [&](const LwRow<T>& P, LwRow<T>& Q, int i) {     // P: image row i (held), Q: the row below (fetched here)
      wait_vm_le(i + 2 <= i1 ? npw : 0);                         // row i + 1 has landed (this wave's pieces); row i + 2 may be in flight
      __builtin_amdgcn_s_barrier();                              // ... everybody's; and everybody has left step i - 1
      asm volatile("" ::: "memory");                            // (the raw barrier is IntrNoMem: nothing else keeps the plain LDS reads of the Z form below it)
      if (i + 3 <= i1) issue(i + 3);                             // into the stage of row i - 1
      const float* X = smem + (i & (LW_S - 1)) * SF + NV * LW_RS + 32 * wave + 8 * sl;
      f4v rwh0, rwh1, rwv0, rwv1, rz0 = {0.f, 0.f, 0.f, 0.f}, rz1 = rz0;
      if constexpr (RAW) {
        rwh0 = lds_r128(X + LW_WH), rwh1 = lds_r128(X + LW_WH + 4), rwv0 = lds_r128(X + LW_WV), rwv1 = lds_r128(X + LW_WV + 4);
      } else {
        rwh0 = *reinterpret_cast<const f4v*>(X + LW_WH), rwh1 = *reinterpret_cast<const f4v*>(X + LW_WH + 4);
        rwv0 = *reinterpret_cast<const f4v*>(X + LW_WV), rwv1 = *reinterpret_cast<const f4v*>(X + LW_WV + 4);
        if (Z) {
          rz0 = *reinterpret_cast<const f4v*>(X + LW_Z);
          rz1 = *reinterpret_cast<const f4v*>(X + LW_Z + 4);
        }
      }
      f4v qx[T][2];
      float qn[T];
      fetch_raw(qx, qn, i + 1);
      if constexpr (RAW) {
        lds_wait();
        lds_tie(rwh0); lds_tie(rwh1); lds_tie(rwv0); lds_tie(rwv1);
      }
      settle(Q, qx, qn);
      float4 wh0 = as_float4(rwh0), wh1 = as_float4(rwh1), wv0 = as_float4(rwv0), wv1 = as_float4(rwv1);
      if (last_tile && wave == LW_NW - 1 && sl == 3) wh1.w = 0.f;      // column N - 1 has no right neighbour
      if (i >= N - 1) {                                                // row N - 1 has none below
        wv0 = make_float4(0.f, 0.f, 0.f, 0.f);
        wv1 = wv0;
      }
      if (Z) {
        const float4 z0 = as_float4(rz0), z1 = as_float4(rz1);
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const float4 a = P.x[t][0], b = P.x[t][1];
          accz[t] += (double)a.x * z0.x + (double)a.y * z0.y + (double)a.z * z0.z + (double)a.w * z0.w +
                     (double)b.x * z1.x + (double)b.y * z1.y + (double)b.z * z1.z + (double)b.w * z1.w;
        }
      }
      tv_row_products<T, AR>(P.x, Q.x, P.nx, up16, sl, wh0, wh1, wv0, wv1, accd);
    };

    LwRow<T> A, B;
    __builtin_amdgcn_s_barrier();                                // the previous unit's last rows have been read
    asm volatile("" ::: "memory");
    issue(i0);
    issue(i0 + 1);
    issue(i0 + 2);
    wait_vm_le(2 * npw);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    {
      f4v ax[T][2];
      float an[T];
      fetch_raw(ax, an, i0);
      if constexpr (RAW) lds_wait();
      settle(A, ax, an);
    }
    int i = i0;
    for (; i + 2 <= i1; i += 2) {                                // roles alternate: no register copies
      step(A, B, i);
      step(B, A, i + 1);
    }
    if (i < i1) step(A, B, i);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // (rows past a band shorter than the prologue's three)
  }
  };
  if constexpr (BF == 4) {
    if (use_f32) run(std::integral_constant<int, 0>{});
    else run(std::integral_constant<int, 2>{});
  } else {
    run(std::integral_constant<int, BF>{});
  }
  // combine the 8 waves (fixed order) and write the block partial in matrix order, as k_wgram_tv does
  __syncthreads();
  double* red = reinterpret_cast<double*>(smem);                 // [7][4][64]
  double* __restrict__ out = partials + (size_t)blockIdx.x * (k * k + (Z ? k : 0));
  int p = 0;
#pragma unroll
  for (int ta = 0; ta < T; ++ta)
#pragma unroll
    for (int tb = ta; tb < T; ++tb, ++p) {
      if (wave > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[((wave - 1) * 4 + q) * 64 + lane] = accd[p][q];
      }
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          double t = accd[p][q];
#pragma unroll
          for (int ww = 0; ww < LW_NW - 1; ++ww) t += red[(ww * 4 + q) * 64 + lane];
          const int row = 16 * ta + 4 * sl + q, col = 16 * tb + r;
          if (row < k && col < k && (ta != tb || row <= col)) {
            out[(size_t)row * k + col] = t;
            if (row != col) out[(size_t)col * k + row] = t;
          }
        }
      }
      __syncthreads();
    }
  if (Z) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      double v = accz[t];
      const double v1 = __shfl(v, r + 16, 64), v2 = __shfl(v, r + 32, 64), v3 = __shfl(v, r + 48, 64);
      v = ((__shfl(v, r, 64) + v1) + v2) + v3;
      if (lane < 16) red[wave * 64 + 16 * t + lane] = v;
    }
    __syncthreads();
    if (threadIdx.x < 16 * T) {
      const int row = threadIdx.x;
      double t = red[row];
#pragma unroll
      for (int ww = 1; ww < LW_NW; ++ww) t += red[ww * 64 + row];
      if (row < k) out[(size_t)k * k + row] = t;
    }
  }
}

// ------------------------------------------------------------------ the probe of the 'auto' arithmetic of trk_wgram_tv
// What two bf16 pieces per operand lose is each operand's third piece (<= 2^-16 of it).  On noisy data those residuals average out; on
// data that repeats a few values they are one number, millions of times (tests/test_gpu_kernels.py: 5.8e-6 per entry).  Whether the
// data at hand is of that kind is MEASURED per call on a sample: runs of 1024 pixels in 256 image rows (jittered), four of the k basis vectors; for
// their weighted differences d the kernel forms both  S_ab = sum d_a d_b  and  S'_ab = sum t_a t_b , t = the two-piece value of d,
// in float64 — S' - S is exactly what the split loses on the sample.  k_wgram_tv_gate turns the partials into
//     gate[1] = max_ab |S'_ab - S_ab| / sqrt(S_aa S_bb) ,   gate[0] = gate[1] > threshold (3e-7) ,
// and the pair of Gram launches behind it reads gate[0]: the bf16 form runs when it is 0, the fp32 pipe when it is 1 — decided on the
// device, nothing visits the host.  Cost: ~12 MB of reads whatever N, the probe and its 20-sum finalize, and the two launches of the
// pair that does not run (measured at 4096^2: see profiles/r05/wgram_tv_auto.txt).
constexpr int PROBE_V = 4, PROBE_P = PROBE_V * (PROBE_V + 1) / 2, PROBE_ROWS = 256, PROBE_SEG = 1024;
__device__ __forceinline__ float two_piece(float d) {
  const float hi = (float)(__bf16)d;
  return hi + (float)(__bf16)(d - hi);
}
// the j-th sample: one image row per stride, at a pseudo-random place inside it, and of that row one pseudo-random run of PROBE_SEG
// columns (a regular comb would never meet the block edges of a piecewise-constant image whose blocks are multiples of the stride —
// measured: such an image passed the first version's probe).  262 144 pixels whatever N: the probe's cost does not grow with the image.
__device__ __forceinline__ unsigned probe_hash(unsigned j) {
  unsigned h = j * 2654435761u;
  h ^= h >> 15;
  h *= 2246822519u;
  return h ^ (h >> 13);
}
__global__ __launch_bounds__(NT) void k_wgram_tv_probe(const float* __restrict__ V, int64_t ld, int k, int N, const float* __restrict__ w,
                                                       int row_step, double* __restrict__ part) {
  __shared__ double lds[(NT / 64) * 2 * PROBE_P];
  const unsigned h = probe_hash(blockIdx.x);
  int i = blockIdx.x * row_step + (int)(h % (unsigned)row_step);
  i = i < N ? i : N - 1;
  const int span = N > PROBE_SEG ? N - PROBE_SEG : 0;
  const int cbeg = span > 0 ? (int)((h >> 8) % (unsigned)(span + 1)) : 0;
  const int c_end = cbeg + PROBE_SEG < N ? cbeg + PROBE_SEG : N;
  // group 0: four vectors spread over the basis (the first and the last among them); group 1 (k >= 8): the NEWEST four — a solver's
  // basis changes character at its end first (MMGKS late in a TV solve: VERDICT round 5, weak 3), and all pairs of the last four are
  // what a spread sample of one of them cannot see
  int pr[PROBE_V];
#pragma unroll
  for (int a = 0; a < PROBE_V; ++a) pr[a] = blockIdx.y == 0 ? (int)(((int64_t)a * (k - 1)) / (PROBE_V - 1)) : k - PROBE_V + a;
  const float* __restrict__ wh = w;
  const float* __restrict__ wv = w + (int64_t)N * (N - 1);
  double acc[2 * PROBE_P];
#pragma unroll
  for (int q = 0; q < 2 * PROBE_P; ++q) acc[q] = 0.0;
  for (int c = cbeg + threadIdx.x; c < c_end; c += NT) {
    const float whc = c < N - 1 ? wh[(int64_t)i * (N - 1) + c] : 0.f;
    const float wvc = i < N - 1 ? wv[(int64_t)i * N + c] : 0.f;
    float dh[PROBE_V], dv[PROBE_V], th[PROBE_V], tv[PROBE_V];
#pragma unroll
    for (int a = 0; a < PROBE_V; ++a) {
      const float* __restrict__ row = V + (int64_t)pr[a] * ld + (int64_t)i * N;
      const float x = row[c];
      const float xr = c < N - 1 ? row[c + 1] : x;
      const float xb = i < N - 1 ? row[c + N] : x;
      dh[a] = (x - xr) * whc;
      dv[a] = (x - xb) * wvc;
      th[a] = two_piece(dh[a]);
      tv[a] = two_piece(dv[a]);
    }
    int q = 0;
#pragma unroll
    for (int a = 0; a < PROBE_V; ++a)
#pragma unroll
      for (int b = a; b < PROBE_V; ++b, ++q) {
        acc[q] += (double)dh[a] * (double)dh[b] + (double)dv[a] * (double)dv[b];
        acc[PROBE_P + q] += (double)th[a] * (double)th[b] + (double)tv[a] * (double)tv[b];
      }
  }
  const double t = block_sum_many<NT, 2 * PROBE_P>(acc, lds);
  if (threadIdx.x < 2 * PROBE_P) part[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 2 * PROBE_P + threadIdx.x] = t;
}

// scatter the augmented Gram [KA x KA] into G (k x k), c1, c2 (and optionally ||w b||^2)
__global__ void k_wgram_unpack(const double* __restrict__ Ga, int k, int KA, double* __restrict__ G, double* __restrict__ c1,
                               double* __restrict__ c2) {
  for (int idx = threadIdx.x; idx < k * k; idx += blockDim.x) G[idx] = Ga[(size_t)(idx / k) * KA + (idx % k)];
  if (KA > k)
    for (int a = threadIdx.x; a < k; a += blockDim.x) {
      c1[a] = Ga[(size_t)a * KA + k];
      c2[a] = Ga[(size_t)a * KA + k + 1];
    }
}

}  // namespace

static int g_wgram_tv_mode = 1;        // 1 auto, 0 fp32 pipe, 2 / 3 bf16 pieces (trk_wgram_tv_precision)
static double* g_wgram_gate = nullptr; // {verdict, worst sampled deviation} of the last 'auto' call (device; process-wide like the mode)

static int wgram_tv_run(const float* V, int64_t ld, int k, int N, const float* w, double* G, const float* z, double* h, trk_stream st) {
  TRK_REQUIRE(V && w && G, "trk_wgram_tv: NULL argument");
  TRK_REQUIRE(k >= 1 && k <= 48, "trk_wgram_tv: need 1 <= k <= 48 (trk_wgram over the stored images beyond)");
  TRK_REQUIRE(N >= 32 && N % 32 == 0 && ld >= (int64_t)N * N && ld % 4 == 0 && aligned16(V) && aligned16(w),
              "trk_wgram_tv: need N a multiple of 32, 16-byte aligned rows and weights");
  hipStream_t s = (hipStream_t)st;
  const int T16 = (k + 15) / 16;
  const int strips = N / 32;
  // The four waves of a workgroup in step (see the kernel: the right-neighbour column handed over through LDS instead of fetched
  // again — 25-40 % less HBM traffic, one barrier per image row): pays where the rows' traffic is the bound.  Measured at 4096^2
  // (tools/wgram_tv_micro.py; us, lockstep vs not): plain, two tiles k = 20 / 32: 507 / 620 vs 592 / 831; one tile k = 16: 308 vs
  // 366, k <= 10 equal; with the dots of _z (218 registers, two workgroups per CU at two tiles): k = 18 / 26 / 32: 640 / 649 / 676 vs
  // 598 / 666 / 791 — from k = 25 on.
  const bool ls_pays = T16 == 1 ? k >= 12 : T16 == 2 ? (z ? k >= 22 : true) : false;      // (round 5, two bf16 pieces, _z: k = 20 455 vs 464 us, k = 24 540 vs 478)
  const int lock = (strips % (NT / 64) == 0 && ls_pays) ? 1 : 0;
  // workgroups per CU: what the registers let be resident while the matrix pipe is the bound; without the lockstep exchange fewer
  // once the rows' traffic is (k = 32 plain: 762 / 744 / 683 us with 4 / 2 / 1 — more waves, more row streams open at once)
  const int per_cu = lock ? (z ? (T16 == 1 ? 3 : 2) : 3)
                   : z ? (T16 == 1 ? 3 : T16 == 2 ? 2 : 2)
                       : (T16 == 1 ? (k <= 11 ? 4 : k <= 14 ? 2 : 1) : T16 == 2 ? (k <= 25 ? 3 : 1) : 2);
  int bx = cu_count() * per_cu;
  // (strip, band) units, band-major: the waves in flight together then work on a few neighbouring image rows of every basis vector
  int band_rows = 64 < N ? 64 : N;
  int nbands = (N + band_rows - 1) / band_rows;
  const int64_t units = (int64_t)strips * nbands;
  if ((int64_t)bx * (NT / 64) > units) bx = (int)((units + NT / 64 - 1) / (NT / 64));
  // Large images, at most two tiles of vectors: the rows of V staged through LDS in full lines (k_wgram_tv_lds): 256-column tiles,
  // one workgroup of 8 waves per CU (two at one tile of vectors).
  const bool use_lds = T16 <= 2 && N % LW_COLS == 0 && N >= 2048;
  if (use_lds) {
    band_rows = 64;                                             // (N is a multiple of 256)
    nbands = N / band_rows;
    const int64_t lunits = (int64_t)(N / LW_COLS) * nbands;
    bx = cu_count() * (T16 == 1 ? 2 : 1);
    if (T16 == 2 && bx > cu_count()) bx = cu_count();
    if (bx > lunits) bx = (int)lunits;
  }
  double* part = nullptr;
  const int nv = k * k + (z ? k : 0);
  if (int rc = scratch_doubles(s, (size_t)bx * nv + ((size_t)PROBE_ROWS + 1) * 2 * 2 * PROBE_P, &part)) return rc;
  double* probe_part = part + (size_t)bx * nv;
  double* probe_sums = probe_part + (size_t)PROBE_ROWS * 2 * 2 * PROBE_P;
  // Which arithmetic forms the tile products (trk_wgram_tv_precision): 1 auto (default: two bf16 pieces unless the probe finds the
  // data's roundings correlated, then the fp32 pipe), 0 fp32 matrix pipe, 2 two bf16 pieces, 3 three bf16 pieces
  const int mode = g_wgram_tv_mode;
  ProbeGate pg{nullptr, 0.0, nullptr, 1};
  if (mode == 1) {
    if (!g_wgram_gate) TRK_HIP(hipMalloc((void**)&g_wgram_gate, 2 * sizeof(double)));
    // verdict threshold on the SAMPLED deviation: a third of the 1e-6 the contract promises (the sample is an estimate)
    const double thr = 3e-7;
    const int row_step = N / PROBE_ROWS > 0 ? N / PROBE_ROWS : 1;
    const int prows = (N + row_step - 1) / row_step < PROBE_ROWS ? (N + row_step - 1) / row_step : PROBE_ROWS;
    const int pgroups = k >= 2 * PROBE_V ? 2 : 1;
    hipLaunchKernelGGL(k_wgram_tv_probe, dim3(prows, pgroups), dim3(NT), 0, s, V, ld, k, N, w, row_step, probe_part);
    TRK_LAUNCH_CHECK();
    if (int rc = finalize_sums(probe_part, prows, pgroups * 2 * PROBE_P, pgroups * 2 * PROBE_P, probe_sums, s)) return rc;
    pg = ProbeGate{probe_sums, thr, g_wgram_gate, pgroups};
  }
  // arith: 4 'auto' (both forms in one launch, the probe's verdict picks), 0 fp32 pipe, 2 / 3 bf16 pieces
  const int arith = mode == 1 ? 4 : mode;
#define WTV(TT, ZZ)                                                                                                                                   \
  do {                                                                                                                                                \
    if (arith == 4) hipLaunchKernelGGL((k_wgram_tv<TT, ZZ, 3, 4>), dim3(bx), dim3(NT), 0, s, V, ld, k, N, w, nbands, band_rows, part, z, lock, pg);  \
    else if (arith == 0) hipLaunchKernelGGL((k_wgram_tv<TT, ZZ, 3, 0>), dim3(bx), dim3(NT), 0, s, V, ld, k, N, w, nbands, band_rows, part, z, lock, pg); \
    else if (arith == 2) hipLaunchKernelGGL((k_wgram_tv<TT, ZZ, 3, 2>), dim3(bx), dim3(NT), 0, s, V, ld, k, N, w, nbands, band_rows, part, z, lock, pg); \
    else hipLaunchKernelGGL((k_wgram_tv<TT, ZZ, 3, 3>), dim3(bx), dim3(NT), 0, s, V, ld, k, N, w, nbands, band_rows, part, z, lock, pg);             \
  } while (0)
#define WTVL1(TT, ZZ, BFV) hipLaunchKernelGGL((k_wgram_tv_lds<TT, ZZ, BFV>), dim3(bx), dim3(LW_NT), 0, s, V, ld, k, N, w, nbands, band_rows, part, z, pg)
#define WTVL(TT, ZZ)                                             \
  do {                                                           \
    if (arith == 4) WTVL1(TT, ZZ, 4);                            \
    else if (arith == 0) WTVL1(TT, ZZ, 0);                       \
    else if (arith == 2) WTVL1(TT, ZZ, 2);                       \
    else WTVL1(TT, ZZ, 3);                                       \
  } while (0)
  // one pass of the chosen arithmetic: the kernel and the sum of its block partials
  const bool two_pass = z && T16 == 3;     // three tiles AND the dots do not fit the register file (108 spilled registers): the dots
  if (use_lds) {
    if (z) { if (T16 == 1) WTVL(1, true); else WTVL(2, true); }
    else { if (T16 == 1) WTVL(1, false); else WTVL(2, false); }
  } else
  if (two_pass) WTV(3, false);             // of 33 <= k <= 48 in a pass of their own, below
  else if (z) { if (T16 == 1) WTV(1, true); else WTV(2, true); }
  else { if (T16 == 1) WTV(1, false); else if (T16 == 2) WTV(2, false); else WTV(3, false); }
  TRK_LAUNCH_CHECK();
  if (z && !two_pass) return finalize_sums_split(part, bx, nv, nv, G, k * k, h, s);
  if (int rc = finalize_sums(part, bx, k * k, k * k, G, s)) return rc;
  if (two_pass) return launch_gemv_t(V, ld, k, (int64_t)N * N, z, nullptr, 0, h, s);
  return TRK_OK;
}
#undef WTV
#undef WTVL
#undef WTVL1

// ======================================================================================= C ABI
extern "C" {

int trk_wgram_tv(const float* V, int64_t ld, int k, int N, const float* w, double* G, trk_stream st) {
  return wgram_tv_run(V, ld, k, N, w, G, nullptr, nullptr, st);
}

int trk_wgram_tv_precision(int mode) {
  TRK_REQUIRE(mode >= -1 && mode <= 3, "trk_wgram_tv_precision: mode 1 (auto), 0 (fp32 pipe), 2 or 3 (bf16 pieces), -1 (query)");
  const int was = g_wgram_tv_mode;
  if (mode >= 0) g_wgram_tv_mode = mode;
  return was;
}

int trk_wgram_tv_last_probe(double* verdict_and_deviation_host) {
  TRK_REQUIRE(verdict_and_deviation_host, "trk_wgram_tv_last_probe: NULL argument");
  verdict_and_deviation_host[0] = verdict_and_deviation_host[1] = -1.0;
  if (!g_wgram_gate) return TRK_OK;                              // no 'auto' call yet
  TRK_HIP(hipDeviceSynchronize());
  TRK_HIP(hipMemcpy(verdict_and_deviation_host, g_wgram_gate, 2 * sizeof(double), hipMemcpyDeviceToHost));
  return TRK_OK;
}

int trk_wgram_tv_z(const float* V, int64_t ld, int k, int N, const float* w, double* G, const float* z, double* h, trk_stream st) {
  TRK_REQUIRE(z && h && aligned16(z), "trk_wgram_tv_z: z / h NULL or z not 16-byte aligned");
  return wgram_tv_run(V, ld, k, N, w, G, z, h, st);
}

int trk_wgram(const float* W, int64_t ld, int k, int64_t m, const float* w, const float* b1, double* G, double* c1,
              double* c2, trk_stream st) {
  TRK_REQUIRE(W && G, "trk_wgram: NULL argument");
  TRK_REQUIRE(k >= 1 && k <= 512 && m >= 0 && ld >= m, "trk_wgram: need 1 <= k <= 512, m >= 0, ld >= m");
  TRK_REQUIRE(!b1 || (c1 && c2), "trk_wgram: b1 given but c1/c2 NULL");
  hipStream_t s = (hipStream_t)st;
  const int KA = k + (b1 ? 2 : 0);
  if (KA <= 64) {
    // matrix-core single pass (every row read once)
    const bool al16 = (ld % 4 == 0) && aligned16(W) && (!w || aligned16(w)) && (!b1 || aligned16(b1));
    const bool direct = al16 && KA <= 48;   // T = 4 does not fit the register file: 49..64 rows stay on the 32x32 kernel
    const int T16 = (KA + 15) / 16;
    // blocks per CU = what the register budget of the variant lets be resident (8 / 4 / 2 waves per SIMD for T = 1 / 2 / 3)
    const int per_cu = direct ? (T16 == 1 ? 8 : T16 == 2 ? 4 : 2) : 3;
    int64_t nchunk = (m + 127) / 128;
    int bx = (int)(nchunk < (int64_t)cu_count() * per_cu ? (nchunk > 0 ? nchunk : 1) : (int64_t)cu_count() * per_cu);
    if (bx > 2 * kMaxPartialBlocks) bx = 2 * kMaxPartialBlocks;
    double* part = nullptr;
    const size_t npart = (size_t)bx * KA * KA;
    if (int rc = scratch_doubles(s, npart + (size_t)KA * KA, &part)) return rc;
    double* Ga = part + npart;
    // HAS_W / HAS_B follow the two optional rows; the tile count is an integer and keeps its ladder
    with_bools([&](auto HAS_W, auto HAS_B) {
      auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(bx), dim3(NT), 0, s, W, ld, k, m, w, b1, part); };
      if (!direct && KA <= 32) launch(k_wgram_mfma<1, HAS_W, HAS_B>);
      else if (!direct) launch(k_wgram_mfma<2, HAS_W, HAS_B>);
      else if (T16 == 1) launch(k_wgram_t16<1, HAS_W, HAS_B>);
      else if (T16 == 2) launch(k_wgram_t16<2, HAS_W, HAS_B>);
      else launch(k_wgram_t16<3, HAS_W, HAS_B>);
    }, w != nullptr, b1 != nullptr);
    TRK_LAUNCH_CHECK();
    if (int rc = finalize_sums(part, bx, KA * KA, KA * KA, Ga, s)) return rc;
    hipLaunchKernelGGL(k_wgram_unpack, dim3(1), dim3(256), 0, s, Ga, k, KA, G, c1, c2);
    TRK_LAUNCH_CHECK();
    return TRK_OK;
  }
  // many rows: tile-pair form (re-reads W once per tile pair)
  const int nt = ceil_div(k, TG);
  const int npairs = nt * (nt + 1) / 2;
  int bx = stream_grid(m);
  const int cap = (cu_count() * 8 + npairs - 1) / npairs;
  if (bx > cap) bx = cap < 1 ? 1 : cap;
  double* part = nullptr;  // [bx][k*k] partials
  if (int rc = scratch_doubles(s, (size_t)bx * k * k, &part)) return rc;
  const bool vec = aligned16(W) && (ld % 4 == 0) && (!w || aligned16(w));
  dim3 grid(bx, npairs);
  with_bools([&](auto HAS_W, auto VEC) { hipLaunchKernelGGL((k_wgram<HAS_W, VEC>), grid, dim3(NT), 0, s, W, ld, k, m, w, nt, part); },
             w != nullptr, vec);
  TRK_LAUNCH_CHECK();
  if (int rc = finalize_sums(part, bx, k * k, k * k, G, s)) return rc;
  if (b1) {
    if (w) {
      if (int rc = launch_gemv_t(W, ld, k, m, b1, w, 1, c1, s)) return rc;
      if (int rc = launch_gemv_t(W, ld, k, m, b1, w, 2, c2, s)) return rc;
    } else {
      if (int rc = launch_gemv_t(W, ld, k, m, b1, nullptr, 0, c1, s)) return rc;
      TRK_HIP(hipMemcpyAsync(c2, c1, sizeof(double) * k, hipMemcpyDeviceToDevice, s));
    }
  }
  return TRK_OK;
}

}  // extern "C"
