// framelet2d.hip — separable band operator y = vec_F(W_n X W_m^T) and its transpose x = vec_F(W_n^T Y W_m): the reference's framelet
// analysis operator (trips/utilities/operators.py:50-113) applied matrix-free, the way the reference applies it, instead of as the CSR
// of kron(W_m, W_n) (169 non-zeros per pixel at level 2).  X = x.reshape(n, m, order='F'): X[i, j] = x[i + n j];
// y[p + R_n q], R_n = blocks_n n, p = b n + i, q = c m + j — oracle.cpu_ref.Framelet2D's layout.
//
// W_n (blocks_n n x n) and W_m are band matrices: row b n + i has its non-zeros in columns i - half .. i + half.  In the interior of a
// block every row is one stencil, shifted; the first and last `half` rows carry the half-sample reflection folded into their
// coefficients, so no kernel reflects an index: what lies outside the image is read as 0 and meets a coefficient that is 0.
//
// Both kernels: one wave per workgroup, lane <-> image row i (x, y and every sub-band are contiguous in i), TJ image columns per lane.
//   forward   the X tile plus halo and the tile's taps along j go to LDS; per row block b the lane filters along i (2H+1 LDS reads
//             per column) into TJ + 2H registers, then per column block c along j in registers and stores — runs of 64 floats
//             contiguous in p.
//   transpose per row block b the lane gathers Y[b n + i', (c, j')] over all c and the tile's columns plus halo straight from memory
//             into TJ sums (the taps of W_m from LDS, wave-uniform), parks them in LDS, and the lanes of the 64 - 2H output rows add
//             the 2H+1 neighbours' sums with the column taps of W_n.  A gather in a fixed order: no atomics, two runs agree to the bit.
// A tile's taps come from the block's stencil when all its rows (columns) are interior and from the per-row table when it touches
// an edge: the same code, another source of taps (taps along i per lane, table layout [b][t][i]; taps along j staged per tile).
// H is the compile-time half-width (1, 2, 4 or 7: levels 1 .. 4); narrower bands are padded with zero taps.
// Design, register counts and measurements: docs/kernels/framelet.md.
#include "trk_internal.h"

#include <cmath>
#include <vector>

using namespace trk;

namespace {

constexpr int WAVE = 64;
constexpr int kMaxHalf = 7;
constexpr int64_t kSmallGridTiles = 2048;
constexpr int kMaxBlocks = 32;                     // the transpose stages 32 blocks x (4 + 14) rows x 16 taps x 4 bytes = 36 KB of LDS at H = 7
// non-temporal stores of the forward output from this many floats (the 256 MiB memory-side cache): nothing downstream finds it cached
constexpr int64_t kFrameletNtStoreFloats = (int64_t)64 << 20;

struct FrImpl {
  int n, m, bn, bm, H;
  float* tab;            // one allocation: tn [bn][2H+1][n] | sn [bn][2H+1] | tm [bm][m][2H+1] | sm [bm][2H+1]
  const float *tn, *sn, *tm, *sm;
};

struct FrGeom {
  int n, m, bn, bm, tiles_i;
};

// taps per table row in LDS, padded to a multiple of four floats (16-byte rows: the wave-uniform reads can be 128 bits wide)
constexpr int padded_taps(int H) { return (2 * H + 1 + 3) / 4 * 4; }

// The taps along j of the NR = TJ (forward: output columns j0 ..) or TJ + 2H (transpose: rows j' = j0 - H ..) table rows a tile uses,
// for every column block, into LDS as wms[c][r][t] — the block's stencil in every row when the tile's columns are interior, the
// table's rows otherwise, zeros for rows outside [0, m).  One round trip per tile instead of one per (b, c) trip of the loops below,
// whose scalar loads of the taps each waited for the scalar cache (512^2, l = 2: forward 26 -> 18 us, docs/kernels/framelet.md).
template <int H, int NR>
__device__ __forceinline__ void stage_taps_j(float* __restrict__ wms, const float* __restrict__ tm, const float* __restrict__ sm, int bm, int m,
                                             int jfirst, bool interior) {
  constexpr int W = 2 * H + 1, WP = padded_taps(H);
  for (int k = threadIdx.x; k < bm * NR * WP; k += WAVE) {
    const int c = k / (NR * WP), r = (k / WP) % NR, t = k % WP, j = jfirst + r;
    float v = 0.f;
    if (t < W && j >= 0 && j < m) v = interior ? sm[c * W + t] : tm[((int64_t)c * m + j) * W + t];
    wms[k] = v;
  }
}

template <int H, int TJ, bool NTS>
__global__ __launch_bounds__(WAVE) void k_framelet_fwd(FrGeom g, const float* __restrict__ tn, const float* __restrict__ sn,
                                                       const float* __restrict__ tm, const float* __restrict__ sm,
                                                       const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy) {
  constexpr int W = 2 * H + 1, WP = padded_taps(H), NJ = TJ + 2 * H, LR = WAVE + 2 * H;
  extern __shared__ float4 lds4[];
  float* __restrict__ wms = reinterpret_cast<float*>(lds4);          // [bm][TJ][WP]
  float(*xs)[LR] = reinterpret_cast<float(*)[LR]>(wms + g.bm * TJ * WP);   // [NJ][LR]
  const int lane = threadIdx.x, n = g.n, m = g.m;
  const int i0 = (int)(blockIdx.x % g.tiles_i) * WAVE, j0 = (int)(blockIdx.x / g.tiles_i) * TJ;
  x += (int64_t)blockIdx.y * ldx;
  y += (int64_t)blockIdx.y * ldy;
  const bool int_i = i0 >= H && i0 + WAVE - 1 <= n - 1 - H;        // wave-uniform: every row / column of the tile is interior
  const bool int_j = j0 >= H && j0 + TJ - 1 <= m - 1 - H;
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj) {
    const int j = j0 - H + jj;
    const bool cj = j >= 0 && j < m;
    for (int r = lane; r < LR; r += WAVE) {
      const int i = i0 - H + r;
      xs[jj][r] = (cj && i >= 0 && i < n) ? x[i + (int64_t)n * j] : 0.f;
    }
  }
  stage_taps_j<H, TJ>(wms, tm, sm, g.bm, m, j0, int_j);
  const unsigned i = i0 + lane;
  const bool live = (int)i < n;
  const int ic = live ? (int)i : n - 1;
  const int64_t Rn = (int64_t)g.bn * n;
  // the taps along i of row block b: the block's stencil or this lane's table row, fetched one block ahead of their use
  float wnext[W];
#pragma unroll
  for (int t = 0; t < W; ++t) wnext[t] = int_i ? sn[t] : tn[(int64_t)t * n + ic];
  __syncthreads();
  for (int b = 0; b < g.bn; ++b) {
    float wn[W];
    const int bnext = b + 1 < g.bn ? b + 1 : b;
#pragma unroll
    for (int t = 0; t < W; ++t) {
      wn[t] = wnext[t];
      wnext[t] = int_i ? sn[bnext * W + t] : tn[((int64_t)bnext * W + t) * n + ic];
    }
    float T[NJ];
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      float a = 0.f;
#pragma unroll
      for (int t = 0; t < W; ++t) a = fmaf(wn[t], xs[jj][lane + t], a);
      T[jj] = a;
    }
    for (int c = 0; c < g.bm; ++c) {
      const float* __restrict__ wm = wms + c * TJ * WP;
      float* __restrict__ ycol = y + (int64_t)b * n + Rn * ((int64_t)c * m + j0);      // wave-uniform; the lane adds its row
#pragma unroll
      for (int jl = 0; jl < TJ; ++jl) {
        float a = 0.f;
#pragma unroll
        for (int t = 0; t < W; ++t) a = fmaf(wm[jl * WP + t], T[jl + t], a);
        if (live && j0 + jl < m) {
          if (NTS) __builtin_nontemporal_store(a, &ycol[Rn * jl + i]);
          else ycol[Rn * jl + i] = a;
        }
      }
    }
  }
}

// the transpose's sums along j for one row block: Z[jl] += sum over c and j' of Y[b n + i', c m + j'] W_m[c m + j', j0 + jl].
// JIN: every column j' = j0 - H .. j0 + TJ - 1 + H lies inside [0, m) (no test per load).
template <int H, int TJ, bool JIN>
__device__ __forceinline__ void gather_j(float (&Z)[TJ], const float* __restrict__ yrow, unsigned loff, int64_t Rn, int bm, int m, int j0,
                                         const float* __restrict__ wms) {
  constexpr int W = 2 * H + 1, WP = padded_taps(H), NJ = TJ + 2 * H;
  auto load = [&](int c, float (&v)[NJ]) {
    const float* __restrict__ ycol = yrow + Rn * ((int64_t)c * m + j0 - H);              // wave-uniform
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      const int jp = j0 - H + jj;
      v[jj] = (JIN || (jp >= 0 && jp < m)) ? ycol[Rn * jj + loff] : 0.f;
    }
  };
  auto add = [&](int c, const float (&v)[NJ]) {
    const float* __restrict__ wm = wms + c * NJ * WP;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
#pragma unroll
      for (int t = 0; t < W; ++t) {
        const int jl = jj + t - 2 * H;                             // W_m[c m + j', j0 + jl] = band_m[c][j'][H + j - j']
        if (jl >= 0 && jl < TJ) Z[jl] = fmaf(wm[jj * WP + t], v[jj], Z[jl]);
      }
    }
  };
  // two column blocks per trip: their 2 (TJ + 2H) loads are in flight together; the sums stay in the order c = 0, 1, ...
  int c = 0;
  for (; c + 1 < bm; c += 2) {
    float v0[NJ], v1[NJ];
    load(c, v0);
    load(c + 1, v1);
    add(c, v0);
    add(c + 1, v1);
  }
  if (c < bm) {
    float v0[NJ];
    load(c, v0);
    add(c, v0);
  }
}

template <int H, int TJ>
__global__ __launch_bounds__(WAVE) void k_framelet_adj(FrGeom g, const float* __restrict__ tn, const float* __restrict__ sn,
                                                       const float* __restrict__ tm, const float* __restrict__ sm,
                                                       const float* __restrict__ yin, int64_t ldin, float* __restrict__ xout,
                                                       int64_t ldout) {
  constexpr int W = 2 * H + 1, WP = padded_taps(H), NJ = TJ + 2 * H, TI = WAVE - 2 * H;
  extern __shared__ float4 lds4[];
  float* __restrict__ wms = reinterpret_cast<float*>(lds4);          // [bm][NJ][WP]
  float(*zs)[WAVE] = reinterpret_cast<float(*)[WAVE]>(wms + g.bm * NJ * WP);   // [TJ][WAVE]
  const int lane = threadIdx.x, n = g.n, m = g.m;
  const int i0 = (int)(blockIdx.x % g.tiles_i) * TI, j0 = (int)(blockIdx.x / g.tiles_i) * TJ;
  yin += (int64_t)blockIdx.y * ldin;
  xout += (int64_t)blockIdx.y * ldout;
  const int ip = i0 - H + lane;                                    // the row i' whose sums along j this lane forms
  const bool live_in = ip >= 0 && ip < n;
  const int ipc = ip < 0 ? 0 : (ip > n - 1 ? n - 1 : ip);          // (a lane outside the image reads a valid row; its sums are dropped)
  const int i = i0 + lane;                                         // the output row of lanes 0 .. TI - 1: its neighbours i - H + t are lanes lane + t
  const bool out_lane = lane < TI && i < n;
  const bool int_i = i0 - H >= H && i0 - H + WAVE - 1 <= n - 1 - H;  // wave-uniform: every row i' / column j' the tile reads is interior
  const bool int_j = j0 - H >= H && j0 + TJ - 1 + H <= m - 1 - H;
  const bool jin = j0 - H >= 0 && j0 + TJ - 1 + H <= m - 1;
  const int64_t Rn = (int64_t)g.bn * n;
  stage_taps_j<H, NJ>(wms, tm, sm, g.bm, m, j0 - H, int_j);
  __syncthreads();
  float acc[TJ];
#pragma unroll
  for (int jl = 0; jl < TJ; ++jl) acc[jl] = 0.f;
  for (int b = 0; b < g.bn; ++b) {
    // the column taps of W_n this lane's output row needs from block b, W_n[b n + i', i] = band_n[b][i'][2H - t] for i' = i - H + t:
    // requested before the gather, used after it
    float wn[W];
#pragma unroll
    for (int t = 0; t < W; ++t) {
      int ipt = i - H + t;
      ipt = ipt < 0 ? 0 : (ipt > n - 1 ? n - 1 : ipt);             // (outside the image the parked sum is 0; any valid address will do)
      wn[t] = int_i ? sn[b * W + 2 * H - t] : tn[((int64_t)b * W + 2 * H - t) * n + ipt];
    }
    float Z[TJ];
#pragma unroll
    for (int jl = 0; jl < TJ; ++jl) Z[jl] = 0.f;
    const float* __restrict__ yrow = yin + (int64_t)b * n;
    if (jin) gather_j<H, TJ, true>(Z, yrow, (unsigned)ipc, Rn, g.bm, m, j0, wms);
    else gather_j<H, TJ, false>(Z, yrow, (unsigned)ipc, Rn, g.bm, m, j0, wms);
    __syncthreads();
#pragma unroll
    for (int jl = 0; jl < TJ; ++jl) zs[jl][lane] = live_in ? Z[jl] : 0.f;
    __syncthreads();
    if (out_lane) {
#pragma unroll
      for (int t = 0; t < W; ++t) {
#pragma unroll
        for (int jl = 0; jl < TJ; ++jl) acc[jl] = fmaf(wn[t], zs[jl][lane + t], acc[jl]);
      }
    }
  }
  if (out_lane) {
#pragma unroll
    for (int jl = 0; jl < TJ; ++jl)
      if (j0 + jl < m) xout[i + (int64_t)n * (j0 + jl)] = acc[jl];
  }
}

// sum of squares of `batch` vectors of nout floats, ld apart: block partials [batch][gridDim.x] for finalize_sums
__global__ __launch_bounds__(256) void k_framelet_sumsq(const float* __restrict__ y, int64_t ld, int64_t nout, double* __restrict__ part) {
  __shared__ double red[4];
  const float* __restrict__ yb = y + (int64_t)blockIdx.y * ld;
  double a0 = 0.0, a1 = 0.0;
  const int64_t step = (int64_t)gridDim.x * 256;
  int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; k + step < nout; k += 2 * step) {
    const float u = yb[k], v = yb[k + step];
    a0 += (double)u * u;
    a1 += (double)v * v;
  }
  if (k < nout) a0 += (double)yb[k] * yb[k];
  const double t = block_sum<256>(a0 + a1, red);
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

template <int H, int TJ>
void fr_launch_fwd(const FrImpl* im, const float* x, int64_t ldx, float* y, int64_t ldy, int batch, hipStream_t s) {
  constexpr int WP = padded_taps(H), NJ = TJ + 2 * H;
  const int tiles_i = (im->n + WAVE - 1) / WAVE;
  const FrGeom g{im->n, im->m, im->bn, im->bm, tiles_i};
  const dim3 grid((unsigned)((int64_t)tiles_i * ((im->m + TJ - 1) / TJ)), (unsigned)batch);
  const size_t lds = sizeof(float) * ((size_t)im->bm * TJ * WP + (size_t)NJ * (WAVE + 2 * H));
  const bool nts = (int64_t)im->bn * im->n * im->bm * im->m >= kFrameletNtStoreFloats;
  with_bools([&](auto NTS) {
    hipLaunchKernelGGL((k_framelet_fwd<H, TJ, NTS>), grid, dim3(WAVE), lds, s, g, im->tn, im->sn, im->tm, im->sm, x, ldx, y, ldy);
  }, nts);
}

// the transpose runs with four columns per lane at every size (measured: docs/kernels/framelet.md)
template <int H>
void fr_launch_adj(const FrImpl* im, const float* y, int64_t ldy, float* x, int64_t ldx, int batch, hipStream_t s) {
  constexpr int TJ = 4, WP = padded_taps(H), NJ = TJ + 2 * H, TI = WAVE - 2 * H;
  const int tiles_i = (im->n + TI - 1) / TI;
  const FrGeom g{im->n, im->m, im->bn, im->bm, tiles_i};
  const dim3 grid((unsigned)((int64_t)tiles_i * ((im->m + TJ - 1) / TJ)), (unsigned)batch);
  const size_t lds = sizeof(float) * ((size_t)im->bm * NJ * WP + (size_t)TJ * WAVE);
  hipLaunchKernelGGL((k_framelet_adj<H, TJ>), grid, dim3(WAVE), lds, s, g, im->tn, im->sn, im->tm, im->sm, y, ldy, x, ldx);
}

template <int H>
void fr_launch_h(const FrImpl* im, int tr, const float* x, int64_t ldx, float* y, int64_t ldy, int batch, hipStream_t s) {
  if (tr) return fr_launch_adj<H>(im, x, ldx, y, ldy, batch, s);
  // forward: eight columns per lane; four while that leaves fewer than kSmallGridTiles tiles, eight waves for each of the 256 CUs (more,
  // smaller tiles: 512^2 is 512 tiles of 8).  A fixed number, not the device's CU count: which kernel a shape takes is the same
  // everywhere.
  const int64_t tiles8 = (int64_t)((im->n + WAVE - 1) / WAVE) * ((im->m + 7) / 8) * batch;
  if (tiles8 < kSmallGridTiles) fr_launch_fwd<H, 4>(im, x, ldx, y, ldy, batch, s);
  else fr_launch_fwd<H, 8>(im, x, ldx, y, ldy, batch, s);
}

int fr_apply(trk_op* op, int tr, const float* x, int64_t ldx, float* y, int64_t ldy, int batch, double* sumsq, hipStream_t s) {
  auto* im = static_cast<FrImpl*>(op->impl);
  TRK_REQUIRE(batch >= 1 && batch <= 65535, "framelet2d: batch must be 1 .. 65535");
  TimerScope tm(op->timer, op->timer_which, tr, s);
  switch (im->H) {
    case 1: fr_launch_h<1>(im, tr, x, ldx, y, ldy, batch, s); break;
    case 2: fr_launch_h<2>(im, tr, x, ldx, y, ldy, batch, s); break;
    case 4: fr_launch_h<4>(im, tr, x, ldx, y, ldy, batch, s); break;
    default: fr_launch_h<7>(im, tr, x, ldx, y, ldy, batch, s); break;
  }
  tm.stop();
  TRK_LAUNCH_CHECK();
  if (sumsq) {
    const int64_t nout = tr ? op->cols : op->rows;
    int64_t nb = (nout + 2047) / 2048, cap = kMaxPartialBlocks;
    if (nb > cap) nb = cap;
    double* part = nullptr;
    if (int rc = scratch_doubles(s, (size_t)nb * batch, &part)) return rc;
    hipLaunchKernelGGL(k_framelet_sumsq, dim3((unsigned)nb, (unsigned)batch), dim3(256), 0, s, y, ldy, nout, part);
    TRK_LAUNCH_CHECK();
    return finalize_sums(part, (int)nb * batch, 1, 1, sumsq, s);
  }
  return TRK_OK;
}

void fr_destroy(trk_op* op) {
  auto* im = static_cast<FrImpl*>(op->impl);
  if (im->tab) (void)hipFree(im->tab);
  delete im;
}

// One 1-D factor, checked on the host: every entry finite, 0 where its column lies outside [0, n), and the interior rows of each
// block (half <= i <= n - 1 - half) one stencil once rounded to float32 — the kernels take an interior tile's taps from that stencil.
int check_band(const char* which, int n, int blocks, int half, const double* band) {
  const int w = 2 * half + 1;
  for (int b = 0; b < blocks; ++b) {
    const double* first = nullptr;
    for (int i = 0; i < n; ++i) {
      const double* row = band + ((size_t)b * n + i) * w;
      for (int t = 0; t < w; ++t) {
        const int col = i - half + t;
        if (!std::isfinite(row[t])) return fail(TRK_EINVAL, "trk_framelet2d_create: band_%s[%d][%d][%d] is not finite", which, b, i, t);
        if ((col < 0 || col >= n) && row[t] != 0.0)
          return fail(TRK_EINVAL, "trk_framelet2d_create: band_%s[%d][%d][%d] lies outside the matrix (column %d) and is not 0", which, b, i, t, col);
      }
      if (i >= half && i <= n - 1 - half) {
        if (!first) first = row;
        for (int t = 0; t < w; ++t)
          if ((float)row[t] != (float)first[t])
            return fail(TRK_EINVAL, "trk_framelet2d_create: interior row %d of block %d of W_%s is not the block's stencil shifted (tap %d)",
                        i, b, which, t);
      }
    }
  }
  return TRK_OK;
}

}  // namespace

extern "C" int trk_framelet2d_create(int n, int m, int blocks_n, int half_n, const double* band_n, int blocks_m, int half_m,
                                     const double* band_m, trk_op** out) {
  TRK_REQUIRE(out && band_n && band_m, "trk_framelet2d_create: NULL argument");
  TRK_REQUIRE(n >= 1 && m >= 1 && blocks_n >= 1 && blocks_m >= 1 && half_n >= 0 && half_m >= 0, "trk_framelet2d_create: bad sizes");
  if (blocks_n > kMaxBlocks || blocks_m > kMaxBlocks)
    return fail(TRK_EUNSUPPORTED, "trk_framelet2d_create: %d and %d blocks; at most %d (the tile's taps along j are staged in LDS)", blocks_n, blocks_m, kMaxBlocks);
  TRK_REQUIRE((int64_t)blocks_n * n < ((int64_t)1 << 31) && (int64_t)blocks_m * m < ((int64_t)1 << 31),
              "trk_framelet2d_create: blocks * n and blocks * m must each be below 2^31");
  if (half_n > kMaxHalf || half_m > kMaxHalf)
    return fail(TRK_EUNSUPPORTED, "trk_framelet2d_create: half-widths %d, %d; the kernels are built for at most %d", half_n, half_m, kMaxHalf);
  if (int rc = check_band("n", n, blocks_n, half_n, band_n)) return rc;
  if (int rc = check_band("m", m, blocks_m, half_m, band_m)) return rc;
  const int hmax = half_n > half_m ? half_n : half_m;
  const int H = hmax <= 1 ? 1 : (hmax <= 2 ? 2 : (hmax <= 4 ? 4 : 7));
  const int W = 2 * H + 1;
  const size_t o_sn = (size_t)blocks_n * W * n, o_tm = o_sn + (size_t)blocks_n * W, o_sm = o_tm + (size_t)blocks_m * m * W;
  std::vector<float> tab(o_sm + (size_t)blocks_m * W, 0.f);
  for (int b = 0; b < blocks_n; ++b)
    for (int i = 0; i < n; ++i)
      for (int t = 0; t <= 2 * half_n; ++t) {
        const float v = (float)band_n[((size_t)b * n + i) * (2 * half_n + 1) + t];
        const int tp = t + H - half_n;
        tab[((size_t)b * W + tp) * n + i] = v;
        if (i == half_n && n > 2 * half_n) tab[o_sn + (size_t)b * W + tp] = v;
      }
  for (int c = 0; c < blocks_m; ++c)
    for (int j = 0; j < m; ++j)
      for (int t = 0; t <= 2 * half_m; ++t) {
        const float v = (float)band_m[((size_t)c * m + j) * (2 * half_m + 1) + t];
        const int tp = t + H - half_m;
        tab[o_tm + ((size_t)c * m + j) * W + tp] = v;
        if (j == half_m && m > 2 * half_m) tab[o_sm + (size_t)c * W + tp] = v;
      }
  auto* im = new FrImpl{n, m, blocks_n, blocks_m, H, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipError_t e = hipMalloc(&im->tab, tab.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(im->tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (im->tab) (void)hipFree(im->tab);
    delete im;
    return fail(TRK_EHIP, "trk_framelet2d_create: table upload: %s", hipGetErrorString(e));
  }
  im->tn = im->tab;
  im->sn = im->tab + o_sn;
  im->tm = im->tab + o_tm;
  im->sm = im->tab + o_sm;
  *out = new trk_op{8, (int64_t)blocks_n * n * blocks_m * m, (int64_t)n * m, im, fr_apply, fr_destroy, nullptr, 0};
  return TRK_OK;
}
