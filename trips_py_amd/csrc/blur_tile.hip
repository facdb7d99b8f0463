// blur_tile.hip — k_blur_tile: the blur of blur2d.hip (same correlation, same origin T = kh-1-kh/2, L = kw-1-kw/2, same boundary
// modes) for ANY PSF with 1 <= kh, kw <= 64 — even, rectangular, non-separable — from an LDS window.
//
// A workgroup of 256 threads owns a TILE_H x TILE_W = 32 x 64 tile of outputs.  The input window of the tile, (32+kh-1) x (64+kw-1)
// samples, is staged into LDS once through bmap<BC> (constant mode writes zeros): ALL boundary handling is in the staging, the
// accumulation has no index map and no branch on position.  A thread owns 8 consecutive outputs of one row; per PSF row it walks a
// sliding register window of 12 staged samples over the row, refilled four at a time by one 16-byte LDS read (row pitch 128 floats),
// 32 multiply-adds per read, so the vector unit and not LDS is the bound.  Weights are read through a const __restrict__ pointer at
// wave-uniform addresses: scalar loads, scalar registers.
//
//   general form   each output is ONE fp32 fmaf chain from 0.f, PSF rows ascending outside, columns ascending inside — k_blur_generic's
//                  order, so the two kernels give the same bits.  kh*kw multiply-adds per output.
//   separable form (rank-1 PSFs, im->separable)  the window is staged 32 rows at a time and row-filtered into a second LDS image of
//                  (32+kh-1) x 64, which is then column-filtered (a thread owns 2 x 4 outputs and reads each row of its columns once):
//                  kh+kw multiply-adds per output.
//
// LDS: general 95 x 128 floats = 48.6 KB (three workgroups per CU), separable 32 x 128 + 95 x 64 floats = 40.7 KB (three to four).
#include "blur_internal.h"

using namespace trk;

namespace {

constexpr int NT = 256;
constexpr int TILE_H = 32, TILE_W = 64;                  // outputs per workgroup (tests/blur_psf_cases.py mirrors these two)
constexpr int KMAX = kBlurTileMaxSide;
constexpr int PITCH = 128, PITCH4 = PITCH / 4;           // staged row: 64 + 63 window columns, rounded up; 2 x 256-byte bank rows
constexpr int WIN_H = TILE_H + KMAX - 1;                 // 95 window rows at most
constexpr int CHUNK = 32;                                // window rows staged at a time by the separable form
static_assert(TILE_W + KMAX - 1 <= PITCH, "the window fits the pitch");
static_assert(TILE_W == 8 * 8 && TILE_H * 8 == NT, "8 x 32 threads of 8 consecutive outputs");

// rows [r0, r0 + nrows) of the tile's window — window row r is image row i0 + r, window column c image column j0 + c, extended by
// mode BC — into S (pitch PITCH); columns from wcols on are zero.  Thread t writes column t % 128 of rows t / 128, t / 128 + 2, ...
template <int BC>
__device__ __forceinline__ void stage_rows(const float* __restrict__ x, int nx, int ny, int i0, int j0, int r0, int nrows, int wcols,
                                           float* S) {
  const int c = threadIdx.x & (PITCH - 1);
  const int gj = (c < wcols) ? bmap<BC>(j0 + c, ny) : -1;
  for (int r = threadIdx.x / PITCH; r < nrows; r += NT / PITCH) {
    float v = 0.f;
    if (gj >= 0) {
      const int gi = bmap<BC>(i0 + r0 + r, nx);
      if (BC != BC_CONSTANT || gi >= 0) v = x[(int64_t)gi * ny + gj];
    }
    S[r * PITCH + c] = v;
  }
}

// acc[c] = fmaf(w[b], row[c + b], acc[c]) for b = 0 .. kw-1 ascending, c = 0 .. 7: `p` points at the 16-byte group of row[0].
// Sliding window of three groups; a chunk of four taps uses groups t, t+1, t+2 and the oldest is then refilled with group t+3.
__device__ __forceinline__ void taps4(const f4& A, const f4& B, const f4& C, const float* __restrict__ w, int ntaps, float (&acc)[8]) {
  const float v[12] = {A[0], A[1], A[2], A[3], B[0], B[1], B[2], B[3], C[0], C[1], C[2], C[3]};
  // tap by tap: each output's chain takes its taps in ascending order
  {
    const float w0 = w[0];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = fmaf(w0, v[c], acc[c]);
  }
  if (ntaps > 1) {                                       // (wave-uniform)
    const float w1 = w[1];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = fmaf(w1, v[c + 1], acc[c]);
  }
  if (ntaps > 2) {
    const float w2 = w[2];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = fmaf(w2, v[c + 2], acc[c]);
  }
  if (ntaps > 3) {
    const float w3 = w[3];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = fmaf(w3, v[c + 3], acc[c]);
  }
}

__device__ __forceinline__ void full4(const f4& A, const f4& B, const f4& C, const float* __restrict__ w, float (&acc)[8]) {
  const float v[12] = {A[0], A[1], A[2], A[3], B[0], B[1], B[2], B[3], C[0], C[1], C[2], C[3]};
  const float w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = fmaf(w3, v[c + 3], fmaf(w2, v[c + 2], fmaf(w1, v[c + 1], fmaf(w0, v[c], acc[c]))));
}

__device__ __forceinline__ void row_taps(const f4* p, const float* __restrict__ w, int kw, float (&acc)[8]) {
  const int nfull = kw >> 2, tail = kw & 3;
  f4 A = p[0], B = p[1], C = p[2];                       // (groups beyond the last one a tap uses are read and not used: the image
  int t = 0;                                             //  has a slack group behind its last row)
  for (; t + 3 <= nfull; t += 3) {
    full4(A, B, C, w + 4 * t, acc);
    A = p[t + 3];
    full4(B, C, A, w + 4 * t + 4, acc);
    B = p[t + 4];
    full4(C, A, B, w + 4 * t + 8, acc);
    C = p[t + 5];
  }
  const int rem = nfull - t;                             // 0, 1 or 2 whole chunks, then the tail (wave-uniform branches)
  if (rem == 0) {
    if (tail) taps4(A, B, C, w + 4 * t, tail, acc);
  } else if (rem == 1) {
    full4(A, B, C, w + 4 * t, acc);
    if (tail) {
      A = p[t + 3];
      taps4(B, C, A, w + 4 * t + 4, tail, acc);
    }
  } else {
    full4(A, B, C, w + 4 * t, acc);
    A = p[t + 3];
    full4(B, C, A, w + 4 * t + 4, acc);
    if (tail) {
      B = p[t + 4];
      taps4(C, A, B, w + 4 * t + 8, tail, acc);
    }
  }
}

// ------------------------------------------------------------------------------------------------ general form
template <bool SUMSQ, int BC>
__global__ __launch_bounds__(NT, 3) void k_blur_tile(const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy,
                                                     int nx, int ny, int kh, int kw, const float* __restrict__ w,
                                                     double* __restrict__ partials, int tiles_x) {
  __shared__ f4 S4[WIN_H * PITCH4 + 4];                  // + the slack group row_taps may read behind the last row
  __shared__ double red[NT / 64];
  float* const S = reinterpret_cast<float*>(S4);
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int T = kh - 1 - kh / 2, L = kw - 1 - kw / 2;
  x += (int64_t)blockIdx.y * ldx;
  y += (int64_t)blockIdx.y * ldy;

  stage_rows<BC>(x, nx, ny, ti * TILE_H - T, tj * TILE_W - L, 0, TILE_H + kh - 1, TILE_W + kw - 1, S);
  __syncthreads();

  const int tx = threadIdx.x & 7, r = threadIdx.x >> 3;  // 8 outputs at columns 8 tx .. 8 tx + 7 of tile row r
  float acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = 0.f;
  const f4* p = S4 + r * PITCH4 + 2 * tx;
  for (int a = 0; a < kh; ++a) row_taps(p + a * PITCH4, w + a * kw, kw, acc);

  const int gi = ti * TILE_H + r, gj = tj * TILE_W + 8 * tx;
  double ss = 0.0;
  if (gi < nx) {
    float* out = y + (int64_t)gi * ny + gj;
    if (gj + 8 <= ny && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
      reinterpret_cast<f4*>(out)[0] = (f4){acc[0], acc[1], acc[2], acc[3]};
      reinterpret_cast<f4*>(out)[1] = (f4){acc[4], acc[5], acc[6], acc[7]};
      if (SUMSQ) {
#pragma unroll
        for (int c = 0; c < 8; ++c) ss += (double)acc[c] * acc[c];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (gj + c < ny) {
          out[c] = acc[c];
          if (SUMSQ) ss += (double)acc[c] * acc[c];
        }
    }
  }
  if (SUMSQ) {
    ss = block_sum<NT>(ss, red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ss;
  }
}

// ------------------------------------------------------------------------------------------------ separable form
// wts = [kw row weights | kh column weights] (sep_dev)
template <bool SUMSQ, int BC>
__global__ __launch_bounds__(NT, 3) void k_blur_tile_sep(const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy,
                                                         int nx, int ny, int kh, int kw, const float* __restrict__ wts,
                                                         double* __restrict__ partials, int tiles_x) {
  __shared__ f4 S4[CHUNK * PITCH4 + 4];                  // the window, CHUNK rows at a time
  __shared__ f4 H4[WIN_H * (TILE_W / 4)];                // the row-filtered window
  __shared__ double red[NT / 64];
  float* const S = reinterpret_cast<float*>(S4);
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int T = kh - 1 - kh / 2, L = kw - 1 - kw / 2;
  x += (int64_t)blockIdx.y * ldx;
  y += (int64_t)blockIdx.y * ldy;
  const int wrows = TILE_H + kh - 1;

  const int tx = threadIdx.x & 7, r = threadIdx.x >> 3;
  for (int r0 = 0; r0 < wrows; r0 += CHUNK) {
    const int nrows = (wrows - r0 < CHUNK) ? wrows - r0 : CHUNK;
    if (r0) __syncthreads();                             // every wave has filtered the chunk before
    stage_rows<BC>(x, nx, ny, ti * TILE_H - T, tj * TILE_W - L, r0, nrows, TILE_W + kw - 1, S);
    __syncthreads();
    if (r < nrows) {
      float h[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) h[c] = 0.f;
      row_taps(S4 + r * PITCH4 + 2 * tx, wts, kw, h);
      f4* hp = H4 + (r0 + r) * (TILE_W / 4) + 2 * tx;
      hp[0] = (f4){h[0], h[1], h[2], h[3]};
      hp[1] = (f4){h[4], h[5], h[6], h[7]};
    }
  }
  __syncthreads();

  // column filter: 2 rows x 4 columns per thread, every row of H read once per thread
  const float* __restrict__ wc = wts + kw;
  const int cx = threadIdx.x & 15, r2 = 2 * (threadIdx.x >> 4);
  const f4* hp = H4 + r2 * (TILE_W / 4) + cx;
  float wprev = wc[0];
  f4 hv = hp[0];
  f4 a0 = wprev * hv + (f4){0.f, 0.f, 0.f, 0.f}, a1 = (f4){0.f, 0.f, 0.f, 0.f};
  for (int s = 1; s < kh; ++s) {
    const float wcur = wc[s];
    hv = hp[s * (TILE_W / 4)];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a0[e] = fmaf(wcur, hv[e], a0[e]);
      a1[e] = fmaf(wprev, hv[e], a1[e]);
    }
    wprev = wcur;
  }
  hv = hp[kh * (TILE_W / 4)];
#pragma unroll
  for (int e = 0; e < 4; ++e) a1[e] = fmaf(wprev, hv[e], a1[e]);

  const int gj = tj * TILE_W + 4 * cx;
  double ss = 0.0;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int gi = ti * TILE_H + r2 + rr;
    const f4 o = rr ? a1 : a0;
    if (gi < nx) {
      float* out = y + (int64_t)gi * ny + gj;
      if (gj + 4 <= ny && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
        *reinterpret_cast<f4*>(out) = o;
        if (SUMSQ) ss += (double)o[0] * o[0] + (double)o[1] * o[1] + (double)o[2] * o[2] + (double)o[3] * o[3];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (gj + e < ny) {
            out[e] = o[e];
            if (SUMSQ) ss += (double)o[e] * o[e];
          }
      }
    }
  }
  if (SUMSQ) {
    ss = block_sum<NT>(ss, red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ss;
  }
}

}  // namespace

namespace trk {

int blur_tile_apply(trk_op* op, const BlurImpl* im, int tr, const float* x, int64_t ldx, float* y, int64_t ldy, int batch,
                    double* sumsq, hipStream_t s) {
  if (im->kh > KMAX || im->kw > KMAX) return fail(TRK_EUNSUPPORTED, "blur2d: the tile kernel takes PSFs up to %dx%d", KMAX, KMAX);
  const int tiles_x = ceil_div(im->ny, TILE_W), tiles_y = ceil_div(im->nx, TILE_H);
  const int64_t ntiles = (int64_t)tiles_x * tiles_y;
  if (ntiles > 0x7fffffff || batch > 65535) return fail(TRK_EUNSUPPORTED, "blur2d: image or batch too large for the tile kernel's grid");
  const int nblk = (int)ntiles;
  double* part = nullptr;
  if (sumsq)
    if (int rc = scratch_doubles(s, (size_t)nblk * batch, &part)) return rc;
  const dim3 grid(nblk, batch), block(NT);
  TimerScope tm(op->timer, op->timer_which, tr, s);
  bc_dispatch(im->bc, [&](auto bc) {
    constexpr int BC = decltype(bc)::value;
    with_bools([&](auto SS) {
      if (im->separable)
        hipLaunchKernelGGL((k_blur_tile_sep<decltype(SS)::value, BC>), grid, block, 0, s, x, ldx, y, ldy, im->nx, im->ny, im->kh,
                           im->kw, im->sep_dev[tr], part, tiles_x);
      else
        hipLaunchKernelGGL((k_blur_tile<decltype(SS)::value, BC>), grid, block, 0, s, x, ldx, y, ldy, im->nx, im->ny, im->kh, im->kw,
                           im->w_dev[tr], part, tiles_x);
    }, part != nullptr);
    return 0;
  });
  tm.stop();
  TRK_LAUNCH_CHECK();
  if (sumsq) return finalize_sums(part, nblk * batch, 1, 1, sumsq, s);
  return TRK_OK;
}

}  // namespace trk
