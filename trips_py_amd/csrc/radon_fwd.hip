// radon_fwd.hip — forward kernels of the parallel-beam projector (radon2d.hip: geometry, tables, the apply's bookkeeping) and their
// dispatch.  Mode-1 angles read a transposed copy of the image so that both modes read ROWS; the grid runs over bands of marching
// rows whose partial sums k_radon_bands_post adds up in a fixed order.
#include "radon_internal.h"

#include <cstdlib>
#include <type_traits>

using namespace trk;
using namespace trk::radon;

namespace {

// ---------------------------------------------------------------------------------------- transpose (LDS tile 32x33)
__global__ __launch_bounds__(256) void k_transpose(const float* __restrict__ in, float* __restrict__ out, int N) {
  __shared__ float tile[32][33];
  in += (int64_t)blockIdx.z * N * N;
  out += (int64_t)blockIdx.z * N * N;
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int i = by + r, j = bx + tx;
    if (i < N && j < N) tile[r][tx] = in[(int64_t)i * N + j];
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int i = bx + r, j = by + tx;  // out[i][j] = in[j][i]
    if (i < N && j < N) out[(int64_t)i * N + j] = tile[tx][r];
  }
}

// ---------------------------------------------------------------------------------------- forward

// One marching step of one ray with full edge handling (direct-gather paths): offset of the 8-byte load and the two tap
// weights in units of 2^-32 (taps outside the image, steps outside [.., te) and rays outside the detector weigh 0).
__device__ __forceinline__ int radon_edge_tap(int tt, int te, bool live, int N, float dq, float base, unsigned A,
                                              const unsigned* __restrict__ Brow, f2v& w) {
  const bool valid = live && tt < te;
  const int tr = tt < te ? tt : te - 1;
  const unsigned Q = A + Brow[tr];
  const int c = radon_abs_col(Q, fmaf((float)tr, dq, base));
  const float f1 = (float)(Q << 8), f0 = QTWO32 - f1;              // units of 2^-32, like the staged march
  // c == -1: only the right tap (column 0) is inside; start the 8-byte load at column 0 instead (an access that
  // STARTS below the buffer is dropped whole by the range check — measured on gfx950 — while one that runs off
  // the end returns its in-range dword)
  const bool neg1 = (c == -1);
  const int cl = neg1 ? 0 : c;
  const float w0 = neg1 ? f1 : (((unsigned)c < (unsigned)N) ? f0 : 0.f);
  const float w1 = neg1 ? 0.f : (((unsigned)(c + 1) < (unsigned)N) ? f1 : 0.f);
  w[0] = valid ? w0 : 0.f;
  w[1] = valid ? w1 : 0.f;
  const bool anyin = (unsigned)cl < (unsigned)N;
  return anyin ? (tr * N + cl) * 4 : 0x7FFFFFF0;                   // far outside: returns 0, fetches nothing
}

// Forward kernel (direct gathers; any N).  grid = (ceil(nd/64) * n_angle_groups, n_bands); block = 256 = 4 waves = 4
// CONSECUTIVE ANGLES of one frame x 64 detectors, marching the RADON_BAND image rows (mode 1: columns, through the transposed
// copy) of band blockIdx.y.  Why this shape (measured at 4096^2 x 180, MI355X): a wave marching the whole image touches 3-4
// new cache lines per step and never returns to them, and every angle sweeps the whole 67 MB image, so the first version
// (one wave = a quarter of the image) moved ~12 GB through the fabric per apply and was bound by L2 misses (2.15 ms;
// halving its VALU work changed nothing).  With row bands the grid runs band by band (blockIdx.x is the fast index),
// the 2 MB band stays in every XCD's 4 MB L2 while all angles and detectors pass over it, and the four waves of a
// workgroup - neighbouring angles, same detectors, same rows at the same time - share most of their L1 lines.
// Band partial sums go to a scratch array [band][angle][detector] that k_radon_bands_sum adds up in a fixed order.
#define RADON_CHUNK 32

template <bool FINAL>
__global__ __launch_bounds__(256) void k_radon_fwd(const float* __restrict__ img, const float* __restrict__ imgT,
                                                   float* __restrict__ out, int N, int nd,
                                                   const AngleParam* __restrict__ ang, int na_per_frame, int ngrp_per_frame,
                                                   int ndblk, int64_t band_stride, int bh,
                                                   const unsigned* __restrict__ A32, const unsigned* __restrict__ B32, int npad) {
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int grp = blockIdx.x / ndblk, dblk = blockIdx.x - grp * ndblk;
  const int frame = grp / ngrp_per_frame;
  const int af = (grp - frame * ngrp_per_frame) * 4 + wv;        // angle within the frame
  if (af >= na_per_frame) return;
  const int a = frame * na_per_frame + af;                         // global angle index (frame-major)
  const AngleParam p = ang[a];
  const float* __restrict__ I = (p.mode ? imgT : img) + (int64_t)frame * N * N;
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)I, 0, (unsigned)N * (unsigned)N * 4u, 0x00020000);
  const int d = dblk * 64 + lane;
  const bool live = d < nd;
  const unsigned A = A32[(int64_t)a * (nd + 2 * A32_PAD) + (live ? d : nd - 1) + A32_PAD];
  const unsigned* __restrict__ Brow = B32 + (int64_t)a * npad;
  const float s = (float)d - 0.5f * (float)(nd - 1);
  const float base = fmaf(s, p.inv, p.k0);
  const int t0 = blockIdx.y * bh, t1 = (t0 + bh < N) ? t0 + bh : N;
  const float qmax = (float)(N - 2);
  double total = 0.0;
  for (int tb = t0; tb < t1; tb += RADON_CHUNK) {
    const int te = (tb + RADON_CHUNK < t1) ? tb + RADON_CHUNK : t1;
    const float qa = fmaf((float)tb, p.dq, base), qb = fmaf((float)(te - 1), p.dq, base);
    // a chunk whose taps are inside the image for EVERY ray of the wave (q is monotone in tt; one column of margin for
    // the estimate) runs without any edge logic
    const bool inside = !live || (fminf(qa, qb) >= 1.f && fmaxf(qa, qb) < qmax);
    if (te - tb == RADON_CHUNK && __builtin_amdgcn_ballot_w64(inside) == ~0ull) {
      f2v acc2 = {0.f, 0.f};
      // two batches of 8 steps in flight: the loads of batch k+1 are issued before batch k is accumulated
      f2v w[2][8], v[2][8];
      auto issue = [&](int k) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int tt = tb + 8 * k + u;
          const unsigned Q = A + Brow[tt];
          const int c = radon_abs_col(Q, fmaf((float)tt, p.dq, base));
          w[k & 1][u][1] = (float)(Q << 8);
          w[k & 1][u][0] = QTWO32 - w[k & 1][u][1];
          v[k & 1][u] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(rsrc, c << 2, (unsigned)tt * (unsigned)N * 4u, 0));
        }
      };
      issue(0);
#pragma unroll
      for (int k = 0; k < RADON_CHUNK / 8; ++k) {
        if (k + 1 < RADON_CHUNK / 8) issue(k + 1);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc2 = __builtin_elementwise_fma(w[k & 1][u], v[k & 1][u], acc2);
      }
      total += (double)(acc2[0] + acc2[1]);
    } else {
      // edge chunk (or the short last one): same batching, weights carry the edge logic
      f2v acc2 = {0.f, 0.f};
#pragma unroll 1
      for (int k = 0; k < RADON_CHUNK / 8 && tb + 8 * k < te; ++k) {
        f2v w[8], v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int off = radon_edge_tap(tb + 8 * k + u, te, live, N, p.dq, base, A, Brow, w[u]);
          v[u] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 0));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc2 = __builtin_elementwise_fma(w[u], v[u], acc2);
      }
      total += (double)(acc2[0] + acc2[1]);
    }
  }
  if (live) {
    if (FINAL) out[(int64_t)a * nd + d] = p.wgt * (float)total;
    else out[(int64_t)blockIdx.y * band_stride + (int64_t)a * nd + d] = (float)total;
  }
}

// LDS-staged forward kernel (N % 4 == 0, 16-byte aligned images).  Same grid, same band partial sums, same arithmetic per
// tap as k_radon_fwd; what changes is how the taps reach the lanes.  Measured on k_radon_fwd: once the bands made the
// image L2-resident, the 8-byte per-lane gathers ran at ~3.6 lanes/clk/CU — the texture addresser's rate for scattered
// 64-bit loads — whatever the band height.  Here each wave stages the window of the image its 64 rays cross during a
// chunk of LDS_R = 16 rows — at most 64 sqrt(2) + 15 + 2 columns, rounded to 16-byte groups: LDS_W = 112 floats — with
// 7 coalesced 16-byte loads per lane (28 consecutive lanes read 448 contiguous bytes), and takes the two taps of a step
// with one ds_read2_b32 (the 32 lanes of a half-wave hit distinct banks: the rays' columns are strictly increasing and
// span < 64 floats).  Columns outside the image are staged as zeros (out-of-range buffer offsets), so the marching loop
// carries no edge logic at all.  The tile is private to its wave: no workgroup barrier, LDS operations of one wave
// execute in order.  The 7 loads go straight into LDS (buffer_load_dwordx4 ... lds — lane l of load i lands at float4 64 i + l
// of the tile, which is exactly the staging order; out-of-range lanes store zeros), which takes the texture-data -> register
// -> LDS detour out of the path.
// The march per step (7 vector instructions): Q = A' + B32[tt] (A' = the ray's table entry minus the window start, per chunk;
// B32[tt] through the scalar cache), column within the window = Q >> 24, weights (float)(Q & 0xFFFFFF) and 2^24 minus that,
// LDS address, one ds_read2_b32, one packed FMA.
#define LDS_R 16
#define LDS_W 112
#define LDS_WT 116    // row stride of a tile staged through the transposing path (direct1)

template <bool FINAL>
__global__ __launch_bounds__(256) void k_radon_fwd_lds(const float* __restrict__ img, const float* __restrict__ imgT,
                                                       float* __restrict__ out, int N, int nd,
                                                       const AngleParam* __restrict__ ang, int na_per_frame,
                                                       int ngrp_per_frame, int ndblk, int64_t band_stride, int bh,
                                                       const unsigned* __restrict__ A32, const unsigned* __restrict__ B32, int npad,
                                                       int direct1) {
  __shared__ __attribute__((aligned(16))) float tile[4][LDS_R * LDS_WT];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int grp = blockIdx.x / ndblk, dblk = blockIdx.x - grp * ndblk;
  const int frame = grp / ngrp_per_frame;
  const int af = (grp - frame * ngrp_per_frame) * 4 + wv;        // angle within the frame
  if (af >= na_per_frame) return;
  const int a = frame * na_per_frame + af;                         // global angle index (frame-major)
  const AngleParam p = ang[a];
  // direct1: angles marched along COLUMNS read the image itself and transpose while staging (no transposed copy, no launch
  // for it): the window is then 112 image rows x 16 columns, a lane's float4 is four marching steps of one row
  const bool tdir = direct1 && p.mode;                             // wave-uniform
  const float* __restrict__ I = ((p.mode && !tdir) ? imgT : img) + (int64_t)frame * N * N;
  const int rs4 = __builtin_amdgcn_readfirstlane((tdir ? LDS_WT : LDS_W) * 4);   // byte stride of a tile row
  const unsigned img_bytes = (unsigned)N * (unsigned)N * 4u;
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)I, 0, img_bytes, 0x00020000);
  float* __restrict__ T = tile[wv];
  const int d = dblk * 64 + lane;
  const float sdh = 0.5f * (float)(nd - 1);
  const float base = fmaf((float)d - sdh, p.inv, p.k0);
  const int nlive = (nd - dblk * 64 < 64) ? nd - dblk * 64 : 64;   // live lanes are 0 .. nlive-1 (wave-uniform)
  const bool live = lane < nlive;
  const unsigned A = A32[(int64_t)a * (nd + 2 * A32_PAD) + (live ? d : nd - 1) + A32_PAD];
  const unsigned* __restrict__ Ball = B32 + (int64_t)a * npad;
  float two32 = 4294967296.0f;                     // kept in an SGPR (opaque to the optimiser): no 32-bit literal per step
  asm("" : "+s"(two32));
  // base is monotone in the lane: the window's column range comes from the first and the last live ray
  const float b0 = fmaf((float)(dblk * 64) - sdh, p.inv, p.k0), b1 = fmaf((float)(dblk * 64 + nlive - 1) - sdh, p.inv, p.k0);
  const float blo = fminf(b0, b1), bhi = fmaxf(b0, b1);
  // staging slots of this lane: float4 number lane + 64 i of the 16 x 28 tile (row, 4-column group) — chunk-invariant
  int sc4[7], srowN4[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int idx = lane + 64 * i;
    const int row = idx / (LDS_W / 4);
    sc4[i] = (idx - row * (LDS_W / 4)) * 4;
    srowN4[i] = row * N * 4;
  }
  const int t0 = blockIdx.y * bh, t1 = (t0 + bh < N) ? t0 + bh : N;
  double total = 0.0;
  for (int tb = t0; tb < t1; tb += LDS_R) {
    const int te = (tb + LDS_R < t1) ? tb + LDS_R : t1;
    // column range of all taps of the chunk (q is monotone in tt as well): wave-uniform
    const float ta = (float)tb * p.dq, tz = (float)(te - 1) * p.dq;
    const float qlo = blo + fminf(ta, tz), qhi = bhi + fmaxf(ta, tz);
    // a chunk in which every tap of the wave lies outside the image (oblique views: the corners the detector overhangs) adds exact
    // zeros: skipped (two columns of margin for the fp32 estimate)
    if (__builtin_amdgcn_readfirstlane((qhi < -2.f || qlo > (float)N + 1.f) ? 1 : 0)) continue;
    // (readfirstlane: the values are wave-uniform but were computed in vector registers)
    const int cs = __builtin_amdgcn_readfirstlane(((int)floorf(qlo) - 1) & ~3);   // one column of slack for the fp32 estimate
    const bool fits = (__builtin_amdgcn_readfirstlane((int)floorf(qhi)) + 2 - cs) < LDS_W;
    const bool full = (te - tb == LDS_R);
    // 64-byte aligned (rows are padded to multiples of 32 entries, tb is a multiple of 16): one s_load_dwordx16 per chunk
    const unsigned* __restrict__ Brow = static_cast<const unsigned*>(__builtin_assume_aligned(Ball + tb, 64));
    f2v acc2 = {0.f, 0.f};
    if (fits) {
      // stage: rows tb .. tb+15 (beyond te: not fetched), columns cs .. cs+111 (outside the image: zeros); the row part of the
      // address is the wave-uniform soffset, the lane part is chunk-invariant but for the window start cs
      f4r v[7];
      const unsigned rowbase = (unsigned)tb * (unsigned)N * 4u;
      if (tdir) {
        // slot idx = lane + 64 i: window coordinate cw = idx / 4 (an image ROW cs + cw), marching steps 4 q .. 4 q + 3, q = idx % 4
        // (image COLUMNS tb + 4 q ..: inside the row because N % 4 == 0); element e goes to tile row 4 q + e, column cw.  The
        // transposed tile has row stride LDS_WT = 116: the four q of a row then fall into different banks
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          const int idx = lane + 64 * i;
          const int cw = idx >> 2, q = idx & 3;
          const int row = cs + cw;
          const bool ok = (unsigned)row < (unsigned)N && tb + 4 * q < N;
          const int voff = ok ? (row * N + tb + 4 * q) * 4 : (int)img_bytes;
          v[i] = __builtin_bit_cast(f4r, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          const int idx = lane + 64 * i;
          const int cw = idx >> 2, q = idx & 3;
#pragma unroll
          for (int e = 0; e < 4; ++e) T[(4 * q + e) * LDS_WT + cw] = v[i][e];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          const int col = cs + sc4[i];
          bool ok = (unsigned)col < (unsigned)N;
          if (!full) ok = ok && (tb + (lane + 64 * i) / (LDS_W / 4) < te);
          const int voff = ok ? (col << 2) + srowN4[i] : (int)img_bytes;          // out of range: returns 0, fetches nothing
          // straight into LDS (buffer_load_dwordx4 ... lds: lane l of load i lands at float4 64 i + l of the tile)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(T + 256 * i), 16, voff, rowbase, 0, 0);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);                        // vmcnt(0): the tile is in LDS
      }
      __builtin_amdgcn_wave_barrier();
      const unsigned Ac = A - ((unsigned)cs << QF);               // column relative to the window (mod 256)
      auto march = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;         // FULL: 16 rows, all 64 rays live — no guards at all
        f2v w[LDS_R], t2[LDS_R];
#pragma unroll
        for (int u = 0; u < LDS_R; ++u) {
          const unsigned Q = Ac + Brow[u];                       // Brow is padded: rows beyond te read valid table entries
          const float f1 = (float)(Q << 8);                      // the 24 fraction bits, in units of 2^-32 (exact: 24 significant bits)
          w[u][1] = (FULL || tb + u < te) ? f1 : 0.f;
          w[u][0] = (FULL || tb + u < te) ? two32 - f1 : 0.f;
          unsigned c = Q >> QF;
          if (!FULL) c = c > (unsigned)(LDS_W - 2) ? (unsigned)(LDS_W - 2) : c;   // dead lanes / rows beyond te may point anywhere
          // byte address = row base [scalar, opaque to the optimiser so that it stays a scalar add and is not turned into a
          // per-lane one] + 4 c [one v_lshl_add]; both taps with one ds_read2_b32
          int rowoff4 = u * rs4;
          asm("" : "+s"(rowoff4));
          const float* tp = reinterpret_cast<const float*>(reinterpret_cast<const char*>(T) + rowoff4 + (c << 2));
          t2[u] = (f2v){tp[0], tp[1]};
        }
#pragma unroll
        for (int u = 0; u < LDS_R; ++u) acc2 = __builtin_elementwise_fma(w[u], t2[u], acc2);
      };
      if (full && nlive == 64) march(std::true_type{});
      else march(std::false_type{});
      __builtin_amdgcn_wave_barrier();
    } else {
      // cannot happen for 64 rays and 16 rows unless the float sums above round unfavourably: direct gathers
#pragma unroll 1
      for (int k = 0; k < LDS_R / 8 && tb + 8 * k < te; ++k) {
        f2v w[8], v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int off = radon_edge_tap(tb + 8 * k + u, te, live, N, p.dq, base, A, Ball, w[u]);
          v[u] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 0));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc2 = __builtin_elementwise_fma(w[u], v[u], acc2);
      }
    }
    total += (double)(acc2[0] + acc2[1]);
  }
  if (live) {
    if (FINAL) out[(int64_t)a * nd + d] = p.wgt * (float)total;
    else out[(int64_t)blockIdx.y * band_stride + (int64_t)a * nd + d] = (float)total;
  }
}

// Quad forward kernel (round 4): FOUR symmetric angles from one set of taps, conflict-free LDS gathers.
//
// What bounds the seven-instruction march of k_radon_fwd_lds once windows are shared — vector issue at 25-30 cycles per wave and
// step, two-way bank conflicts of its ds_read2_b32 — is worked out in docs/kernels/radon.md 4.4c (tools/microbench/issue_rate.hip).
// Two changes take each pipe off the critical path:
//   * SYMMETRY.  With beta in [0, 45 deg], ct = cos(beta), t = tan(beta), q_b(s, i) = s/ct + h(1 - t) + i t  (h = (N-1)/2):
//       angle beta        rows of x,   q = q_b(s, i)                      slot 0
//       angle 180 - beta  rows of x,   q = (N-1) - q_b(s, i)              slot 1  (mirrored columns: taps swap their weights)
//       angle 90 - beta   rows of xT,  q = q_b(-s, j)                     slot 2  (detector index flipped)
//       angle 90 + beta   rows of xT,  q = (N-1) - q_b(s, j)              slot 3
//     (all four identities exact; checked against the oracle to 1e-15; the general sign cases are in radon_create_impl).  A wave
//     computes Q, both weights and the LDS address ONCE per step and uses them for the four members: the window [cs, cs + W) of
//     x and of xT (region F) and the mirrored window [N - cs - W, N - cs) of both (region M, stored in descending order so that its
//     address is one constant minus the forward address).  7 shared instructions + 1 (mirror address) + 4 packed FMAs per
//     256 ray-steps instead of 28: the vector unit drops to ~40 % and the march is bound by its four ds_read2_b32.
//   * HALF-WAVE WINDOWS.  A 32-lane group (what one LDS cycle serves for ds_read_b32) owns the rays whose column at the band's top
//     row lies in a 31-column interval: at any row its <= 32 columns are distinct mod 32 — no bank conflicts by construction
//     (lanes without a ray repeat an owned address: broadcast), at 31 / (32 inv) of the lanes busy.  Measured in isolation:
//     17.7 cycles per 256 ray-steps and CU against 36.7 for the march above.
// The member tables A32 / B32 / CB of every angle are DERIVED from its quad's base tables at create time, so the adjoint (which
// reads the members' tables) still sees bit-identical weights.  Angles without partners run as quads with fewer members.
// Workgroup = 4 waves = 4 quads of neighbouring beta sharing the staged tiles; chunks of QD_R = 8 rows, double-buffered with a true
// prefetch (the taps are inline-assembly LDS reads, so the compiler does not drain the direct-to-LDS loads in front of them).
// QD_R = 8 rows per chunk, at most QD_MAXCH = 32 chunks per band (radon_internal.h)
#define QD_W 120                          // window width (floats): 62 owned columns + 8 rows of slope + the drift of 4 neighbouring quads + alignment
#define QD_HALF 31
#define QD_WO (2 * QD_HALF)
// LDS layout of a region (F: windows as they are; M: mirrored windows): [row pair p][source: x, xT][row in pair][QD_W] floats.
//   * one wave-load (60 lanes x 16 bytes = 240 floats) fills the two rows of ONE source: full-width loads with one buffer
//     resource (half-masked loads per source cost the texture path twice as much per byte: measured, TD 87 % busy);
//   * the xT window sits QD_SRC = 240 floats behind the x window: inside the 8-bit offsets of ds_read2_b32, so ONE address register
//     serves both sources;
//   * region M stores pairs, rows and columns in DESCENDING order: address_M(u, 118 - k) = constant - address_F(u, k).
#define QD_SRC (2 * QD_W)                 // 240
#define QD_PAIR (2 * QD_SRC)              // 480
#define QD_REGION ((QD_R / 2) * QD_PAIR)  // 1920 floats
// tiles in flight per workgroup: two (measured: deeper staging does not pay at any size — the extra LDS costs resident workgroups,
// 512^2: 40 -> 60 us with four tiles in flight, 4096^2: 0.76 -> 1.34 ms)
constexpr int QD_TILES = 2;

__device__ __forceinline__ unsigned lds_off(const void* p) { return (unsigned)(size_t)(__attribute__((address_space(3))) const void*)p; }

__global__ __launch_bounds__(256, 4) void k_radon_fwd_quad(const float* __restrict__ img, const float* __restrict__ imgT,
                                                        float* __restrict__ out, int N, int nd,
                                                        const QuadParam* __restrict__ quads, int nq_per_frame, int ngrp_per_frame,
                                                        int na_per_frame, int nwin, int64_t band_stride, int bh,
                                                        const float* __restrict__ fidx, const unsigned* __restrict__ A32q,
                                                        const unsigned* __restrict__ B32q, int npad,
                                                        const AngleParam* __restrict__ ang, const unsigned* __restrict__ A32,
                                                        const unsigned* __restrict__ B32, const int* __restrict__ wg_list, int grid_x) {
  __shared__ __attribute__((aligned(16))) float tile[QD_TILES][2 * QD_REGION];
  __shared__ float ext[4][QD_MAXCH][2];
  __shared__ int chinfo[QD_MAXCH][2];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  // wg_list (round 6): this launch runs only the workgroups of the full grid that k_radon_fwd_quadf leaves to it
  const int wg_id = wg_list ? wg_list[1 + blockIdx.x] : 0;
  const int blk_y = wg_list ? wg_id / grid_x : (int)blockIdx.y, blk_x = wg_list ? wg_id - blk_y * grid_x : (int)blockIdx.x;
  // workgroups b and b + 8 run on the same XCD (round-robin placement: speed only, never correctness): give every XCD one
  // contiguous eighth of the windows, for all quad groups — its L2 then holds an eighth of the band (and the mirrored eighth)
  // instead of every fourth window of all of it
  const int nw8 = (nwin + 7) >> 3;
  const int xcd = blk_x & 7, bidx = blk_x >> 3;
  const int grp = bidx / nw8, jj = xcd * nw8 + (bidx - grp * nw8);
  if (jj >= nwin) return;
  const int frame = grp / ngrp_per_frame;
  const int q0 = (grp - frame * ngrp_per_frame) * 4;
  const int nval = (nq_per_frame - q0 < 4) ? nq_per_frame - q0 : 4;
  const QuadParam* __restrict__ qg = quads + (int64_t)frame * nq_per_frame + q0;
  int smask = 0;                                                    // slots any of the workgroup's quads uses: what gets staged
  for (int w = 0; w < nval; ++w) smask |= qg[w].mask;
  const int t0 = blk_y * bh, t1 = (t0 + bh < N) ? t0 + bh : N;
  const int OFFS = bh + 4;
  const bool valid = wv < nval;
  const QuadParam p = qg[valid ? wv : 0];
  const int qrow = frame * nq_per_frame + q0 + (valid ? wv : 0);
  const int ndp = nd + 2 * A32_PAD;
  const unsigned img_bytes = (unsigned)N * (unsigned)N * 4u;
  const auto rsrc0 = __builtin_amdgcn_make_buffer_rsrc((void*)(img + (int64_t)frame * N * N), 0, img_bytes, 0x00020000);
  const auto rsrc1 = __builtin_amdgcn_make_buffer_rsrc((void*)((imgT ? imgT : img) + (int64_t)frame * N * N), 0, img_bytes, 0x00020000);
  const float sdh = 0.5f * (float)(nd - 1);
  // a half-wave owns the rays whose column at the band's top row lies in [qa, qb), 31 columns: its candidates are the 32
  // detectors from the first one inside (found exactly: the estimate of the interval's pre-image is good to a small fraction of a
  // detector, one test decides between its two possible values)
  const int hw = lane >> 5, li = lane & 31;
  const float qa = (float)(jj * QD_WO - OFFS + QD_HALF * hw), qb = qa + (float)QD_HALF;
  const float t0f = fidx[t0];
  const float offs = fmaf(t0f, p.dq, p.k0);
  const float dA = (qa - offs) * p.rinv + sdh;
  const int d0 = (int)ceilf(dA - 0.05f);
  const float qt0 = fmaf(t0f, p.dq, fmaf((float)d0 - sdh, p.inv, p.k0));
  const int d = d0 + (qt0 < qa ? 1 : 0) + li;
  const float base = fmaf((float)d - sdh, p.inv, p.k0);
  const float qtop = fmaf(t0f, p.dq, base);
  const bool owned = valid && p.mask != 0 && (unsigned)d < (unsigned)nd && qtop >= qa && qtop < qb;
  const unsigned long long omask = __builtin_amdgcn_ballot_w64(owned);
  const bool any = omask != 0ull;
  const unsigned om_lo = (unsigned)omask, om_hi = (unsigned)(omask >> 32);
  const int l_first = any ? __builtin_ctzll(omask) : 0, l_last = any ? 63 - __builtin_clzll(omask) : 0;
  const float blo = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, base), l_first));   // inv > 0: increasing
  const float bhi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, base), l_last));
  const int dcl = d < 0 ? 0 : (d >= nd ? nd - 1 : d);
  const unsigned A = A32q[(int64_t)qrow * ndp + dcl + A32_PAD];
  // lanes without a ray follow the first owned ray of their half (of the other half if theirs owns none): a broadcast, inside the tile
  const int lf0 = om_lo ? __builtin_ctz(om_lo) : (om_hi ? 32 + __builtin_ctz(om_hi) : 0);
  const int lf1 = om_hi ? 32 + __builtin_ctz(om_hi) : lf0;
  const unsigned A_f0 = (unsigned)__builtin_amdgcn_readlane((int)A, lf0), A_f1 = (unsigned)__builtin_amdgcn_readlane((int)A, lf1);
  const unsigned A_m = owned ? A : (hw ? A_f1 : A_f0);
  const unsigned* __restrict__ Ball = B32q + (int64_t)qrow * npad;
  float two32v = 4294967296.0f;                    // in a VECTOR register: an SGPR operand would make the subtraction a 4-cycle issue
  asm volatile("" : "+v"(two32v));
  double total[4] = {0.0, 0.0, 0.0, 0.0};

  // column range of every chunk, per wave -> LDS -> the union over the four waves, once per band (dq >= 0: q grows with the row)
  const int nch = (t1 - t0 + QD_R - 1) / QD_R;
  if (lane < nch) {
    const int tb = t0 + lane * QD_R, te = (tb + QD_R < t1) ? tb + QD_R : t1;
    ext[wv][lane][0] = any ? blo + (float)tb * p.dq : 3.0e38f;
    ext[wv][lane][1] = any ? bhi + (float)(te - 1) * p.dq : -3.0e38f;
  }
  __syncthreads();
  if (wv == 0 && lane < nch) {
    const float ulo = fminf(fminf(ext[0][lane][0], ext[1][lane][0]), fminf(ext[2][lane][0], ext[3][lane][0]));
    const float uhi = fmaxf(fmaxf(ext[0][lane][1], ext[1][lane][1]), fmaxf(ext[2][lane][1], ext[3][lane][1]));
    const bool nobody = ulo > uhi;
    const int cs = nobody ? 0 : (((int)floorf(ulo) - 1) & ~3);
    const bool fits = !nobody && ((int)floorf(nobody ? 0.f : uhi) + 2 - cs) < QD_W;
    chinfo[lane][0] = cs;
    chinfo[lane][1] = nobody ? 2 : (fits ? 1 : 0);                // 2: no wave owns a ray here — nothing to stage, nothing to march
  }
  __syncthreads();

  // staging: wave wv fills row pair wv of region F and of region M, one load per source (lanes 0-59: row in pair = lane / 30,
  // four columns from 4 (lane % 30)).  Rows beyond te and columns outside the image arrive as zeros (offset out of range).
  const int sr = lane >= 30 ? 1 : 0, sk = (lane - 30 * sr) << 2;                   // chunk-invariant
  const int rowF = (2 * wv + sr) * N * 4, rowM = (2 * (QD_R / 2 - 1 - wv) + 1 - sr) * N * 4;
  const int uF = 2 * wv + sr, uM = 2 * (QD_R / 2 - 1 - wv) + 1 - sr;
  auto stage = [&](int ch, int cs) {
    const int tb = t0 + ch * QD_R, te = (tb + QD_R < t1) ? tb + QD_R : t1;
    float* __restrict__ T = tile[ch % QD_TILES];
    const unsigned rowbase = (unsigned)tb * (unsigned)N * 4u;
    const int colF = cs + sk, colM = (N - cs - QD_W) + sk;
    const bool okF = ((unsigned)colF < (unsigned)N) && (tb + uF < te), okM = ((unsigned)colM < (unsigned)N) && (tb + uM < te);
    const int voffF = okF ? (colF << 2) + rowF : (int)img_bytes, voffM = okM ? (colM << 2) + rowM : (int)img_bytes;
    auto* dF = (__attribute__((address_space(3))) void*)(T + wv * QD_PAIR);
    auto* dFt = (__attribute__((address_space(3))) void*)(T + wv * QD_PAIR + QD_SRC);
    auto* dM = (__attribute__((address_space(3))) void*)(T + QD_REGION + wv * QD_PAIR);
    auto* dMt = (__attribute__((address_space(3))) void*)(T + QD_REGION + wv * QD_PAIR + QD_SRC);
    if (lane < 60) {
      if (smask & 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc0, dF, 16, voffF, rowbase, 0, 0);
      if (smask & 4) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc1, dFt, 16, voffF, rowbase, 0, 0);
      if (smask & 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc0, dM, 16, voffM, rowbase, 0, 0);
      if (smask & 8) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc1, dMt, 16, voffM, rowbase, 0, 0);
    }
  };

  f2v acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
  // Every chunk's window in a register (lane ch holds chunk ch): inside the loop nothing the COMPILER sees touches LDS, so it has no
  // reason to drain the direct-to-LDS loads (it orders every LDS access it knows of behind all of them), and chunks can be
  // staged QD_TILES - 1 ahead.  A workgroup's chunks form a dependent chain — barrier, wait for a tile, march 8 rows — and at small
  // images (few workgroups per CU) the chain is bound by the latency of ONE staging round trip per chunk (512^2: 16 chunks x
  // 1.7 us); with three chunks in flight the round trips overlap.
  const int cs_all = lane < nch ? chinfo[lane][0] : 0, st_all = lane < nch ? chinfo[lane][1] : 2;
  const int per_stage = __builtin_popcount(smask & 15);          // wave-level load instructions one staged chunk issues
  auto st_of = [&](int c) { return c < nch ? __builtin_amdgcn_readlane(st_all, c) : 2; };
  auto cs_of = [&](int c) { return c < nch ? __builtin_amdgcn_readlane(cs_all, c) : 0; };
  auto wait_loads = [&](int later) {                             // until at most `later` of this wave's loads are outstanding
    switch (later) {
      case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
      case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
      case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
      case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
      case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
      case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
      case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
  };
#pragma unroll
  for (int c = 0; c < QD_TILES - 1; ++c)
    if (st_of(c) == 1) stage(c, cs_of(c));
  for (int ch = 0; ch < nch; ++ch) {
    const int tb = t0 + ch * QD_R, te = (tb + QD_R < t1) ? tb + QD_R : t1;
    const float* __restrict__ T = tile[ch % QD_TILES];
    const int cs = cs_of(ch), st = st_of(ch);
    // The chunk's eight B32 entries in ONE scalar load, requested BEFORE the barrier (round 6).  Fetched one by one inside the march
    // (as rounds 4-5 had it: `Ac + Brow[u]` next to the reads) every entry came with `s_waitcnt lgkmcnt(0)` — scalar loads return
    // out of order, so a wait for one is a wait for everything counted in lgkmcnt, the LDS reads included: every step drained the
    // three steps of reads "in flight", and the waves issued 38 % of their resident time (profiles/r05/radon_4096_pmc.txt).
    typedef unsigned u8v __attribute__((ext_vector_type(8)));
    const u8v Bv = *reinterpret_cast<const u8v*>(__builtin_assume_aligned(Ball + tb, 32));
    // this wave's loads of chunk ch have landed (those of the chunks staged after it may still fly), then the workgroup meets:
    // chunk ch is complete in LDS and everybody has left the buffer chunk ch + QD_TILES - 1 goes into
    int later = 0;
#pragma unroll
    for (int c = 1; c < QD_TILES - 1; ++c) later += (st_of(ch + c) == 1) ? per_stage : 0;
    wait_loads(later);
    asm volatile("s_barrier" ::: "memory");
    if (st_of(ch + QD_TILES - 1) == 1) stage(ch + QD_TILES - 1, cs_of(ch + QD_TILES - 1));
    const bool full = (te - tb == QD_R);
    if (st == 1 && any) {
      const unsigned Ac = A_m - ((unsigned)cs << QF);
      const unsigned Toff = lds_off(T);
      unsigned Cm = 2u * Toff + 4u * (unsigned)(QD_REGION + (QD_R / 2 - 1) * QD_PAIR + QD_W + (QD_W - 2));
      asm volatile("" : "+v"(Cm));
      auto march = [&](auto full_tag, auto all_tag) {
        constexpr bool FULL = decltype(full_tag)::value, ALL = decltype(all_tag)::value;
        f2v w[QD_R];
        unsigned a0[QD_R], a1[QD_R];
        // weights and addresses of a step are made three steps ahead of their use, just before its reads are issued: the vector
        // work of step u + 3 runs while the reads of steps u .. u + 2 are in flight, and few of these registers are live at once
        auto prep = [&](int u) {
          const unsigned Q = Ac + Bv[u];
          float f1 = (float)(Q << 8);                             // the 24 fraction bits, in units of 2^-32 (exact)
          float f0 = two32v - f1;
          if (!FULL) {
            f1 = (tb + u < te) ? f1 : 0.f;
            f0 = (tb + u < te) ? f0 : 0.f;
          }
          w[u] = (f2v){f0, f1};
          unsigned c = Q >> QF;
          if (!FULL) c = c > (unsigned)(QD_W - 2) ? (unsigned)(QD_W - 2) : c;
          int rowoff = (int)Toff + ((u >> 1) * QD_PAIR + (u & 1) * QD_W) * 4;   // a scalar add (opaque to the optimiser, or it becomes a second vector add)
          asm("" : "+s"(rowoff));
          a0[u] = (c << 2) + (unsigned)rowoff;
          a1[u] = Cm - a0[u];
        };
        // three steps (12 reads) in flight; LDS returns in order, so "at most 8 outstanding" means step u has arrived
        f2v tA[QD_R], tB[QD_R], tC[QD_R], tD[QD_R];
        auto issue = [&](int u) {
          asm volatile("ds_read2_b32 %0, %1 offset1:1" : "=v"(tA[u]) : "v"(a0[u]));
          asm volatile("ds_read2_b32 %0, %1 offset0:240 offset1:241" : "=v"(tB[u]) : "v"(a0[u]));
          asm volatile("ds_read2_b32 %0, %1 offset1:1" : "=v"(tC[u]) : "v"(a1[u]));
          asm volatile("ds_read2_b32 %0, %1 offset0:240 offset1:241" : "=v"(tD[u]) : "v"(a1[u]));
          static_assert(QD_SRC == 240, "the offsets above are QD_SRC and QD_SRC + 1");
        };
        prep(0);
        issue(0);
        prep(1);
        issue(1);
        prep(2);
        issue(2);
#pragma unroll
        for (int u = 0; u < QD_R; ++u) {
          if (u + 3 < QD_R) prep(u + 3);
          if (u <= QD_R - 3) asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
          else if (u == QD_R - 2) asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
          else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          asm volatile("" : "+v"(tA[u]), "+v"(tB[u]), "+v"(tC[u]), "+v"(tD[u]));
          if (u + 3 < QD_R) issue(u + 3);
          if (ALL || (p.mask & 1)) acc[0] = __builtin_elementwise_fma(w[u], tA[u], acc[0]);
          if (ALL || (p.mask & 4)) acc[2] = __builtin_elementwise_fma(w[u], tB[u], acc[2]);
          // mirrored windows: the pair read at the mirrored address is (tap c+1, tap c): the weights swap halves
          if (ALL || (p.mask & 2)) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[0,1,1]" : "+v"(acc[1]) : "v"(w[u]), "v"(tC[u]));
          if (ALL || (p.mask & 8)) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[0,1,1]" : "+v"(acc[3]) : "v"(w[u]), "v"(tD[u]));
        }
      };
      if (p.mask == 15) {
        if (full) march(std::true_type{}, std::true_type{});
        else march(std::false_type{}, std::true_type{});
      } else {
        if (full) march(std::true_type{}, std::false_type{});
        else march(std::false_type{}, std::false_type{});
      }
    } else if (st == 0 && any) {
      // the four quads are too far apart for one window: every member gathers for itself from its own image and tables
#pragma unroll 1
      for (int m = 0; m < 4; ++m) {
        if (!((p.mask >> m) & 1)) continue;
        const int am_m = m == 0 ? p.am[0] : (m == 1 ? p.am[1] : (m == 2 ? p.am[2] : p.am[3]));   // (no dynamic index into p: it would move to scratch)
        const int a = frame * na_per_frame + am_m;
        const AngleParam pm = ang[a];
        const int dm = ((p.flip >> m) & 1) ? nd - 1 - d : d;
        const int dmc = dm < 0 ? 0 : (dm >= nd ? nd - 1 : dm);
        const float base_m = fmaf((float)dm - sdh, pm.inv, pm.k0);
        const unsigned Amm = A32[(int64_t)a * ndp + dmc + A32_PAD];
        const unsigned* __restrict__ Bm = B32 + (int64_t)a * npad;
        f2v w[8], v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int off = radon_edge_tap(tb + u, te, owned, N, pm.dq, base_m, Amm, Bm, w[u]);
          v[u] = __builtin_bit_cast(f2v, pm.mode ? __builtin_amdgcn_raw_buffer_load_b64(rsrc1, off, 0, 0)
                                                 : __builtin_amdgcn_raw_buffer_load_b64(rsrc0, off, 0, 0));
        }
        f2v am2 = {0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 8; ++u) am2 = __builtin_elementwise_fma(w[u], v[u], am2);
        const double tm = (double)(am2[0] + am2[1]);
        total[0] += m == 0 ? tm : 0.0;
        total[1] += m == 1 ? tm : 0.0;
        total[2] += m == 2 ? tm : 0.0;
        total[3] += m == 3 ? tm : 0.0;
      }
    }
    if ((ch & 1) || ch == nch - 1) {                               // fp32 partial sums over 16 rows, then fp64 (as the other forward kernels)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        total[m] += (double)(acc[m][0] + acc[m][1]);
        acc[m] = (f2v){0.f, 0.f};
      }
    }
  }
  if (owned) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      if (!((p.mask >> m) & 1)) continue;
      const int dm = ((p.flip >> m) & 1) ? nd - 1 - d : d;
      out[(int64_t)blk_y * band_stride + ((int64_t)frame * na_per_frame + p.am[m]) * nd + dm] = (float)total[m];
    }
  }
}

// ---------------------------------------------------------------------------------------- forward, quads: plan + lean kernel (round 6)
// Counters of k_radon_fwd_quad at 4096^2 x 180 (profiles/r05/radon_4096_pmc.txt, r06): 241 M vector instructions of which the march
// itself is 134 M; 150 M scalar; the vector unit 68 % busy and the waves stalled at issue — the kernel is bound by its instruction
// count, and 44 % of it is bookkeeping that depends on the GEOMETRY only: which detector a lane owns, the column range of every chunk
// (two barriers and an LDS round per workgroup), whether a window fits, the clamps of partial chunks, four march variants, and
// scalar registers spilled to vector lanes by all of it.  k_radon_quad_plan works that out ONCE per operator, per workgroup of the grid
// (the same arithmetic, statement for statement, as k_radon_fwd_quad's prologue: the two kernels own the same rays), and
// k_radon_fwd_quadf is the march alone: whole chunks of eight rows, all four members, one window start per chunk from the plan.
// Workgroups it cannot serve (a window that does not fit, a ragged band, groups of mostly single angles) are LISTED by the plan and
// run by k_radon_fwd_quad as before; both write the same band partials, the same bits.
constexpr int QD_NONE = INT32_MIN;
__global__ __launch_bounds__(256) void k_radon_quad_plan(int N, int nd, const QuadParam* __restrict__ quads, int nq_per_frame,
                                                         int ngrp_per_frame, int nwin, int bh, const float* __restrict__ fidx,
                                                         int have_xT, QuadPlan* __restrict__ plan, int* __restrict__ slow) {
  __shared__ float ext[4][QD_MAXCH][2];
  __shared__ int nfit;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  QuadPlan& P = plan[(int64_t)blockIdx.y * gridDim.x + blockIdx.x];
  const int nw8 = (nwin + 7) >> 3;
  const int xcd = blockIdx.x & 7, bidx = blockIdx.x >> 3;
  const int grp = bidx / nw8, jj = xcd * nw8 + (bidx - grp * nw8);
  if (jj >= nwin) {
    if (threadIdx.x == 0) P.fast = 2;
    return;
  }
  const int frame = grp / ngrp_per_frame;
  const int q0 = (grp - frame * ngrp_per_frame) * 4;
  const int nval = (nq_per_frame - q0 < 4) ? nq_per_frame - q0 : 4;
  const QuadParam* __restrict__ qg = quads + (int64_t)frame * nq_per_frame + q0;
  int members = 0;
  for (int w = 0; w < nval; ++w) members += __builtin_popcount(qg[w].mask & 15);
  const int t0 = blockIdx.y * bh, t1 = (t0 + bh < N) ? t0 + bh : N;
  const int OFFS = bh + 4;
  const bool valid = wv < nval;
  const QuadParam p = qg[valid ? wv : 0];
  const float sdh = 0.5f * (float)(nd - 1);
  // ---- k_radon_fwd_quad's ownership, statement for statement
  const int hw = lane >> 5, li = lane & 31;
  const float qa = (float)(jj * QD_WO - OFFS + QD_HALF * hw), qb = qa + (float)QD_HALF;
  const float t0f = fidx[t0];
  const float offs = fmaf(t0f, p.dq, p.k0);
  const float dA = (qa - offs) * p.rinv + sdh;
  const int d0 = (int)ceilf(dA - 0.05f);
  const float qt0 = fmaf(t0f, p.dq, fmaf((float)d0 - sdh, p.inv, p.k0));
  const int dl0 = d0 + (qt0 < qa ? 1 : 0);
  const int d = dl0 + li;
  const float base = fmaf((float)d - sdh, p.inv, p.k0);
  const float qtop = fmaf(t0f, p.dq, base);
  const bool owned = valid && p.mask != 0 && (unsigned)d < (unsigned)nd && qtop >= qa && qtop < qb;
  const unsigned long long omask = __builtin_amdgcn_ballot_w64(owned);
  const bool any = omask != 0ull;
  const int l_first = any ? __builtin_ctzll(omask) : 0, l_last = any ? 63 - __builtin_clzll(omask) : 0;
  const float blo = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, base), l_first));
  const float bhi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, base), l_last));
  const int nch = (t1 - t0 + QD_R - 1) / QD_R;
  if (lane < nch) {
    const int tb = t0 + lane * QD_R, te = (tb + QD_R < t1) ? tb + QD_R : t1;
    ext[wv][lane][0] = any ? blo + (float)tb * p.dq : 3.0e38f;
    ext[wv][lane][1] = any ? bhi + (float)(te - 1) * p.dq : -3.0e38f;
  }
  if (threadIdx.x == 0) nfit = 0;
  __syncthreads();
  if (li == 0) P.dfirst[wv][hw] = dl0;
  if (lane == 0) {
    P.omask_lo[wv] = (unsigned)omask;
    P.omask_hi[wv] = (unsigned)(omask >> 32);
  }
  if (wv == 0 && lane < QD_MAXCH) {
    int csv = QD_NONE;
    if (lane < nch) {
      const float ulo = fminf(fminf(ext[0][lane][0], ext[1][lane][0]), fminf(ext[2][lane][0], ext[3][lane][0]));
      const float uhi = fmaxf(fmaxf(ext[0][lane][1], ext[1][lane][1]), fmaxf(ext[2][lane][1], ext[3][lane][1]));
      const bool nobody = ulo > uhi;
      const int cs = nobody ? 0 : (((int)floorf(ulo) - 1) & ~3);
      const bool fits = !nobody && ((int)floorf(nobody ? 0.f : uhi) + 2 - cs) < QD_W;
      if (!nobody) {
        csv = cs;
        if (!fits) atomicAdd(&nfit, 1);
      }
    }
    P.cs[lane] = csv;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool whole = (t1 - t0) % QD_R == 0;
    const bool fast = have_xT && whole && nfit == 0 && 4 * members >= 3 * 4 * nval;
    P.fast = fast ? 1 : 0;
    if (!fast) {
      const int k = atomicAdd(&slow[0], 1);
      slow[1 + k] = blockIdx.y * gridDim.x + blockIdx.x;
    }
  }
}

__global__ __launch_bounds__(256, 4) void k_radon_fwd_quadf(const float* __restrict__ img, const float* __restrict__ imgT,
                                                            float* __restrict__ out, int N, int nd,
                                                            const QuadParam* __restrict__ quads, int nq_per_frame, int ngrp_per_frame,
                                                            int na_per_frame, int nwin, int64_t band_stride, int bh,
                                                            const unsigned* __restrict__ A32q, const unsigned* __restrict__ B32q, int npad,
                                                            const QuadPlan* __restrict__ plan) {
  __shared__ __attribute__((aligned(16))) float tile[2][2 * QD_REGION];
  const QuadPlan& P = plan[(int64_t)blockIdx.y * gridDim.x + blockIdx.x];
  if (P.fast != 1) return;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int nw8 = (nwin + 7) >> 3;
  const int xcd = blockIdx.x & 7, bidx = blockIdx.x >> 3;
  const int grp = bidx / nw8;
  const int frame = grp / ngrp_per_frame;
  const int q0 = (grp - frame * ngrp_per_frame) * 4;
  const int nval = (nq_per_frame - q0 < 4) ? nq_per_frame - q0 : 4;
  const bool valid = wv < nval;
  const int qrow = frame * nq_per_frame + q0 + (valid ? wv : 0);
  const int t0 = blockIdx.y * bh;
  const int nch = ((t0 + bh < N ? bh : N - t0)) / QD_R;              // whole chunks only (the plan's condition)
  const int ndp = nd + 2 * A32_PAD;
  const unsigned img_bytes = (unsigned)N * (unsigned)N * 4u;
  const auto rsrc0 = __builtin_amdgcn_make_buffer_rsrc((void*)(img + (int64_t)frame * N * N), 0, img_bytes, 0x00020000);
  const auto rsrc1 = __builtin_amdgcn_make_buffer_rsrc((void*)(imgT + (int64_t)frame * N * N), 0, img_bytes, 0x00020000);
  const int hw = lane >> 5, li = lane & 31;
  const int d = P.dfirst[wv][hw] + li;
  const unsigned om_lo = P.omask_lo[wv], om_hi = P.omask_hi[wv];
  const bool any = (om_lo | om_hi) != 0u;
  const bool owned = (((hw ? om_hi : om_lo) >> li) & 1u) != 0u;
  const int dcl = d < 0 ? 0 : (d >= nd ? nd - 1 : d);
  const unsigned A = A32q[(int64_t)qrow * ndp + dcl + A32_PAD];
  // lanes without a ray follow the first owned ray of their half (of the other half if theirs owns none): a broadcast, inside the tile
  const int lf0 = om_lo ? __builtin_ctz(om_lo) : (om_hi ? 32 + __builtin_ctz(om_hi) : 0);
  const int lf1 = om_hi ? 32 + __builtin_ctz(om_hi) : lf0;
  const unsigned A_f0 = (unsigned)__builtin_amdgcn_readlane((int)A, lf0), A_f1 = (unsigned)__builtin_amdgcn_readlane((int)A, lf1);
  const unsigned A_m = owned ? A : (hw ? A_f1 : A_f0);
  const unsigned* __restrict__ Ball = B32q + (int64_t)qrow * npad + t0;
  float two32v = 4294967296.0f;                    // in a VECTOR register: an SGPR operand would make the subtraction a 4-cycle issue
  asm volatile("" : "+v"(two32v));
  const int cs_all = lane < QD_MAXCH ? P.cs[lane] : QD_NONE;
  // staging: wave wv fills row pair wv of region F and of region M, one load per source (lanes 0-59: row in pair = lane / 30, four
  // columns from 4 (lane % 30)); columns outside the image arrive as zeros (offset out of range).  Per chunk: the window start times
  // four plus a per-lane constant, and a range test — nothing else
  const int sr = lane >= 30 ? 1 : 0, sk = (lane - 30 * sr) << 2;
  const int cF = sk, cM = N - QD_W + sk;                                                  // column = cs + cF / cM - cs
  const int oF = ((2 * wv + sr) * N + sk) * 4, oM = ((2 * (QD_R / 2 - 1 - wv) + 1 - sr) * N + (N - QD_W + sk)) * 4;
  const unsigned row8 = (unsigned)QD_R * (unsigned)N * 4u;
  unsigned rowbase = (unsigned)t0 * (unsigned)N * 4u + row8;                              // of the chunk being staged (chunk 1 first)
  auto stage = [&](int buf, int cs, unsigned rb) {
    float* __restrict__ T = tile[buf];
    const int cs4 = cs << 2;
    const int voffF = ((unsigned)(cs + cF) < (unsigned)N) ? cs4 + oF : (int)img_bytes;
    const int voffM = ((unsigned)(cM - cs) < (unsigned)N) ? oM - cs4 : (int)img_bytes;
    auto* dF = (__attribute__((address_space(3))) void*)(T + wv * QD_PAIR);
    auto* dFt = (__attribute__((address_space(3))) void*)(T + wv * QD_PAIR + QD_SRC);
    auto* dM = (__attribute__((address_space(3))) void*)(T + QD_REGION + wv * QD_PAIR);
    auto* dMt = (__attribute__((address_space(3))) void*)(T + QD_REGION + wv * QD_PAIR + QD_SRC);
    if (lane < 60) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc0, dF, 16, voffF, rb, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc1, dFt, 16, voffF, rb, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc0, dM, 16, voffM, rb, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc1, dMt, 16, voffM, rb, 0, 0);
    }
  };
  f2v acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
  double total[4] = {0.0, 0.0, 0.0, 0.0};
  int cs = __builtin_amdgcn_readlane(cs_all, 0);
  if (cs != QD_NONE) stage(0, cs, rowbase - row8);
  typedef unsigned u8v __attribute__((ext_vector_type(8)));
  for (int ch = 0; ch < nch; ++ch) {
    const int cs_nx = ch + 1 < nch ? __builtin_amdgcn_readlane(cs_all, ch + 1) : QD_NONE;
    // the chunk's eight B32 entries: one scalar load, requested before the barrier
    const u8v Bv = *reinterpret_cast<const u8v*>(__builtin_assume_aligned(Ball + ch * QD_R, 32));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // this wave's share of chunk ch has landed ...
    asm volatile("s_barrier" ::: "memory");                          // ... everybody's; and everybody has left the other buffer
    if (cs_nx != QD_NONE) stage((ch + 1) & 1, cs_nx, rowbase);
    rowbase += row8;
    if (cs != QD_NONE && any) {
      const unsigned Ac = A_m - ((unsigned)cs << QF);
      const unsigned Toff = lds_off(tile[ch & 1]);
      unsigned Cm = 2u * Toff + 4u * (unsigned)(QD_REGION + (QD_R / 2 - 1) * QD_PAIR + QD_W + (QD_W - 2));
      asm volatile("" : "+v"(Cm));
      f2v w[QD_R];
      unsigned a0[QD_R], a1[QD_R];
      auto prep = [&](int u) {
        const unsigned Q = Ac + Bv[u];
        const float f1 = (float)(Q << 8);                           // the 24 fraction bits, in units of 2^-32 (exact)
        const float f0 = two32v - f1;
        w[u] = (f2v){f0, f1};
        int rowoff = (int)Toff + ((u >> 1) * QD_PAIR + (u & 1) * QD_W) * 4;
        asm("" : "+s"(rowoff));
        a0[u] = ((Q >> QF) << 2) + (unsigned)rowoff;
        a1[u] = Cm - a0[u];
      };
      f2v tA[QD_R], tB[QD_R], tC[QD_R], tD[QD_R];
      auto issue = [&](int u) {
        asm volatile("ds_read2_b32 %0, %1 offset1:1" : "=v"(tA[u]) : "v"(a0[u]));
        asm volatile("ds_read2_b32 %0, %1 offset0:240 offset1:241" : "=v"(tB[u]) : "v"(a0[u]));
        asm volatile("ds_read2_b32 %0, %1 offset1:1" : "=v"(tC[u]) : "v"(a1[u]));
        asm volatile("ds_read2_b32 %0, %1 offset0:240 offset1:241" : "=v"(tD[u]) : "v"(a1[u]));
      };
      prep(0);
      issue(0);
      prep(1);
      issue(1);
      prep(2);
      issue(2);
#pragma unroll
      for (int u = 0; u < QD_R; ++u) {
        if (u + 3 < QD_R) prep(u + 3);
        if (u <= QD_R - 3) asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
        else if (u == QD_R - 2) asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        asm volatile("" : "+v"(tA[u]), "+v"(tB[u]), "+v"(tC[u]), "+v"(tD[u]));
        if (u + 3 < QD_R) issue(u + 3);
        acc[0] = __builtin_elementwise_fma(w[u], tA[u], acc[0]);
        acc[2] = __builtin_elementwise_fma(w[u], tB[u], acc[2]);
        // mirrored windows: the pair read at the mirrored address is (tap c+1, tap c): the weights swap halves
        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[0,1,1]" : "+v"(acc[1]) : "v"(w[u]), "v"(tC[u]));
        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[0,1,1]" : "+v"(acc[3]) : "v"(w[u]), "v"(tD[u]));
      }
    }
    if ((ch & 1) || ch == nch - 1) {                               // fp32 partial sums over 16 rows, then fp64 (as the other forward kernels)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        total[m] += (double)(acc[m][0] + acc[m][1]);
        acc[m] = (f2v){0.f, 0.f};
      }
    }
    cs = cs_nx;
  }
  if (owned) {
    const QuadParam p = quads[qrow];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      if (!((p.mask >> m) & 1)) continue;
      const int dm = ((p.flip >> m) & 1) ? nd - 1 - d : d;
      out[(int64_t)blockIdx.y * band_stride + ((int64_t)frame * na_per_frame + p.am[m]) * nd + dm] = (float)total[m];
    }
  }
}

// ---------------------------------------------------------------------------------------- forward, band-resident (small images; round 5)
// At 512^2 (C3) k_radon_fwd_lds spends 45 % of its vector instructions on staging a window per wave and 16 rows (addresses of 7
// loads, window bookkeeping, the wait for the loads), and its 2 160 workgroups of four waves run in 1.7 rounds.  A band of 64 rows of a
// 512-wide image is 130 KB: it FITS the LDS of one CU.  Here a workgroup of 16 waves loads its band once — rows of the image for the
// row-driven angles, rows of the transposed image for the column-driven ones, zero columns either side — and every wave then marches
// (angle, 64 detectors) tasks through all 64 rows with no staging, no barrier and no load left in the loop: per 16 rows one window
// start (the tables know the column mod 256), then the seven instructions of a step.  Chunks of 16 rows in fp32, flushed to float64,
// as k_radon_fwd_lds sums them; the band partials go to the same array (64-row bands).  Grid: frames x {row bands, column bands} x
// slices of that mode's angle list (adj_ang: the angles sorted by mode), about one workgroup per CU.
constexpr int BR_FLUSH_SHIFT = 2;                      // fp32 sums of 4 rows, then float64
__global__ __launch_bounds__(BR_NT, 4) void k_radon_fwd_band(const float* __restrict__ img, const float* __restrict__ imgT,
                                                             float* __restrict__ part, int N, int nd,
                                                             const AngleParam* __restrict__ ang, int na,
                                                             const AdjAngle* __restrict__ sorted, const int* __restrict__ n_mode0,
                                                             int nslice, int64_t band_stride,
                                                             const unsigned* __restrict__ A32, const unsigned* __restrict__ B32, int npad,
                                                             int have_xT, int rows) {
  extern __shared__ __attribute__((aligned(16))) float band[];   // rows x (N + 2 BR_PAD) floats, then the task counter
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int nbands = N / rows;
  const int nw = (int)(blockDim.x >> 6), nthr = (int)blockDim.x;   // 16 waves (one workgroup per CU) or 8 (narrow images: two per CU)
  int& next_task = *reinterpret_cast<int*>(band + rows * (N + 2 * BR_PAD));
  // blockIdx.x = ((frame * 2 + mode) * nbands + b) * nslice + slice
  int bid = blockIdx.x;
  const int slice = bid % nslice; bid /= nslice;
  const int b = bid % nbands; bid /= nbands;
  const int mode = bid & 1, frame = bid >> 1;
  const int n0 = n_mode0[frame];
  const int cnt = mode ? na - n0 : n0;                           // angles of this mode in the frame
  const int ndblk = (nd + 63) / 64;
  // the mode's (angle, 64 detectors) tasks in list order, dealt to the slices in equal contiguous shares
  const int all_tasks = cnt * ndblk;
  const int task0 = (int)((int64_t)all_tasks * slice / nslice), task1 = (int)((int64_t)all_tasks * (slice + 1) / nslice);
  if (task1 <= task0) return;
  const int RS = N + 2 * BR_PAD;                                 // row stride in floats (a multiple of 4)
  if (mode && !have_xT) {
    // no transposed copy at hand: the band of the transposed image is 64 COLUMNS of the image — a wave-load takes 16 image rows x 16
    // columns (whole 64-byte sectors), a lane's four values go to four rows of the band (consecutive lanes: consecutive addresses)
    const float* __restrict__ X = img + (int64_t)frame * N * N + (int64_t)b * rows;
    const int r = lane & 15, jq = lane >> 4;
    const int cgs = rows / 16, pieces = (N / 16) * cgs;            // (16-row group, 16-column group)
    for (int p0 = wv; p0 < pieces; p0 += 4 * nw) {
      f4r v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pc = p0 + u * nw;
        const int rg = pc / cgs, cg = pc - rg * cgs;
        v[u] = pc < pieces ? *reinterpret_cast<const f4r*>(X + (int64_t)(16 * rg + r) * N + 16 * cg + 4 * jq) : (f4r){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pc = p0 + u * nw;
        if (pc < pieces) {
          const int rg = pc / cgs, cg = pc - rg * cgs;
#pragma unroll
          for (int e = 0; e < 4; ++e) band[(16 * cg + 4 * jq + e) * RS + BR_PAD + 16 * rg + r] = v[u][e];
        }
      }
    }
  } else {
    // the band: 64 rows x N floats as float4, 8 (N = 512) per thread in flight
    const float* __restrict__ I = (mode ? imgT : img) + (int64_t)frame * N * N + (int64_t)b * rows * N;
    const int q4 = N / 4, tot = rows * q4;
    for (int i0 = threadIdx.x; i0 < tot; i0 += 8 * nthr) {
      f4r v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = i0 + u * nthr;
        v[u] = idx < tot ? *reinterpret_cast<const f4r*>(I + 4 * (int64_t)idx) : (f4r){0.f, 0.f, 0.f, 0.f};   // (row * N + 4 c4 = 4 idx)
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = i0 + u * nthr;
        if (idx < tot) {
          const int row = idx / q4, c4 = idx - row * q4;
          *reinterpret_cast<f4r*>(&band[row * RS + BR_PAD + 4 * c4]) = v[u];
        }
      }
    }
  }
  // the pads are zeros
  if (threadIdx.x < rows * 2) {
    const int row = threadIdx.x >> 1, side = threadIdx.x & 1;
    *reinterpret_cast<f4r*>(&band[row * RS + (side ? BR_PAD + N : 0)]) = (f4r){0.f, 0.f, 0.f, 0.f};
  }
  if (threadIdx.x == 0) next_task = task0 + nw;
  __syncthreads();
  float two32 = 4294967296.0f;
  asm("" : "+s"(two32));
  const int t0 = b * rows;
  const float sdh = 0.5f * (float)(nd - 1);
  const int ndp = nd + 2 * A32_PAD;
  // a wave takes the next task when it has finished one (tasks at the image's edge and beside it cost differently).  (Fetching the
  // NEXT task's angle constants and table entries while the current one is marched, and the four chunks' windows at once, one per lane:
  // measured 21.8 us against 20.4 — not kept.  Nor the band in two halves, rows 32-63 still in flight while every wave marches the first
  // two chunks of its first task: 21.9 us.  Nor the row stride as a compile-time constant with the row offsets as immediates of two hand-issued
  // ds_read_b32 per step (no scalar instruction per step: 80 -> 45 per chunk, twice the LDS instructions): 27.3 us per plain apply against 26.2.)
  for (int task = task0 + wv; task < task1;) {
    const int ai = task / ndblk, dblk = task - ai * ndblk;
    const int a = frame * na + sorted[frame * na + (mode ? n0 : 0) + ai].orig;                    // (scalar loads)
    const AngleParam p = ang[a];
    const int nlive = (nd - dblk * 64 < 64) ? nd - dblk * 64 : 64;
    const bool live = lane < nlive;
    const int d = dblk * 64 + lane;
    const unsigned A = A32[(int64_t)a * ndp + (live ? d : nd - 1) + A32_PAD];      // dead lanes repeat the last ray; never stored
    const unsigned* __restrict__ Ball = B32 + (int64_t)a * npad;
    const float b0 = fmaf((float)(dblk * 64) - sdh, p.inv, p.k0), b1 = fmaf((float)(dblk * 64 + nlive - 1) - sdh, p.inv, p.k0);
    const float blo = fminf(b0, b1), bhi = fmaxf(b0, b1);
    double total = 0.0;
#pragma unroll 1
    for (int c = 0; c < rows / 16; ++c) {
      const int tb = t0 + 16 * c;
      const float ta = (float)tb * p.dq, tz = (float)(tb + 15) * p.dq;
      const float qlo = blo + fminf(ta, tz), qhi = bhi + fmaxf(ta, tz);
      if (__builtin_amdgcn_readfirstlane((qhi < -2.f || qlo > (float)N + 1.f) ? 1 : 0)) continue;      // nothing of the wave touches the image here
      const int cs = __builtin_amdgcn_readfirstlane((int)floorf(qlo) - 1);
      const int ce = __builtin_amdgcn_readfirstlane((int)floorf(qhi) + 2);
      const unsigned* __restrict__ Brow = static_cast<const unsigned*>(__builtin_assume_aligned(Ball + tb, 64));
      const unsigned Ac = A - ((unsigned)cs << QF);              // column relative to cs (mod 256: the window is < 256 wide)
      const char* rowp = reinterpret_cast<const char*>(band) + (16 * c) * RS * 4;
      // fp32 sums of FOUR rows, then float64 (round 6; rounds 2-5: of sixteen).  The float64 instrument (profiles/r05/c3_instrument.txt)
      // showed what the longer fp32 chains cost where the solver amplifies roundings — iterates 5-7 of C3's transient sat 44-90 x
      // above the fp32-storage floor with 16-row sums and on it with 4-row sums (R.set_ref_sums(4, 32))
      f2v acc2[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
      if (cs >= 0 && ce <= N - 1) {
        // every tap of the wave inside the image: address = row (scalar) + 4 (cs + pad) (scalar) + 4 * relative column
        f2v w[16], t2[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const unsigned Q = Ac + Brow[u];
          const float f1 = (float)(Q << 8);
          w[u][1] = f1;
          w[u][0] = two32 - f1;
          int off = u * RS * 4 + (cs + BR_PAD) * 4;
          asm("" : "+s"(off));
          const float* tp = reinterpret_cast<const float*>(rowp + off + ((Q >> QF) << 2));
          t2[u] = (f2v){tp[0], tp[1]};
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) acc2[u >> BR_FLUSH_SHIFT] = __builtin_elementwise_fma(w[u], t2[u], acc2[u >> BR_FLUSH_SHIFT]);
      } else {
        // the window overhangs the image: columns clamped into the zero pads ([-2, N]: both taps of a clamped step read zeros)
        f2v w[16], t2[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const unsigned Q = Ac + Brow[u];
          const float f1 = (float)(Q << 8);
          w[u][1] = f1;
          w[u][0] = two32 - f1;
          int col = cs + (int)(Q >> QF);
          asm("v_med3_i32 %0, %1, -2, %2" : "=v"(col) : "v"(col), "s"(N));
          int off = u * RS * 4 + BR_PAD * 4;
          asm("" : "+s"(off));
          const float* tp = reinterpret_cast<const float*>(rowp + off + (col << 2));
          t2[u] = (f2v){tp[0], tp[1]};
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) acc2[u >> BR_FLUSH_SHIFT] = __builtin_elementwise_fma(w[u], t2[u], acc2[u >> BR_FLUSH_SHIFT]);
      }
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) total += (double)(acc2[g4][0] + acc2[g4][1]);
    }
    if (live) part[(int64_t)b * band_stride + (int64_t)a * nd + d] = (float)total;
    int nx = 0;
    if (lane == 0) nx = atomicAdd(&next_task, 1);
    task = __builtin_amdgcn_readfirstlane(nx);
  }
}

// sino[a][d] = wgt_a * sum over bands (fixed order, fp64) of the band partial sums, then the optional epilogue
// a * sino + b * z.  One thread per (angle row, e = d + A32_PAD in [0, nd + 4)): the padding positions exist for REC, which
// also writes the adjoint's record {w S[d -], w S[d +], w S[d], A32[d]} of every position (what k_radon_adj_prep would
// make from the finished sinogram; the neighbours come through LDS, the two at the block's edges are recomputed).
// ssq_part != NULL: sum(out^2) of this block's outputs in ssq_part[blockIdx.x].
template <bool REC>
__global__ __launch_bounds__(256) void k_radon_bands_post(const float* __restrict__ part, int nb, int64_t band_stride,
                                                          float* __restrict__ sino, int nd, const AngleParam* __restrict__ ang,
                                                          Epi epi, double* __restrict__ ssq_part,
                                                          uint4* __restrict__ rec, const int4* __restrict__ adj_pos,
                                                          const AdjAngle* __restrict__ adj_ang, const float* __restrict__ adj_wgt,
                                                          const unsigned* __restrict__ A32) {
  __shared__ double lds[4];
  __shared__ float sv[258];
  const int ndp = nd + 2 * A32_PAD;
  const int64_t rows = band_stride / nd;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = idx / ndp;
  const int e = (int)(idx - row * ndp), d = e - A32_PAD;
  const bool valid = row < rows;
  // the loads first, the coefficients (which may wait for the pending partials) after: two latency chains side by side
  struct Raw { float o, z; };
  auto raw = [&](int64_t r, int dd) -> Raw {
    if (dd < 0 || dd >= nd) return Raw{0.f, 0.f};
    const int64_t k = r * nd + dd;
    double t = 0.0;
    for (int b0 = 0; b0 < nb; b0 += 8) {           // eight band partials in flight (all of a 512-row image's 64-row bands), added in band order
      float pv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) pv[u] = (b0 + u < nb) ? part[(int64_t)(b0 + u) * band_stride + k] : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) t += (double)pv[u];
    }
    return Raw{ang[r].wgt * (float)t, (epi.on && epi.z) ? epi.z[k] : 0.f};
  };
  const Raw r0 = valid ? raw(row, d) : Raw{0.f, 0.f};
  const float dv = (epi.dot_part && valid && d >= 0 && d < nd) ? epi.dotv[row * nd + d] : 0.f;
  Raw rm{0.f, 0.f}, rp{0.f, 0.f};
  if (REC) {
    if (threadIdx.x == 0 && valid && e > 0) rm = raw(row, d - 1);
    if (threadIdx.x == 255 && valid && e < ndp - 1) rp = raw(row, d + 1);
  }
  int64_t rs = 0;
  float w = 0.f;
  bool flip = false;
  unsigned a32 = 0u;
  if (REC && valid) {
    const int4 rr = adj_pos[row];
    rs = rr.x;
    w = __builtin_bit_cast(float, rr.y);
    flip = rr.z != 0;
    a32 = A32[row * ndp + e];
  }
  float ca, cb;
  double cad, cbd;
  epi_coefs(epi, blockIdx.x == 0, &lds[0], ca, cb, nullptr, &cad, &cbd);
  auto fin = [&](const Raw& v) -> float { return epi.on ? epi_combine(epi.on, ca, cb, cad, cbd, v.o, v.z, epi.z != nullptr) : v.o; };
  const bool inr = valid && d >= 0 && d < nd;
  const float v0 = inr ? fin(r0) : 0.f;
  if (inr) sino[row * nd + d] = v0;
  if (REC) {
    sv[threadIdx.x + 1] = v0;
    if (threadIdx.x == 0) sv[0] = (valid && e > 0 && d - 1 >= 0 && d - 1 < nd) ? fin(rm) : 0.f;
    if (threadIdx.x == 255) sv[257] = (valid && e < ndp - 1 && d + 1 >= 0 && d + 1 < nd) ? fin(rp) : 0.f;
    __syncthreads();
    if (valid) {
      const float vm = e > 0 ? sv[threadIdx.x] : 0.f, vp = e < ndp - 1 ? sv[threadIdx.x + 2] : 0.f;
      const float sm = w * vm, sp = w * vp;          // (0 outside the detector)
      uint4 o;
      o.x = __builtin_bit_cast(unsigned, flip ? sp : sm);
      o.y = __builtin_bit_cast(unsigned, flip ? sm : sp);
      o.z = __builtin_bit_cast(unsigned, w * v0);
      o.w = a32;
      rec[rs * ndp + e] = o;
    }
  }
  if (ssq_part) {                                                 // uniform over the grid
    const double q = block_sum<256>((double)v0 * v0, lds);
    if (threadIdx.x == 0) ssq_part[blockIdx.x] = q;
  }
  if (epi.dot_part) {                                             // uniform over the grid
    const double q = block_sum<256>((double)v0 * dv, lds);
    if (threadIdx.x == 0) epi.dot_part[blockIdx.x] = q;
  }
}

}  // namespace

namespace trk {
namespace radon {

// Which forward kernel an input at `xb` gets: per-wave LDS windows (N % 4 == 0, 16-byte aligned input; staged by direct-to-LDS
// loads), the quad kernels from 1024^2 on (win: four symmetric angles per wave, conflict-free half-wave windows shared by the four
// quads of a workgroup), else direct gathers.  direct1: the per-wave-window kernel reads the angles marched along columns from the
// image itself, transposing while it stages — no transposed copy, no launch for it (512^2 x 180: the copy was 5 of the apply's
// 31 us; 32 frames of 256^2: 5.8 of 23).  The quad kernels keep the copy (2.6 % at 4096^2).
// (Global -> LDS directly, buffer_load_dwordx4 ... lds, new on gfx950, instead of through registers: 1.30 -> 1.11 ms at 4096^2.)
FwdPath fwd_path(const RadonImpl* im, const float* xb) {
  FwdPath f;
  f.lds = (im->N % 4 == 0) && ((reinterpret_cast<uintptr_t>(xb) & 15u) == 0);
  // measured: 512^2 35 us (shared windows) vs 32 us (per-wave windows); 2048^2 0.256 vs 0.277 ms; 4096^2 0.96 vs 1.11 ms, and with
  // the quads 0.94 -> see DESIGN.md 4.4.  (Every handle has at least one quad per frame, and without band_res a band is at most 256 =
  // QD_R * QD_MAXCH rows: radon_create_impl)
  f.win = im->n_bands > 1 && im->N >= 1024 && f.lds && im->band <= QD_R * QD_MAXCH && !im->band_res;
  f.direct1 = f.lds && !f.win;
  return f;
}

int radon_forward(RadonImpl* im, const float* xb, float* yb, int hints, bool post, bool want_rec, const Epi& epi, double* ssq_part,
                  int64_t post_blocks, hipStream_t s) {
  const int N = im->N, nd = im->nd, na = im->na, nt = im->nt;
  const FwdPath fp = fwd_path(im, xb);
  const bool lds = fp.lds;
  // the adjoint that produced xb may have left its transpose in xT already (hinted chain): then the copy costs nothing and the
  // kernel without the transposing staging is the faster one (512^2 x 180 inside Golub-Kahan: 24.5 vs 27.6 us)
  const bool have_xT = im->n_mode1 > 0 && (hints & HINT_INPUT_FROM_OPPOSITE) && im->xT_src == xb;
  const bool band_res = im->band_res && !fp.win && lds;
  const int direct1 = (fp.direct1 && !have_xT && !band_res) ? 1 : 0;
  if (im->n_mode1 > 0 && !direct1 && !band_res && !have_xT) {
    dim3 g(ceil_div(N, 32), ceil_div(N, 32), nt);
    hipLaunchKernelGGL(k_transpose, g, dim3(256), 0, s, xb, im->xT, N);
  }
  im->xT_src = nullptr;              // holds for this apply only: the caller's promise covers the very next one
  const int ndblk = ceil_div(nd, 64), ngrp = ceil_div(na, 4), nb = im->n_bands;
  const int64_t bs = (int64_t)nt * na * nd;
  dim3 grid(ndblk * ngrp * nt, nb, 1);
  if (band_res) {
    const int rows = im->band, nbr = N / rows;
    // one workgroup of 16 waves per CU whatever the width (measured at 32 frames of 256^2: two workgroups of 8 waves per CU, which the
    // narrower band's LDS would allow, 18.4 us against 16.5)
    const size_t lds_bytes = sizeof(float) * (size_t)rows * (N + 2 * BR_PAD) + 16;
    int nslice = (cu_count() + nt * 2 * nbr / 2) / (nt * 2 * nbr);
    if (nslice < 1) nslice = 1;
    static bool attr_set = false;
    if (!attr_set) {
      TRK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_radon_fwd_band), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      attr_set = true;
    }
    hipLaunchKernelGGL(k_radon_fwd_band, dim3((unsigned)(nt * 2 * nbr * nslice)), dim3(BR_NT), lds_bytes, s, xb, im->xT, im->part, N, nd, im->ang_dev,
                       na, im->adj_ang, im->adj_n0, nslice, bs, im->A32, im->B32, im->npad, have_xT ? 1 : 0, rows);
  } else if (fp.win) {
    // quad kernels: band partials of rays no window owns must read as zero
    if (hipMemsetAsync(im->part, 0, sizeof(float) * (size_t)nb * bs, s) != hipSuccess) return fail(TRK_EHIP, "radon: hipMemsetAsync failed");
    const int nwq = ceil_div(N + im->band + 4, QD_WO), ngq = ceil_div(im->nq, 4);
    dim3 gq(8 * ceil_div(nwq, 8) * ngq * nt, nb, 1);           // windows dealt to the XCDs in contiguous eighths (see the kernel)
    // round 6: the lean kernel for the workgroups its plan allows, k_radon_fwd_quad for the listed rest (TRK_RADON_NO_QUADF=1: all
    // of them, as rounds 4-5).  The plan depends on the geometry and the grid only: made at the first apply, kept with the handle
    const bool no_quadf = getenv("TRK_RADON_NO_QUADF") != nullptr;      // read per call: the tests switch it
    dim3 gslow = gq;
    const int* wg_list = nullptr;
    if (!no_quadf) {
      if (!im->qplan || im->qplan_gx != (int)gq.x || im->qplan_nb != nb) {
        if (im->qplan) (void)hipFree(im->qplan);
        if (im->qslow) (void)hipFree(im->qslow);
        im->qplan = nullptr;
        im->qslow = nullptr;
        const size_t nwg = (size_t)gq.x * nb;
        TRK_HIP(hipMalloc((void**)&im->qplan, sizeof(QuadPlan) * nwg));
        TRK_HIP(hipMalloc((void**)&im->qslow, sizeof(int) * (nwg + 1)));
        TRK_HIP(hipMemsetAsync(im->qslow, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_radon_quad_plan, gq, dim3(256), 0, s, N, nd, im->quad_dev, im->nq, ngq, nwq, im->band, im->fidx,
                           im->xT ? 1 : 0, im->qplan, im->qslow);
        TRK_HIP(hipMemcpyAsync(&im->qslow_n, im->qslow, sizeof(int), hipMemcpyDeviceToHost, s));
        TRK_HIP(hipStreamSynchronize(s));
        im->qplan_gx = (int)gq.x;
        im->qplan_nb = nb;
      }
      hipLaunchKernelGGL(k_radon_fwd_quadf, gq, dim3(256), 0, s, xb, im->xT, im->part, N, nd, im->quad_dev, im->nq, ngq, na, nwq, bs, im->band,
                         im->A32q, im->B32q, im->npad, im->qplan);
      gslow = dim3((unsigned)im->qslow_n, 1, 1);
      wg_list = im->qslow;
    }
    if (gslow.x > 0)
      hipLaunchKernelGGL(k_radon_fwd_quad, gslow, dim3(256), 0, s, xb, im->xT, im->part, N, nd, im->quad_dev, im->nq, ngq, na, nwq, bs,
                         im->band, im->fidx, im->A32q, im->B32q, im->npad, im->ang_dev, im->A32, im->B32, wg_list, (int)gq.x);
  } else if (!post) {
    if (lds) hipLaunchKernelGGL(k_radon_fwd_lds<true>, grid, dim3(256), 0, s, xb, im->xT, yb, N, nd, im->ang_dev, na, ngrp, ndblk, bs, im->band, im->A32, im->B32, im->npad, direct1);
    else hipLaunchKernelGGL(k_radon_fwd<true>, grid, dim3(256), 0, s, xb, im->xT, yb, N, nd, im->ang_dev, na, ngrp, ndblk, bs, im->band, im->A32, im->B32, im->npad);
  } else {
    if (lds) hipLaunchKernelGGL(k_radon_fwd_lds<false>, grid, dim3(256), 0, s, xb, im->xT, im->part, N, nd, im->ang_dev, na, ngrp, ndblk, bs, im->band, im->A32, im->B32, im->npad, direct1);
    else hipLaunchKernelGGL(k_radon_fwd<false>, grid, dim3(256), 0, s, xb, im->xT, im->part, N, nd, im->ang_dev, na, ngrp, ndblk, bs, im->band, im->A32, im->B32, im->npad);
  }
  if (post) {
    if (want_rec)
      hipLaunchKernelGGL(k_radon_bands_post<true>, dim3((unsigned)post_blocks), dim3(256), 0, s, im->part, nb, bs, yb, nd, im->ang_dev, epi,
                         ssq_part, im->rec, im->adj_pos, im->adj_ang, im->adj_wgt, im->A32);
    else
      hipLaunchKernelGGL(k_radon_bands_post<false>, dim3((unsigned)post_blocks), dim3(256), 0, s, im->part, nb, bs, yb, nd, im->ang_dev, epi,
                         ssq_part, im->rec, im->adj_pos, im->adj_ang, im->adj_wgt, im->A32);
    if (want_rec) im->rec_src = yb;
  }
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

}  // namespace radon
}  // namespace trk
