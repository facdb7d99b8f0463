// radon_internal.h — what the parallel-beam projector's three sources share (radon2d.hip: handle, tables, apply bookkeeping;
// radon_fwd.hip: forward kernels; radon_adj.hip: adjoint kernels) and nobody else includes.  Geometry and the fixed-point ray
// coordinate: the comment at the head of radon2d.hip.
#pragma once
#include "trk_internal.h"

#include <cstdint>

namespace trk {
namespace radon {

constexpr int QF = 24;                          // fractional bits of the fixed-point ray coordinate
constexpr float QONE = 16777216.0f;             // 2^24: the adjoint's weights are in units of 2^-24
constexpr float QTWO32 = 4294967296.0f;         // 2^32: the forward's weights are in units of 2^-32 ((float)(Q << 8))
constexpr int A32_PAD = 2;                      // A32 rows hold d = -2 .. nd+1

// tile geometry the handle is sized by (radon_create_impl) next to the kernels that march it
constexpr int RADON_BAND = 128;   // rows of a forward band (k_radon_fwd, k_radon_fwd_lds; the quad kernels: 128 or 256)
constexpr int QD_R = 8;           // rows of a chunk of the quad forward kernels
constexpr int QD_MAXCH = 32;      // chunks of a band, at most
constexpr int ADJ_T = 32;           // adjoint: tile edge (pixels) of the large-image instantiation; small images: 16 x 16, one pixel per thread
// band-resident forward (k_radon_fwd_band)
constexpr int BR_ROWS = 64, BR_NW = 16, BR_NT = 64 * BR_NW, BR_PAD = 4, BR_NMAX = 1024;
// rows per band: 64 where 64 x (N + 8) floats fit in 150 KB (N <= 592, i.e. the multiples of 64 up to 576), else 32 (N <= 1024: 132 KB)
inline int br_rows(int N) { return (size_t)BR_ROWS * (N + 2 * BR_PAD) * 4 <= 150 * 1024 ? BR_ROWS : BR_ROWS / 2; }

struct AngleParam {
  float inv, dq, k0, wgt;   // fp32 copies: only for ESTIMATES (window placement, candidate location); wgt includes the forward's 2^-32
  int mode;
  float rinv;               // ~1/inv
};

struct alignas(8) AdjAngle { // the adjoint's per-angle constants, sorted by marching mode per frame
  float c1m, c1p;           // 1 - |inv| (<= 0) ON THE 2^-24 GRID, for the neighbour on the smaller-q / larger-q side: a neighbouring ray at
                            // distance |inv| weighs clamp(c1m + t0) / clamp(c1p - t0).  Read as ONE scalar pair: the packed FMA's
                            // addend (adj_gather).  Which grid neighbours of the real 1 - |inv| the two hold is chosen when the handle is
                            // made (radon_create_impl: error diffusion over the angles)
  float rinv, dq, k0;
  int orig;                 // index of the angle within its frame
  int flip;                 // inv < 0: the ray on the larger-q side is d0 - 1 (the records store neighbours by side)
  int pad_;
};

struct alignas(8) AdjQuad {  // base geometry of a quad for the adjoint: c1m / c1p = 1 - inv (<= 0) on the 2^-24 grid (as AdjAngle's),
  float c1m, c1p;           // rinv = cos(beta), dq = tan(beta), k0 = h (1 - dq)
  float rinv, dq, k0;
  int pad_;
};

struct QuadParam {
  float inv, dq, k0, rinv;   // base geometry: inv = 1/cos(beta) in [1, sqrt 2], dq = tan(beta) in [0, 1], k0 = h (1 - dq), rinv = cos(beta)
  int am[4];                 // member angle of each slot (index within the frame), -1: none
  int flip;                  // bit m: member m writes detector nd - 1 - d
  int mask;                  // bit m: slot m has a member
  int pad0, pad1;
};
// per-workgroup bookkeeping of the quad forward kernels, made once per operator (k_radon_quad_plan)
struct QuadPlan {
  int cs[QD_MAXCH];              // window start of every chunk; QD_NONE: no wave owns a ray there
  int dfirst[4][2];              // [wave][half]: the detector of lane li = 0 of that half (lane li: + li)
  unsigned omask_lo[4], omask_hi[4];   // the lanes that own a ray
  int fast;                      // 1: k_radon_fwd_quadf; 0: k_radon_fwd_quad (listed); 2: nothing to do
  int pad[64 - QD_MAXCH - 8 - 8 - 1];
};
static_assert(sizeof(QuadPlan) == 256, "one plan entry = 256 bytes");

struct RadonImpl {
  int N, nd, na;   // na = angles PER FRAME
  int nt;          // time frames sharing one launch (block-diagonal dynamic operator, io.py:391-420); 1 = static
  AngleParam* ang_dev;   // nt*na entries, frame-major
  float* xT;  // nt*N*N transposed images (forward, mode-1 angles); owned by the handle (non-reentrant across streams)
  int n_mode1;
  float* part;  // [n_bands][nt*na][nd] forward band partial sums (n_bands > 1 only); owned by the handle
  float* fidx;  // fidx[i] = (float) i, i < N + 16
  unsigned* A32;  // [nt*na][nd + 4]
  unsigned* B32;  // [nt*na][npad]
  uint2* CB;      // [nt*na][npad]: {C[a][tt] as float bits, B32[a][tt]}, C = the adjoint's locator offset
  int npad;
  // adjoint: angles sorted by mode per frame; per apply a record array {w S[d-1], w S[d], w S[d+1], A32[d]}
  AdjAngle* adj_ang;
  float* adj_wgt;
  int* adj_n0;
  uint4* rec;
  int4* adj_pos;     // [nt*na]: angle row (caller's order) -> {its sorted row (the inverse of adj_ang[].orig), that row's
                     // adjoint weight (bits), its flip flag, 0}: one load where the record writer chased three
  int n_bands, band;
  int band_res;     // forward by k_radon_fwd_band: 64-row bands resident in LDS (small images)
  // adjoint with the angles of a tile split over `nsplit` workgroups (small images): partial tiles and one counter per tile
  float* adj_part;
  unsigned* adj_cnt;
  int64_t adj_part_cap, adj_cnt_cap;
  // quads: groups of up to four symmetric angles served by one wave of k_radon_fwd_quad (nq per frame, padded with empty ones)
  QuadParam* quad_dev;
  unsigned* A32q;   // [nt*nq][nd + 4]  base tables
  unsigned* B32q;   // [nt*nq][npad]
  int nq;
  // round 6: the quad kernel's per-workgroup bookkeeping made once per operator (k_radon_quad_plan) and the compact list of the
  // workgroups the lean kernel (k_radon_fwd_quadf) does not serve
  // round 6, adjoint by mirrored tile pairs (k_radon_adj_quad): per quad {c1, rinv, dq, k0} of the BASE geometry, {C, B32} of the base per
  // marching index, the members' weights; recq = per-apply records indexed by (quad, slot, BASE detector)
  struct AdjQuad* adjq;
  uint2* CBq;        // [nt*nq][npad]
  float* wq;         // [nt*nq][4]
  uint4* recq;       // [nt*nq][4][nd + 4]
  int adjq_ok;
  struct QuadPlan* qplan;
  int* qslow;       // [0] = count, then the workgroup ids (band * grid_x + block) k_radon_fwd_quad still runs
  int qslow_n;      // host copy of the count
  int qplan_gx, qplan_nb;   // the grid the plan was made for
  // what the side buffers currently hold, when a fused apply left them behind for the next apply of the other direction
  // (trk_op_apply_axpby hints): rec = the records of the sinogram at rec_src, xT = the transpose of the image at xT_src
  const float* rec_src;
  const float* xT_src;
  // a fused norm left as block partials (TRK_HINT_SUMSQ_DEFERRED): pend_n partials in pend_buf[pend_which ^ 1] belong to
  // *pend_target; the next chained apply's epilogue kernel finishes it, anything else calls radon_flush first
  double* pend_buf[2];
  int64_t pend_cap;
  int pend_which;
  double* pend_target;
  const double* pend_part;
  int pend_n;
  // the float64 instrument (ref64.hip): the angles in float64, and the arithmetic this handle's applies run in —
  // 0 the product's kernels; 1 float64 geometry and sums (fp32 vectors); 2 the fixed-point tables' weights, float64 sums
  RadonRefAngle* ref_ang;
  int ref_mode;
  int ref_chunk_fwd, ref_chunk_adj;   // emulated fp32 partial sums of the instrument (0: float64 sums)
  float* ref_tmp;     // max(rows, cols) floats: Op(x) before the half step's combination (ref_mode != 0 only)
};

// Optional epilogue of the kernel that writes an apply's output (trk_op_apply_axpby): out = a * Op(x) + b * z.
struct Epi {
  int on;            // 0: out = Op(x)
  Coef a, b;
  const float* z;    // NULL: out = a * Op(x)
  // a norm the previous fused apply of this operator left as block partials (TRK_HINT_SUMSQ_DEFERRED): coefficients that
  // point at pend_target take the sum of the partials instead, and workgroup 0 stores the finished value there
  double* pend_target;
  const double* pend_part;
  int pend_n;
  // forward only (trk_gk_step_proj): block partials of <out, dotv> next to the fused norm's
  const float* dotv;
  double* dot_part;
  // adjoint only (trk_gk_step_lsqr): the damped-LSQR update whose vk is this epilogue's z
  LsqrReq lq;
  // adjoint only (trk_gk_step_post): a mailbox post carried by workgroup 0
  PostReq pq;
};

// Which forward kernel an input gets (fwd_path, radon_fwd.hip)
struct FwdPath {
  bool lds, win, direct1;
};

// Which adjoint kernel a call gets.  `riders`: the fused epilogue carries the damped-LSQR update or the mailbox post.
//   quad    k_radon_adj_quad by mirrored tile pairs, with its own pre-pass (k_radon_adj_prepq)
//   groups  k_radon_adj_tile<32, 4, 8, *, 4>: the four parts of a split tile in one workgroup
//   tileT*  k_radon_adj_tile<T, PX, AB, *>, split over `nsplit` workgroups per tile
//   simple  k_radon_adj_simple, one pixel per thread (TRK_RADON_ADJ_SIMPLE=1, read per call: the tests switch it; frames below 16^2)
// prep: the records come from k_radon_adj_prep (which a hinted forward may have run already), not from the tile kernel itself.
// blocks: workgroups per frame and split part, one fused-norm partial each.
enum class AdjKind { quad, groups, tile32_b8, tile16_b16, tile16_b4, simple };
struct AdjPath {
  AdjKind kind;
  bool prep;
  int nsplit, tiles_x;
  int64_t blocks;
};

constexpr int HINT_OUT_FEEDS_OPPOSITE = 1, HINT_INPUT_FROM_OPPOSITE = 2, HINT_SUMSQ_DEFERRED = 4;   // = TRK_HINT_* (trk.h)

// the sum of the pending partials — the same bits in every workgroup (one wave, fixed order) — in all threads
__device__ __forceinline__ double pend_total(const Epi& e, double* lds1) {
  if (threadIdx.x < 64) {
    // eight loads in flight per trip, added in the order a one-by-one loop would (the convention of trk_internal.h: every
    // consumer of the same partials gets the same bits); one by one, the 1024 partials of a 512^2 adjoint were 16 dependent
    // L2 round trips at the head of every workgroup of the kernel that follows
    double v = 0.0;
    for (int i = threadIdx.x; i < e.pend_n; i += 512) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = (i + 64 * u < e.pend_n) ? e.pend_part[i + 64 * u] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) v += t[u];
    }
    v = wave_sum_all(v);
    if (threadIdx.x == 0) *lds1 = v;
  }
  __syncthreads();
  return *lds1;
}
// (num_v / den_v: the scalars *k.num / *k.den as fetched BEFORE the pending sum was formed — behind its barrier they were one more
//  exposed round trip at the end of every workgroup of the band reduction and of the adjoint's finishers; a value that is the
//  pending target itself is stale there and not used)
__device__ __forceinline__ double coef_eval_pend(const Coef& k, const double* target, double total, double num_v, double den_v) {
  double v = k.c;
  if (k.num) {
    const double t = (k.num == target) ? total : num_v;
    v *= (k.flags & TRK_SQRT_NUM) ? sqrt(t) : t;
  }
  if (k.den) {
    const double t = (k.den == target) ? total : den_v;
    v /= (k.flags & TRK_SQRT_DEN) ? sqrt(t) : t;
  }
  return v;
}
// both coefficients of the epilogue (uniform over the grid; ends with every thread past a barrier when a norm is pending)
__device__ __forceinline__ void epi_coefs(const Epi& e, bool first_block, double* lds1, float& ca, float& cb, double* total_out = nullptr,
                                          double* cad = nullptr, double* cbd = nullptr) {
  ca = 1.f;
  cb = 0.f;
  double da = 1.0, db = 0.0;
  if (e.on) {
    if (e.pend_target) {
      const double an = e.a.num ? *e.a.num : 0.0, ad = e.a.den ? *e.a.den : 0.0;
      const double bn = (e.z && e.b.num) ? *e.b.num : 0.0, bd = (e.z && e.b.den) ? *e.b.den : 0.0;
      const double total = pend_total(e, lds1);
      if (total_out) *total_out = total;
      da = coef_eval_pend(e.a, e.pend_target, total, an, ad);
      if (e.z) db = coef_eval_pend(e.b, e.pend_target, total, bn, bd);
      if (first_block && threadIdx.x == 0) *e.pend_target = total;
    } else {
      da = coef_eval(e.a);
      if (e.z) db = coef_eval(e.b);
    }
    ca = (float)da;
    cb = (float)db;
  }
  if (cad) *cad = da;
  if (cbd) *cbd = db;
}
// the epilogue's arithmetic: e.on == 2 (default) float64 coefficients and products, one rounding of the result; e.on == 1
// (TRK_RADON_EPI_F32=1) that of trk_axpby — fp32 coefficients, one FMA: the fused half step equals apply + trk_axpby to the bit
__device__ __forceinline__ float epi_combine(int on, float ca, float cb, double cad, double cbd, float o, float z, bool has_z) {
  if (on == 2) return (float)(has_z ? fma(cad, (double)o, cbd * (double)z) : cad * (double)o);
  return has_z ? fmaf(ca, o, cb * z) : ca * o;
}

// Both taps of a forward step come from ONE 8-byte load at (row, floor(q)); out-of-range taps get weight 0.
typedef float f2v __attribute__((ext_vector_type(2)));
typedef unsigned int u2v __attribute__((ext_vector_type(2)));
typedef float f4r __attribute__((ext_vector_type(4)));

// Absolute left-tap column of a step: the fixed-point sum Q knows it mod 256, the fp32 estimate of q (off by far less than a
// column) says which multiple of 256.
__device__ __forceinline__ int radon_abs_col(unsigned Q, float qest) {
  const int ce = (int)floorf(qest);
  const int cm = (int)(Q >> QF);
  return ce + (((cm - ce + 128) & 255) - 128);
}

// ---- host functions that cross files
// radon_adj.hip: which adjoint kernel a call gets
AdjPath adj_path(const RadonImpl* im, int batch, bool riders);
// radon_fwd.hip: the forward of one vector — transposed copy if a kernel needs one, the plan of the quad kernels, the launches, the
// band reduction with the epilogue `epi` / the norm partials `ssq_part` / (want_rec) the records of the adjoint that follows
int radon_forward(RadonImpl* im, const float* xb, float* yb, int hints, bool post, bool want_rec, const Epi& epi, double* ssq_part,
                  int64_t post_blocks, hipStream_t s);
// radon_adj.hip: the adjoint of one vector — record pre-pass, the split-tile buffers, the gather kernel `ap` names
int radon_adjoint(RadonImpl* im, const AdjPath& ap, const float* xb, float* yb, int hints, int batch, const Epi& epi, double* ssq_part,
                  hipStream_t s);

}  // namespace radon
}  // namespace trk
