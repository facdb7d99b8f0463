// radon_adj.hip — adjoint kernels of the parallel-beam projector (radon2d.hip: geometry, tables, the apply's bookkeeping) and their
// dispatch.  Gather form, no atomics: per pixel and angle the nearest ray and its two neighbours, from 16-byte records staged in LDS.
#include "radon_internal.h"

#include <cstdlib>

using namespace trk;
using namespace trk::radon;

namespace {

// ---------------------------------------------------------------------------------------- adjoint (gather)
// The forward weights of ray d on its two taps are (1-f, f) with f = q - floor(q), i.e. hat(q - col) = max(0, 1 - |q - col|) on
// pixel `col`.  Per pixel and angle the gather takes the ray d0 nearest to the pixel's inverse image d* (fp32 estimate) and
// its two neighbours — every ray with |q - col| < 1 is among them because |dq/dd| = 1/|cos| >= 1:
//   * t0 = q(d0, tt) - col comes from the SAME tables as the forward, as an integer: t_int = A32[d0] + B32[tt] - (col << 24)
//     (mod 2^32, |t0| <= 0.71 + the estimate's error), so hat(t0) = 1 - |t_int| 2^-24 is bit-identical to the forward's weight;
//   * the neighbours sit at t0 +- |inv| >= 1 away on either side, so their weights are clamp(c1 + t0) and clamp(c1 - t0),
//     c1 = 1 - |inv| <= 0: ONE packed FMA with the hardware clamp to [0, 1] (one fp32 rounding, 6e-8).
// What is read per pixel and angle is ONE 16-byte record {w S[d0 -], w S[d0 +], w S[d0], A32[d0]} (w = the angle's weight;
// -/+: the neighbour on the smaller-q / larger-q side, which is d0 -+ 1 or d0 +- 1 by the sign of inv), written per apply by
// k_radon_adj_prep for the angles sorted by marching mode.
//
// k_radon_adj_tile: a workgroup owns a T x T pixel tile and walks the angles in batches of AB (8 or 16).  Per batch it stages,
// with direct-to-LDS loads, (i) for every angle the 64 records around the tile's inverse image, as a RING indexed by d0 & 63
// (the tile's footprint is < 48 detectors, so no index arithmetic beyond a mask is needed to read a record), and (ii) the
// pairs {C[a][tt], B32[a][tt]} of the tile's marching indices (C: the locator offset, d* = col rinv + C).  A thread holds
// PX pixels that share the marching index — a run along the row for mode-0 angles, along the column for mode-1 angles — so
// that pair is read once per angle and thread; the two partial images meet through LDS at the end.  Per pixel and angle:
// 9.5 vector instructions and one ds_read_b128 — d* (packed FMA for two pixels), its rounding (a packed add of 1.5 x 2^23:
// the integer sits in the low mantissa bits), ring address (and, shift-add), t_int (one three-operand add), its conversion,
// the centre weight (one FMA), both neighbour weights (one packed FMA with clamp), two accumulating FMAs (one packed).  The
// kernel is bound by vector-instruction issue (4 cycles per wave instruction): the first gather form of round 1 needed 34
// instructions and three dword loads on the texture path, the second 26 and one 12-byte load, this kernel's first version 15.
constexpr float RND_MAGIC = 12582912.0f;   // 1.5 * 2^23: x + RND_MAGIC has rint(x) in its low mantissa bits (|x| < 2^22)

// records of one vector: rec[(frame*na + sorted angle)][e], e = d + 2 in [0, nd + 3]
__global__ __launch_bounds__(256) void k_radon_adj_prep(const float* __restrict__ sino, uint4* __restrict__ rec, int nd, int na,
                                                        const AdjAngle* __restrict__ ang, const float* __restrict__ wgt,
                                                        const unsigned* __restrict__ A32) {
  const int ndp = nd + 2 * A32_PAD;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;      // over (sorted angle of the frame) x ndp; blockIdx.y = frame
  const int64_t r = idx / ndp;
  if (r >= (int64_t)na) return;
  const int e = (int)(idx - r * ndp);
  const int64_t rs = (int64_t)blockIdx.y * na + r;                   // sorted row (frame-major)
  const int64_t ro = (int64_t)blockIdx.y * na + ang[rs].orig;        // the same angle in the caller's order
  const int d = e - A32_PAD;
  const float w = wgt[rs];
  const float* __restrict__ S = sino + ro * nd;
  const float sm = (d - 1 >= 0 && d - 1 < nd) ? w * S[d - 1] : 0.f, sp = (d + 1 >= 0 && d + 1 < nd) ? w * S[d + 1] : 0.f;
  const bool flip = ang[rs].flip != 0;
  uint4 o;
  o.x = __builtin_bit_cast(unsigned, flip ? sp : sm);             // the neighbour at t0 - |inv|
  o.y = __builtin_bit_cast(unsigned, flip ? sm : sp);             // the neighbour at t0 + |inv|
  o.z = __builtin_bit_cast(unsigned, (d >= 0 && d < nd) ? w * S[d] : 0.f);
  o.w = A32[ro * ndp + e];
  rec[rs * ndp + e] = o;
}

// LDS by byte offset: the ring slot of detector d0 is (d0 & 63) * 16 behind the ring's base, which is one v_and_b32 and one
// v_lshl_add_u32 with the (wave-uniform) base in an SGPR — spelled out, or the optimiser turns it into shift + mask + add
__device__ __forceinline__ unsigned lds_offset(const void* p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const void*)p;
}
typedef unsigned u4r __attribute__((ext_vector_type(4)));     // a record {w S[d0 -], w S[d0 +], w S[d0], A32[d0]}
// The read is issued as inline assembly: written as a C++ load, the compiler orders it after EVERY outstanding direct-to-LDS
// load (it cannot see that the prefetch of batch b + 1 lands in the other ring buffer) and put s_waitcnt vmcnt(0) in front of each
// record read — the prefetch issued a few instructions earlier was waited for before the gather of batch b began, twelve exposed
// L2 round trips per tile at 512^2 x 180.  The counterpart of hiding the read: the CALLER waits (ring_wait) before using r.
__device__ __forceinline__ u4r ring_read(unsigned ring_base, unsigned bits) {
  unsigned addr;
  const unsigned slot = bits & 63u;
  asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(addr) : "v"(slot), "s"(ring_base));
  u4r r;
  asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(addr) : "memory");
  return r;
}
// a {C, B32} pair by inline assembly, for the same reason (a C++ LDS load in the angle loop was given `s_waitcnt vmcnt(0)`: the wait
// for the NEXT batch's direct-to-LDS loads).  The caller waits (ring_wait) and ties (pair_tie) before using OR COPYING it: the data
// lands after the instruction has issued, so nothing may touch the destination registers in between — no conditional assignment
// (a join would copy them), no element-wise repacking
typedef unsigned u2r __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u2r pair_read(const void* p) {
  u2r r;
  asm volatile("ds_read_b64 %0, %1" : "=v"(r) : "v"(lds_offset(p)) : "memory");
  return r;
}
__device__ __forceinline__ void pair_tie(u2r& r) { asm volatile("" : "+v"(r)); }
// all of this wave's LDS reads have returned; ring_tie makes a record's uses depend on the wait (volatile asm keeps its order)
__device__ __forceinline__ void ring_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void ring_tie(u4r& r) { asm volatile("" : "+v"(r)); }

// one pixel, one angle: the record, t0 from the tables, three hat weights.  accn: the two neighbour terms (packed), acc0: the centre
__device__ __forceinline__ void adj_gather(const u4r r, unsigned B, unsigned negcol24, f2v sc2, float nsc, f2v cr, f2v& accn,
                                           float& acc0) {
  // NOTE the elements are copied to scalars first: __builtin_bit_cast(float, r[k]) on an ext-vector ELEMENT reads element 0
  // whatever k is (hipcc / ROCm 7.2; found the hard way — the adjoint summed (w0 + wp + wm) S[d0-1])
  const unsigned slo = r[0], shi = r[1], s0 = r[2], a32 = r[3];
  unsigned ti;                                                   // t_int = A32 + B32 - (col << 24), wrap-around mod 2^32 is the point
  asm("v_add3_u32 %0, %1, %2, %3" : "=v"(ti) : "v"(a32), "v"(B), "v"(negcol24));
  const float tf = (float)(int)ti;                               // t0 in units of 2^-24, exact
  // {clamp(c1m + t0), clamp(c1p - t0)} in one packed FMA: both lanes read the LOW half of t2 and of the scale (op_sel_hi 0), each its own half of the addend; the high
  // lane negates the scale 2^-24.  64-bit operands must sit in even-aligned register pairs, hence the two-element carriers
  // whose high halves are never read.  The one scalar operand an instruction may have is the angle's {c1, rinv} pair as it came
  // from the scalar load (the scale, loop-invariant, lives in a vector pair): with c1 as the vector operand every angle paid a
  // v_mov to get it there, one of its eleven vector instructions.
  f2v t2;
  t2[0] = tf;
  f2v wn;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,0,1] neg_hi:[0,1,0] clamp" : "=v"(wn) : "v"(t2), "v"(sc2), "s"(cr));
  float w0;                                                      // 1 - |t0|: exact (t0 is a multiple of 2^-24)
  asm("v_fma_f32 %0, |%1|, %2, 1.0" : "=v"(w0) : "v"(tf), "s"(nsc));
  const f2v sn = {__builtin_bit_cast(float, slo), __builtin_bit_cast(float, shi)};
  accn = __builtin_elementwise_fma(wn, sn, accn);
  acc0 = fmaf(w0, __builtin_bit_cast(float, s0), acc0);
}

// G > 1 (round 5; a 512^2 image: 256 tiles = one per CU): the parts of a tile are G groups of four waves of ONE workgroup of 1024 threads —
// the same angle ranges, the same batches, their own rings — whose partial tiles meet in LDS in part order: the same bits as the
// split over workgroups, without write-through partial tiles, tickets and a finisher that starts when everybody else is done.
template <int T, int PX, int AB, bool PREP, int G = 1>
__global__ __launch_bounds__(256 * G) void k_radon_adj_tile(const float* __restrict__ sino, const uint4* __restrict__ rec,
                                                        float* __restrict__ img, int N, int nd, int na,
                                                        const AdjAngle* __restrict__ ang, const float* __restrict__ wgt,
                                                        const unsigned* __restrict__ A32, const int* __restrict__ n_mode0,
                                                        const uint2* __restrict__ CB, int npad, int tiles_x,
                                                        double* __restrict__ ssq_part, Epi epi, float* __restrict__ xT_out,
                                                        int nsplit, float* __restrict__ part_img, unsigned* __restrict__ tile_cnt) {
  __shared__ __attribute__((aligned(16))) uint4 ring_all[G][2][AB][64];
  __shared__ __attribute__((aligned(16))) uint2 cbs_all[G][2][AB][T];
  __shared__ double xch_all[G][PX > 1 ? T : 1][T + 1];     // (float64 since round 6: the two modes' totals meet unrounded)
  static_assert(T * T == 256 * PX && (T == 16 || T == 32), "256 threads x PX pixels cover the T x T tile");
  static_assert(G == 1 || (PX == 4 && T == 32), "groups: the 32 x 32 form only");
  __shared__ double lds[4];
  const int tid = G > 1 ? (int)(threadIdx.x & 255) : (int)threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = G > 1 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8)) : 0;
  auto& ring = ring_all[grp];
  auto& cbs = cbs_all[grp];
  auto& xch = xch_all[grp];
  const int frame = blockIdx.y;
  // nsplit > 1 (small images: too few tiles to fill the chip with 32 x 32 tiles): workgroup (part, tile) gathers the sorted
  // angles [a_lo, a_hi) of the frame for its tile; the partial tiles meet in the workgroup that finishes LAST (below).  Parts of
  // one tile are ntiles workgroups apart: the same XCD when ntiles % 8 == 0 (speed only)
  const int ntiles = tiles_x * tiles_x;
  if (G > 1) nsplit = G;
  const int part = G > 1 ? grp : (nsplit > 1 ? blockIdx.x / ntiles : 0);
  const int tile_id = G > 1 ? (int)blockIdx.x : (int)blockIdx.x - part * ntiles;
  const int ty = tile_id / tiles_x, tx = tile_id - ty * tiles_x;
  const int i0 = ty * T, j0 = tx * T;
  const int ndp = nd + 2 * A32_PAD;
  const int a_lo = nsplit > 1 ? (int)(((int64_t)part * na) / nsplit) : 0;
  const int a_hi = nsplit > 1 ? (int)(((int64_t)(part + 1) * na) / nsplit) : na;
  sino += (int64_t)frame * na * nd;
  A32 += (int64_t)frame * na * ndp;
  CB += (int64_t)frame * na * npad;
  int n0 = n_mode0[frame] - a_lo;
  ang += (int64_t)frame * na + a_lo;                   // from here on `na` is the part's angle count and angle 0 its first
  wgt += (int64_t)frame * na + a_lo;
  rec += ((int64_t)frame * na + a_lo) * ndp;
  const int na_frame = na;
  na = a_hi - a_lo;
  n0 = n0 < 0 ? 0 : (n0 > na ? na : n0);
  const auto rrec = __builtin_amdgcn_make_buffer_rsrc((void*)rec, 0, (unsigned)((int64_t)na * ndp * 16), 0x00020000);
  const float sdh = 0.5f * (float)(nd - 1);
  const auto rcb = __builtin_amdgcn_make_buffer_rsrc((void*)CB, 0, (unsigned)((int64_t)na_frame * npad * 8), 0x00020000);

  // thread -> pixels.  mode 0 (marching index = row): row r0, columns c0 + k T/PX;  mode 1 (= column): column c1, rows
  // r1 + k T/PX, k < PX (PX = 1: the same pixel in both).  Neighbouring lanes hold NEIGHBOURING pixels, so the 16 lanes of a
  // ds_read_b128 group read records at most ~10 detectors apart: distinct LDS banks (a record is 4 banks wide, 16 records fill
  // the 64) or the same record (a broadcast).  With 4 consecutive pixels per lane instead, neighbouring lanes were up to 4
  // detectors apart and 35 % of the LDS cycles were bank conflicts (PMC).
  constexpr int TS = T / PX;                           // threads along the run direction = pixel stride of one thread
  const int r0 = tid / TS, c0 = tid % TS;
  const int r1 = PX > 1 ? tid % TS : tid / T, c1 = PX > 1 ? tid / TS : tid % T;   // (mode 1: neighbouring lanes = neighbouring ROWS)
  float fcolA[PX], fcolB[PX];
  unsigned colA[PX], colB[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    fcolA[k] = (float)(j0 + c0 + k * TS);            // mode 0: interpolated coordinate = column
    colA[k] = 0u - ((unsigned)(j0 + c0 + k * TS) << QF);   // negated: t_int = A32 + B32 - (col << 24)
    fcolB[k] = (float)(i0 + r1 + k * TS);            // mode 1: interpolated coordinate = row
    colB[k] = 0u - ((unsigned)(i0 + r1 + k * TS) << QF);
  }
  f2v anA[PX], anB[PX];
  float accA[PX], accB[PX];
  // fp32 sums over at most ADJ_FLUSH angles, then float64 (round 6; rounds 1-5: fp32 over all angles of the part).  The float64
  // instrument (profiles/r05/c3_instrument.txt) put the 180-angle fp32 sum one amplification step (x 6.5 per iteration of C3's
  // transient) above the fp32-storage floor, a 32-angle cadence on it (R.set_ref_sums(4, 32))
  constexpr int ADJ_FLUSH = 32;
  double totA[PX], totB[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    accA[k] = accB[k] = 0.f;
    anA[k] = anB[k] = (f2v){0.f, 0.f};
    totA[k] = totB[k] = 0.0;
  }
  f2v sc2 = {5.9604644775390625e-8f, 5.9604644775390625e-8f};          // 2^-24, kept in an (aligned) VGPR pair
  float nsc = -5.9604644775390625e-8f;
  asm("" : "+v"(sc2));
  asm("" : "+s"(nsc));

  const int nbatch = (na + AB - 1) / AB;
  // groups: every group meets every barrier — the batches of the LARGEST part (a part may hold one angle more than another)
  int nbatch_all = nbatch;
  if (G > 1) {
    nbatch_all = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int sz = (int)(((int64_t)(g + 1) * na_frame) / G) - (int)(((int64_t)g * na_frame) / G);
      nbatch_all = (sz + AB - 1) / AB > nbatch_all ? (sz + AB - 1) / AB : nbatch_all;
    }
  }
  // Staging of batch b into buffer b & 1: wave w takes the rings of angles w, w + 4, ... of the batch, lane l the detector whose
  // ring slot is l.  PREP: the records {w S[d -], w S[d +], w S[d], A32[d]} were written by k_radon_adj_prep and go straight
  // to LDS (one 16-byte direct-to-LDS load per lane and angle).  !PREP: they are made here from the sinogram itself — four
  // dwords per lane into registers while the previous batch is gathered, written to LDS afterwards — which saves the pre-pass
  // launch and pays when a frame has few angles (dynamic problems, 15 per frame: 32 frames 21.0 -> 20.0 us, 4 frames 11.0 ->
  // 8.4 us) but costs more instructions per record (180 angles: 512^2 46 -> 57 us, 4096^2 1.04 -> 1.32 ms).
  // The {C, B32} pairs of the tile's marching indices always go straight to LDS (16 bytes = two indices per thread).
  uint4 sreg[AB / 4];
  int cb_orig = 0;
  if (tid < AB * T / 2) {
    const int a = tid / (T / 2);
    cb_orig = ang[a < na ? a : na - 1].orig;
  }
  // lane l holds {rinv, dq, k0} of angle l (mod AB) of the batch stage_load is called for next, fetched a batch ahead
  float nx_rinv, nx_dq, nx_k0;
  auto fetch_angles = [&](int b) {
    int a = b * AB + (lane & (AB - 1));
    a = a < na ? a : na - 1;
    nx_rinv = ang[a].rinv;
    nx_dq = ang[a].dq;
    nx_k0 = ang[a].k0;
  };
  fetch_angles(0);
  int nam1;                                          // na - 1 as a value the vector unit has no copy of, so that the row
  asm("s_add_i32 %0, %1, -1" : "=s"(nam1) : "s"(na) : "scc");   // offsets below stay scalar arithmetic
  auto stage_load = [&](int b) {
    // inverse image of the tile: d* = col rinv + (sdh - (k0 + tt dq) rinv) is linear, so the tile's d* are centred on the
    // image of its centre and span at most (T - 1) sqrt(2) detectors (22 / 44 for T = 16 / 32): a 64-slot ring around the centre
    // holds them and their +-1 neighbours.  The ring bases of the batch's AB angles are computed by AB LANES, one angle each, and
    // handed out by v_readlane: the arithmetic is wave-uniform per angle but gfx950 has no scalar float unit — done per ring
    // (first from the four corners, 35 vector instructions per ring, then from the centre, 20) staging was 43 % / 30 % of the
    // 16 x 16 kernel's vector instructions at 512^2 x 180 (PMC).
    int dbase_l;
    {
      int a = b * AB + (lane & (AB - 1));
      a = a < na ? a : na - 1;
      const bool m1 = a >= n0;
      const float tt_c = (float)(m1 ? j0 : i0) + 0.5f * (float)(T - 1), co_c = (float)(m1 ? i0 : j0) + 0.5f * (float)(T - 1);
      dbase_l = (int)floorf(fmaf(co_c - fmaf(tt_c, nx_dq, nx_k0), nx_rinv, sdh)) - 32;
    }
    if (b + 1 < nbatch) fetch_angles(b + 1);
#pragma unroll
    for (int h = 0; h < AB / 4; ++h) {
      const int al = wv + 4 * h;
      int a;
      asm("s_min_i32 %0, %1, %2" : "=s"(a) : "s"(b * AB + al), "s"(nam1) : "scc");
      const int row = a * ndp;
      const int dbase = __builtin_amdgcn_readlane(dbase_l, al);      // ring covers dbase .. dbase + 63
      const int d = dbase + ((lane - dbase) & 63);                   // the detector whose ring slot is this lane
      int e;                                                         // beyond the detector: weightless (S = 0) anyway
      asm("v_med3_i32 %0, %1, 0, %2" : "=v"(e) : "v"(d + A32_PAD), "s"(ndp - 1));
      if (PREP) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rrec, (__attribute__((address_space(3))) void*)&ring[b & 1][al][0], 16,
                                                 (row + e) * 16, 0, 0, 0);
        continue;
      }
      const AdjAngle p = ang[a];
      const float* __restrict__ S = sino + (int64_t)p.orig * nd;
      const float w = wgt[a];
      const int dm = d - 1, dp = d + 1;
      const float sm = ((unsigned)dm < (unsigned)nd) ? w * S[dm] : 0.f;
      const float s0 = ((unsigned)d < (unsigned)nd) ? w * S[d] : 0.f;
      const float sp = ((unsigned)dp < (unsigned)nd) ? w * S[dp] : 0.f;
      sreg[h].x = __builtin_bit_cast(unsigned, p.flip ? sp : sm);    // the neighbour at t0 - |inv|
      sreg[h].y = __builtin_bit_cast(unsigned, p.flip ? sm : sp);    // the neighbour at t0 + |inv|
      sreg[h].z = __builtin_bit_cast(unsigned, s0);
      sreg[h].w = A32[(int64_t)p.orig * ndp + e];
    }
    if (tid < AB * T / 2) {
      const int buf = b & 1;
      const int al = tid / (T / 2), pr = tid - al * (T / 2);
      int a = b * AB + al;
      a = a < na ? a : na - 1;
      const int tt0 = (a >= n0 ? j0 : i0) + 2 * pr;                  // even: 16-byte aligned pairs (npad is even)
      // (the LDS address of a direct-to-LDS load is wave-uniform base + 16 * lane: wave 1 lands 1 KB behind wave 0)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rcb, (__attribute__((address_space(3))) void*)(reinterpret_cast<char*>(&cbs[buf][0][0]) + wv * 1024),
                                               16, (cb_orig * npad + tt0) * 8, 0, 0, 0);
      // the table row of this thread's pair in the batch after: fetched a batch ahead — read here, the load and the vmcnt(0) its
      // use needs sat between the ring loads and the gather, one exposed L2 round trip per batch for waves 0 and 1
      int an = (b + 1) * AB + al;
      an = an < na ? an : na - 1;
      cb_orig = ang[an].orig;
    }
  };
  auto stage_store = [&](int b) {
    if (PREP) return;
#pragma unroll
    for (int h = 0; h < AB / 4; ++h) ring[b & 1][wv + 4 * h][lane] = sreg[h];
  };

  stage_load(0);
  stage_store(0);
  for (int b = 0; b < nbatch_all; ++b) {
    const int buf = b & 1;
    __builtin_amdgcn_s_waitcnt(0x0F70);              // vmcnt(0): this wave's share of batch b has landed
    __syncthreads();                                 // batch b complete; everyone is done with the other buffer
    if (G > 1 && b >= nbatch) continue;              // (a smaller part of the workgroup: only the barrier)
    if (b + 1 < nbatch) stage_load(b + 1);           // in flight while batch b is gathered
    const int nal = (na - b * AB < AB) ? na - b * AB : AB;
    // the batch's mode-0 angles come first (the angles are sorted by mode): two loops without a mode test inside, unrolled so
    // that the LDS reads of several angles are in flight together (small images run few waves per SIMD: latency, not issue)
    const int a0 = b * AB;
    const int nm0 = (n0 - a0 < 0) ? 0 : (n0 - a0 < nal ? n0 - a0 : nal);
    const unsigned rbase0 = __builtin_amdgcn_readfirstlane(lds_offset(&ring[buf][0][0]));
    // One pixel per thread (16 x 16 tiles): FOUR angles per trip, written so that their four {C, B32} reads and then their four
    // record reads are in flight together.  Angle by angle the compiler waited for each LDS read before the next (the requested
    // unrolling was not done): two exposed LDS round trips per angle and wave, which four waves per SIMD cannot cover — at
    // 512^2 x 180 the kernel was latency-bound at 36 us with 12 vector instructions per angle, 16 M in all (PMC).
    auto angles = [&](int al_lo, int al_hi, const float* fcol, const unsigned* ncol, int cbrow, f2v* an, float* ac) {
      int al = al_lo;
      if (PX == 1) {
        for (; al + 4 <= al_hi; al += 4) {
          AdjAngle p[4];
          uint2 cb[4];
          u4r rr[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) p[u] = ang[a0 + al + u];
#pragma unroll
          for (int u = 0; u < 4; ++u) cb[u] = cbs[buf][al + u][cbrow];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const unsigned bits = __builtin_bit_cast(unsigned, fmaf(fcol[0], p[u].rinv, __builtin_bit_cast(float, cb[u].x)) + RND_MAGIC);
            rr[u] = ring_read(rbase0 + (al + u) * 1024, bits);
          }
          ring_wait();
#pragma unroll
          for (int u = 0; u < 4; ++u) ring_tie(rr[u]);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            f2v cr = {p[u].c1m, p[u].c1p};           // the packed clamp-FMA takes its addend from this scalar pair
            asm("" : "+s"(cr));
            adj_gather(rr[u], cb[u].y, ncol[0], sc2, nsc, cr, an[0], ac[0]);
          }
        }
      }
      // (round 6) the NEXT angle's constants and {C, B32} pair are requested right behind this angle's record reads, so that one wait
      // covers both: angle by angle the loop had two exposed round trips (scalar + LDS for the pair, then LDS for the records)
      if (al < al_hi) {
        float pn_c1 = ang[a0 + al].c1m, pn_c1p = ang[a0 + al].c1p, pn_rinv = ang[a0 + al].rinv;     // wave-uniform: scalar loads
        u2r cbn = pair_read(&cbs[buf][al][cbrow]);
        ring_wait();
        pair_tie(cbn);
#pragma unroll 2
        for (; al < al_hi; ++al) {
          const float p_rinv = pn_rinv;
          f2v cr = {pn_c1, pn_c1p};
          asm("" : "+s"(cr));
          const u2r cbv = cbn;                       // (a copy made AFTER the tie)
          const float C = __builtin_bit_cast(float, (unsigned)cbv[0]);
          const unsigned cb_y = cbv[1];
          u4r rr[PX];
#pragma unroll
          for (int k = 0; k < PX; ++k) {
            const unsigned bits = __builtin_bit_cast(unsigned, fmaf(fcol[k], p_rinv, C) + RND_MAGIC);
            rr[k] = ring_read(rbase0 + al * 1024, bits);
          }
          const int aln = al + 1 < al_hi ? al + 1 : al;      // (the last angle re-reads itself: unconditional, no join)
          pn_c1 = ang[a0 + aln].c1m;
          pn_c1p = ang[a0 + aln].c1p;
          pn_rinv = ang[a0 + aln].rinv;
          cbn = pair_read(&cbs[buf][aln][cbrow]);
          ring_wait();
          pair_tie(cbn);
#pragma unroll
          for (int k = 0; k < PX; ++k) {
            ring_tie(rr[k]);
            adj_gather(rr[k], cb_y, ncol[k], sc2, nsc, cr, an[k], ac[k]);
          }
        }
      }
    };
    angles(0, nm0, fcolA, colA, r0, anA, accA);
    angles(nm0, nal, fcolB, colB, c1, anB, accB);
    if (((b + 1) * AB) % ADJ_FLUSH == 0) {           // wave-uniform; only the batch where the modes change flushes both
      if (nm0 > 0) {
#pragma unroll
        for (int k = 0; k < PX; ++k) {
          totA[k] += (double)(accA[k] + (anA[k][0] + anA[k][1]));
          accA[k] = 0.f;
          anA[k] = (f2v){0.f, 0.f};
        }
      }
      if (nm0 < nal) {
#pragma unroll
        for (int k = 0; k < PX; ++k) {
          totB[k] += (double)(accB[k] + (anB[k][0] + anB[k][1]));
          accB[k] = 0.f;
          anB[k] = (f2v){0.f, 0.f};
        }
      }
    }
    if (b + 1 < nbatch) stage_store(b + 1);          // the other buffer: nobody reads it before the next barrier
  }
  // the two partial images meet: mode-0 sums go through LDS to the thread that holds the pixel in the mode-1 layout
  if (PX > 1) {
#pragma unroll
    for (int k = 0; k < PX; ++k) xch[r0][c0 + k * TS] = totA[k] + (double)(accA[k] + (anA[k][0] + anA[k][1]));
    __syncthreads();
  }
  float oraw[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k)
    oraw[k] = (float)((totB[k] + (double)(accB[k] + (anB[k][0] + anB[k][1]))) +
                      (PX > 1 ? xch[r1 + k * TS][c1] : totA[k] + (double)(accA[k] + (anA[k][0] + anA[k][1]))));
  if (G > 1) {
    // the groups' partial tiles meet in LDS, added in part order by the first group, which carries the epilogue alone
    __shared__ float red[G > 1 ? G - 1 : 1][256][PX];
    if (grp > 0) {
#pragma unroll
      for (int k = 0; k < PX; ++k) red[grp - 1][tid][k] = oraw[k];
    }
    __syncthreads();
    if (grp > 0) return;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      float t = oraw[k];
#pragma unroll
      for (int s = 1; s < G; ++s) t += red[s - 1][tid][k];
      oraw[k] = t;
    }
  } else if (PX == 4 && nsplit > 1) {                              // (the host splits only the 32 x 32 form)
    // The parts of a tile meet: every workgroup leaves its partial tile (thread-major, 16 bytes per lane), then takes a ticket; the
    // one that draws the LAST ticket adds the partial tiles in part order (the same bits whoever comes last) and carries the
    // epilogue.  The parts may have run on different XCDs, whose L2s are not coherent: the bytes are stored WRITE-THROUGH (sc1) and
    // loaded past the L1 (sc1), every storing wave drains its stores before the workgroup's one ticket (an agent-scope atomic add),
    // and the loads are issued only after the add has returned and the workgroup has met (MI355X_MICROARCH.md, inter-workgroup
    // visibility: the "workgroup whose add came last" hand-off).  A release / acquire fence pair per workgroup instead
    // (__threadfence) writes back and invalidates whole caches: 512^2 x 180 ran 130 us instead of 33.
    constexpr int MAXSPLIT = 8;
    const int64_t pstride = (int64_t)gridDim.y * ntiles * (T * T);
    float* P = part_img + ((int64_t)frame * ntiles + tile_id) * (T * T) + tid * PX;     // (not __restrict__: the other parts write it too)
    {
      f4r v = {oraw[0], oraw[PX > 1 ? 1 : 0], oraw[PX > 2 ? 2 : 0], oraw[PX > 3 ? 3 : 0]};
      asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(P + part * pstride), "v"(v) : "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ unsigned ticket;
    unsigned* cnt = tile_cnt + (int64_t)frame * ntiles + tile_id;
    if (tid == 0) ticket = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (ticket != (unsigned)(nsplit - 1)) return;
    if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // for the next launch
    f4r pv[MAXSPLIT];
#pragma unroll
    for (int s = 0; s < MAXSPLIT; ++s) {
      // straight-line code (parts beyond nsplit re-read part 0 and are not added): a branch around an inline-assembly load would
      // let the compiler copy its destination at the join, before the data has arrived
      const float* src = P + (s < nsplit ? s : 0) * pstride;
      asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(pv[s]) : "v"(src) : "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < MAXSPLIT; ++s) asm volatile("" : "+v"(pv[s]));
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      float t = pv[0][k];
#pragma unroll
      for (int s = 1; s < MAXSPLIT; ++s) t = s < nsplit ? t + pv[s][k] : t;
      oraw[k] = t;
    }
  }
  const bool lead = tile_id == 0 && blockIdx.y == 0;               // the workgroup that carries the once-per-launch duties
  double q = 0.0;
  img += (int64_t)frame * N * N;
  // epilogue (trk_op_apply_axpby): out = a * (A^T s) + b * z; xT_out: also the transposed image the next forward apply wants
  // (measured at 512^2: fetching z and the coefficients before the angle loop instead costs 1.6 us — registers)
  float zv[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int i = i0 + r1 + k * TS, j = j0 + c1;
    zv[k] = (epi.on && epi.z && i < N && j < N) ? epi.z[((int64_t)frame * N + i) * N + j] : 0.f;
  }
  // (the operands of the rider below: requested here, so that they travel while the coefficients are worked out)
  float lw[PX], lx[PX], lr[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int i = i0 + r1 + k * TS, j = j0 + c1;
    const bool in = epi.lq.on && i < N && j < N;
    const int64_t g = ((int64_t)frame * N + i) * N + j;
    lw[k] = (in && !epi.lq.first) ? epi.lq.w[g] : 0.f;
    lx[k] = (in && epi.lq.x_in) ? epi.lq.x_in[g] : 0.f;
    lr[k] = (in && epi.lq.ref) ? epi.lq.ref[g] : 0.f;
  }
  float ca, cb;
  double pend_sum = 0.0, cad, cbd;
  epi_coefs(epi, lead, &lds[0], ca, cb, &pend_sum, &cad, &cbd);
  if (xT_out) xT_out += (int64_t)frame * N * N;
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int i = i0 + r1 + k * TS, j = j0 + c1;
    float o = oraw[k];
    if (i < N && j < N) {
      if (epi.on) o = epi_combine(epi.on, ca, cb, cad, cbd, o, zv[k], epi.z != nullptr);
      img[(int64_t)i * N + j] = o;
      if (xT_out) xT_out[(int64_t)j * N + i] = o;
      q += (double)o * o;
    }
  }
  if (ssq_part) {                                                 // uniform over the grid
    q = block_sum<256>(q, lds);
    if (tid == 0) ssq_part[(size_t)blockIdx.y * ntiles + tile_id] = q;
  }
  if (epi.pq.on && lead && tid < 64) {
    // the mailbox post of the step before (k_mailbox_post / k_mailbox_post_sum, core.hip): its scalars are final here — the
    // deferred one is `pend_sum`, which this workgroup has just stored — and the host polls the sequence word
    const PostReq& Q = epi.pq;
    double sum = 0.0;
    if (Q.part) sum = scalar_from_wave(ScalarSrc{Q.part, Q.n_part}, tid);
    if (tid == 0) {
      for (int c = 0; c < Q.count; ++c) {
        const double* sp = Q.src + c;
        Q.dst[c] = (epi.pend_target && sp == epi.pend_target) ? pend_sum : *sp;
      }
      if (Q.part) {
        *Q.sum_dev = sum;
        *Q.sum_host = sum;
      }
      __threadfence_system();
      __hip_atomic_store(Q.seq, Q.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  if (epi.lq.on) {                                                // uniform over the grid
    // the damped-LSQR step of the iterate that z = V[k-1] belongs to, on this workgroup's pixels: k_lsqr_damped_update's
    // arithmetic, expression for expression (gemv.hip) — the same floats whichever kernel forms them
    const LsqrReq& L = epi.lq;
    __shared__ double lcf[3];
    __syncthreads();
    if (tid == 0) {
      const double b2v = (epi.pend_target && epi.pend_target == L.b2) ? pend_sum : *L.b2;
      const double alpha = sqrt(*L.a2), beta = sqrt(b2v);
      double rhobar, phibar, tw = 0.0;
      if (L.first) {
        rhobar = alpha;
        phibar = sqrt(*L.beta0_sq);
      } else {
        rhobar = -L.st_in[0] * alpha;
        tw = L.st_in[1] * alpha / L.st_in[2];
        phibar = L.st_in[3];
      }
      const double rhobar1 = sqrt(rhobar * rhobar + L.damp * L.damp);
      phibar *= rhobar / rhobar1;
      const double rho = sqrt(rhobar1 * rhobar1 + beta * beta);
      const double cs = rhobar1 / rho, sn = beta / rho;
      lcf[0] = 1.0 / alpha;
      lcf[1] = tw;
      lcf[2] = cs * phibar / rho;
      if (lead) {
        L.st_out[0] = cs;
        L.st_out[1] = sn;
        L.st_out[2] = rho;
        L.st_out[3] = sn * phibar;
      }
    }
    __syncthreads();
    const double ia = lcf[0], tw = lcf[1], px = lcf[2];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int i = i0 + r1 + k * TS, j = j0 + c1;
      if (i < N && j < N) {
        const int64_t g = ((int64_t)frame * N + i) * N + j;
        const float wo = lw[k], xo = lx[k];
        const float wn = (float)(ia * (double)zv[k] - (L.first ? 0.0 : tw * (double)wo));
        const float xn = (float)((L.x_in ? (double)xo : 0.0) + px * (double)wn);
        L.w[g] = wn;
        L.x_out[g] = xn;
        if (L.ref) {
          const double e = (double)xn - lr[k];
          acc += e * e;
        }
      }
    }
    if (L.ref) {
      acc = block_sum<256>(acc, lds);
      if (tid == 0) L.err_part[(size_t)blockIdx.y * ntiles + tile_id] = acc;
    }
  }
}

// ---------------------------------------------------------------------------------------- adjoint by mirrored tile pairs (round 6)
// The symmetry that carries the forward's quads (k_radon_fwd_quad) applied to the adjoint.  With the BASE geometry of a quad — beta in
// [0, 45 deg], q_b(d, tt) = (A_b[d] + B_b[tt]) 2^-24 — one evaluation of {nearest base detector d0, t0 = q_b(d0, tt) - col, the three hat
// weights} at (tt, col) serves
//     slot 0 (rows of x):            pixel (tt, col)            slot 1 (rows of x, mirrored):  pixel (tt, N-1-col)
//     slot 2 (rows of x^T):          pixel (col, tt)            slot 3 (rows of x^T, mirrored): pixel (N-1-col, tt)
// each with ITS member's sinogram values at the base detectors d0 - 1, d0, d0 + 1 (a mirrored member sees t = -t0: the hat is even; a
// flipped member's detector index runs the other way: the record array recq is written per (quad, slot, BASE detector) by
// k_radon_adj_prepq, so that one ring slot index serves all slots).  A pixel's four members need four different geometries, so the
// sharing is between MIRRORED PIXELS: (tt, col) and (tt, N-1-col) exchange slots 0 / 1, (col, tt) and (N-1-col, tt) slots 2 / 3.  A
// workgroup therefore owns the orbit of a 32 x 32 tile under the two mirrors — tiles (a, b), (a, b~), (a~, b), (a~, b~) — and runs four
// sub-phases over all quads: rows of a / rows of a~ (slots 0 and 1, the column-mirrored pair of tiles each), columns of b / columns
// of b~ (slots 2 and 3, the row-mirrored pair each).  Per geometry: 8 shared vector instructions + 2 per member (k_radon_adj_tile: 10.25
// per pixel and angle; here 6), one ds_read_b128 per pixel and angle as before.  The four sums of a pixel (two sub-phases, two members
// each) meet in LDS; the tiles leave through one coalesced pass that carries the epilogue (a * A^T s + b * z, the norm partials,
// the transposed copy for the next forward apply).  Same taps and weights as k_radon_adj_tile, another summation order: tested
// against the float64 oracle and against that kernel.
__global__ __launch_bounds__(256) void k_radon_adj_prepq(const float* __restrict__ sino, uint4* __restrict__ recq, int nd, int na, int nq,
                                                         const QuadParam* __restrict__ quads, const float* __restrict__ wq,
                                                         const unsigned* __restrict__ A32q) {
  const int ndp = nd + 2 * A32_PAD;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;      // over (quad of the frame, slot) x ndp; blockIdx.y = frame
  const int64_t r = idx / ndp;
  if (r >= (int64_t)nq * 4) return;
  const int e = (int)(idx - r * ndp), q = (int)(r >> 2), m = (int)(r & 3);
  const int64_t qr = (int64_t)blockIdx.y * nq + q;
  const QuadParam p = quads[qr];
  const int am = m == 0 ? p.am[0] : (m == 1 ? p.am[1] : (m == 2 ? p.am[2] : p.am[3]));
  const bool flip = ((p.flip >> m) & 1) != 0;
  const float w = wq[qr * 4 + m];
  const int d = e - A32_PAD;
  const float* __restrict__ S = sino + ((int64_t)blockIdx.y * na + (am < 0 ? 0 : am)) * nd;
  auto val = [&](int db) -> float {                                 // the member's sample at BASE detector db
    const int dm = flip ? nd - 1 - db : db;
    return (am >= 0 && db >= 0 && db < nd) ? w * S[dm] : 0.f;
  };
  uint4 o;
  o.x = __builtin_bit_cast(unsigned, val(d - 1));                   // the base ray at t0 - inv (inv > 0)
  o.y = __builtin_bit_cast(unsigned, val(d + 1));                   // the base ray at t0 + inv
  o.z = __builtin_bit_cast(unsigned, val(d));
  o.w = A32q[qr * ndp + e];
  recq[(qr * 4 + m) * ndp + e] = o;
}

__global__ __launch_bounds__(256, 3) void k_radon_adj_quad(const uint4* __restrict__ recq, float* __restrict__ img, int N, int nd, int nq,
                                                        const AdjQuad* __restrict__ aq, const uint2* __restrict__ CBq, int npad,
                                                        int tiles_h, double* __restrict__ ssq_part, Epi epi,
                                                        float* __restrict__ xT_out) {
  constexpr int T = 32, PX = 4, TS = 8, QB = 4;                        // QB: quads per staged batch
  __shared__ __attribute__((aligned(16))) uint4 ring[2][QB][4][64];   // [buffer][quad of the batch][base tile 0: slot A, slot B; base tile 1: A, B]
  __shared__ __attribute__((aligned(16))) uint2 cbs[2][QB][T];        // {C, B32} of the base at the sub-phase's 32 marching indices
  __shared__ float sum[4][T][T + 1];                                   // the orbit's four tiles: [2 (row >= N/2) + (col >= N/2)]
  __shared__ double lds[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frame = blockIdx.y;
  const int ta = blockIdx.x / tiles_h, tb = blockIdx.x - ta * tiles_h;
  const int i0 = ta * T, j0 = tb * T;                                  // tile (a, b); its mirrors start at N - T - i0 / N - T - j0
  const int ndp = nd + 2 * A32_PAD;
  aq += (int64_t)frame * nq;
  CBq += (int64_t)frame * nq * npad;
  recq += (int64_t)frame * nq * 4 * ndp;
  const auto rrec = __builtin_amdgcn_make_buffer_rsrc((void*)recq, 0, (unsigned)((int64_t)nq * 4 * ndp * 16), 0x00020000);
  const auto rcb = __builtin_amdgcn_make_buffer_rsrc((void*)CBq, 0, (unsigned)((int64_t)nq * npad * 8), 0x00020000);
  const float sdh = 0.5f * (float)(nd - 1);
  f2v sc2 = {5.9604644775390625e-8f, 5.9604644775390625e-8f};          // 2^-24, kept in an (aligned) VGPR pair
  float nsc = -5.9604644775390625e-8f;
  asm("" : "+v"(sc2));
  asm("" : "+s"(nsc));
  const int nbatch = (nq + QB - 1) / QB;
  const int r0 = tid / TS, c0 = tid % TS;                              // sub-phases 0, 1: row r0, columns c0 + 8 k
  int nqm1;
  asm("s_add_i32 %0, %1, -1" : "=s"(nqm1) : "s"(nq) : "scc");

#pragma unroll 1
  for (int sp = 0; sp < 4; ++sp) {
    // the sub-phase's geometry: marching index tt (fixed per thread), interpolated coordinates col_k and their mirrors N-1-col_k
    const bool colmode = sp >= 2;
    const int u0 = colmode ? j0 : i0, v0 = colmode ? i0 : j0;          // marching tile start / interpolated tile start (unmirrored)
    const int tl = colmode ? tid / TS : r0;                            // marching index within the tile
    const int cl = colmode ? tid % TS : c0;                            // first interpolated index within the tile
    const bool mir_t = (sp & 1) != 0;                                  // sub-phases 1, 3: the mirrored marching tile
    const int tt0 = mir_t ? N - T - u0 : u0;                           // its first marching index (ascending table order)
    const int tt = mir_t ? N - 1 - (u0 + tl) : u0 + tl;
    const int ttl = tt - tt0;
    const int slotA = colmode ? 2 : 0;
    float fcol[2][PX];
    unsigned ncol[2][PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int c = v0 + cl + k * TS;
      fcol[0][k] = (float)c;
      ncol[0][k] = 0u - ((unsigned)c << QF);
      fcol[1][k] = (float)(N - 1 - c);
      ncol[1][k] = 0u - ((unsigned)(N - 1 - c) << QF);
    }
    // centres of the two base tiles (the interpolated tile and its mirror) for the ring bases
    const float tt_c = (float)tt0 + 0.5f * (float)(T - 1);
    const float co_c0 = (float)v0 + 0.5f * (float)(T - 1), co_c1 = (float)(N - T - v0) + 0.5f * (float)(T - 1);
    f2v an[2][PX];
    float ac[2][PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      an[0][k] = an[1][k] = (f2v){0.f, 0.f};
      ac[0][k] = ac[1][k] = 0.f;
    }
    // staging of batch b into buffer b & 1: wave w takes rings w, w + 4, ... of the batch's 4 QB (ring = quad * 4 + 2 * base tile + slot
    // B), lane l the base detector whose ring slot is l; threads 0 .. 16 QB - 1 the {C, B32} pairs (16 bytes = two indices each)
    float nx_rinv, nx_dq, nx_k0;
    auto fetch_quads = [&](int b) {
      int q = b * QB + (lane & (QB - 1));
      q = q < nq ? q : nq - 1;
      nx_rinv = aq[q].rinv;
      nx_dq = aq[q].dq;
      nx_k0 = aq[q].k0;
    };
    fetch_quads(0);
    auto stage_load = [&](int b) {
      // lane (q, base tile) = (lane & (QB-1), (lane / QB) & 1) works out one ring base; handed out by v_readlane (no scalar float unit)
      int dbase_l;
      {
        const float co_c = ((lane / QB) & 1) ? co_c1 : co_c0;
        dbase_l = (int)floorf(fmaf(co_c - fmaf(tt_c, nx_dq, nx_k0), nx_rinv, sdh)) - 32;
      }
      if (b + 1 < nbatch) fetch_quads(b + 1);
#pragma unroll
      for (int h = 0; h < QB; ++h) {
        const int rr = wv + 4 * h;                                     // ring of the batch: quad rr / 4, base tile (rr / 2) & 1, slot A + (rr & 1)
        const int ql = rr >> 2, bt = (rr >> 1) & 1;
        int q;
        asm("s_min_i32 %0, %1, %2" : "=s"(q) : "s"(b * QB + ql), "s"(nqm1) : "scc");
        const int row = (q * 4 + slotA + (rr & 1)) * ndp;
        const int dbase = __builtin_amdgcn_readlane(dbase_l, ql + QB * bt);
        const int d = dbase + ((lane - dbase) & 63);
        int e;
        asm("v_med3_i32 %0, %1, 0, %2" : "=v"(e) : "v"(d + A32_PAD), "s"(ndp - 1));
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rrec, (__attribute__((address_space(3))) void*)&ring[b & 1][ql][rr & 3][0], 16, (row + e) * 16, 0, 0, 0);
      }
      if (tid < QB * T / 2) {
        const int ql = tid / (T / 2), pr = tid - ql * (T / 2);
        int q = b * QB + ql;
        q = q < nq ? q : nq - 1;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rcb, (__attribute__((address_space(3))) void*)(reinterpret_cast<char*>(&cbs[b & 1][0][0]) + wv * 1024), 16,
                                                 (q * npad + tt0 + 2 * pr) * 8, 0, 0, 0);
      }
    };
    stage_load(0);
    for (int b = 0; b < nbatch; ++b) {
      const int buf = b & 1;
      __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0): this wave's share of batch b has landed
      __syncthreads();                               // batch b complete; everyone is done with the other buffer
      if (b + 1 < nbatch) stage_load(b + 1);
      const int nql = (nq - b * QB < QB) ? nq - b * QB : QB;
      const unsigned rbase = __builtin_amdgcn_readfirstlane(lds_offset(&ring[buf][0][0][0]));
      // Software pipeline over the batch's 2 QB half-quads (round 6, second pass): the eight record reads of half-quad i + 1 are in
      // flight while half-quad i is weighed — LDS returns in order, so "at most nine younger reads outstanding" means half-quad i has
      // landed.  No scalar load may be outstanding inside (they return out of order: any wait would have to be lgkmcnt(0)), so the
      // batch's constants are fetched up front; the {C, B32} pair of the next quad rides between the two halves' reads.
      float q_c1m[QB], q_c1p[QB], q_rinv[QB];
#pragma unroll
      for (int ql = 0; ql < QB; ++ql) {
        const int qi = b * QB + (ql < nql ? ql : 0);          // wave-uniform: scalar loads
        q_c1m[ql] = aq[qi].c1m;
        q_c1p[ql] = aq[qi].c1p;
        q_rinv[ql] = aq[qi].rinv;
      }
      u2r cbq = pair_read(&cbs[buf][0][ttl]);
      ring_wait();
      pair_tie(cbq);
      u4r ra[2][PX], rb[2][PX];
      auto issue = [&](int ql, int h, float rinv_q, float C) {
        const unsigned rb_h = rbase + (unsigned)(ql * 4 + 2 * h) * 1024u;
#pragma unroll
        for (int k = 0; k < PX; ++k) {
          const unsigned bits = __builtin_bit_cast(unsigned, fmaf(fcol[h][k], rinv_q, C) + RND_MAGIC);
          unsigned addr;
          const unsigned slot = bits & 63u;
          asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(addr) : "v"(slot), "s"(rb_h));
          asm volatile("ds_read_b128 %0, %1" : "=v"(ra[h][k]) : "v"(addr) : "memory");
          asm volatile("ds_read_b128 %0, %1 offset:1024" : "=v"(rb[h][k]) : "v"(addr) : "memory");
        }
      };
      auto weigh = [&](int h, unsigned cb_y, f2v cr) {
#pragma unroll
        for (int k = 0; k < PX; ++k) {
          ring_tie(ra[h][k]);
          ring_tie(rb[h][k]);
          // slot A's member sees the pixel of this geometry, slot B's its mirror: tile set h / 1 - h
          const unsigned slo = ra[h][k][0], shi = ra[h][k][1], s0 = ra[h][k][2], a32 = ra[h][k][3];
          const unsigned mlo = rb[h][k][0], mhi = rb[h][k][1], m0 = rb[h][k][2];
          unsigned ti;
          asm("v_add3_u32 %0, %1, %2, %3" : "=v"(ti) : "v"(a32), "v"(cb_y), "v"(ncol[h][k]));
          const float tf = (float)(int)ti;
          f2v t2;
          t2[0] = tf;
          f2v wn;
          asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,0,1] neg_hi:[0,1,0] clamp" : "=v"(wn) : "v"(t2), "v"(sc2), "s"(cr));
          float w0;
          asm("v_fma_f32 %0, |%1|, %2, 1.0" : "=v"(w0) : "v"(tf), "s"(nsc));
          const f2v sn = {__builtin_bit_cast(float, slo), __builtin_bit_cast(float, shi)};
          const f2v mn = {__builtin_bit_cast(float, mlo), __builtin_bit_cast(float, mhi)};
          an[h][k] = __builtin_elementwise_fma(wn, sn, an[h][k]);
          ac[h][k] = fmaf(w0, __builtin_bit_cast(float, s0), ac[h][k]);
          an[1 - h][k] = __builtin_elementwise_fma(wn, mn, an[1 - h][k]);
          ac[1 - h][k] = fmaf(w0, __builtin_bit_cast(float, m0), ac[1 - h][k]);
        }
      };
      issue(0, 0, q_rinv[0], __builtin_bit_cast(float, (unsigned)cbq[0]));
#pragma unroll
      for (int ql = 0; ql < QB; ++ql) {
        if (ql < nql) {                                      // wave-uniform
          const u2r cbv = cbq;                               // (a copy of a pair that has landed and been tied)
          const float C = __builtin_bit_cast(float, (unsigned)cbv[0]);
          const unsigned cb_y = cbv[1];
          f2v cr = {q_c1m[ql], q_c1p[ql]};
          asm("" : "+s"(cr));
          issue(ql, 1, q_rinv[ql], C);                       // 8 more reads ...
          const int qln = ql + 1 < QB ? ql + 1 : ql;         // (the last quad of a batch re-reads its own pair: unconditional, no join)
          cbq = pair_read(&cbs[buf][qln][ttl]);              // ... and the next quad's pair behind them
          asm volatile("s_waitcnt lgkmcnt(9)" ::: "memory");  // half 0 of this quad has landed
          weigh(0, cb_y, cr);
          ring_wait();                                       // half 1 and the pair have landed (they had half 0's arithmetic to do so)
          pair_tie(cbq);
          if (ql + 1 < QB) {                                 // (compile-time; the reads themselves are unconditional — a quad beyond the batch's
            const bool more = ql + 1 < nql;                  //  last re-reads this one's rings: no join behind an asynchronous read)
            issue(more ? ql + 1 : ql, 0, more ? q_rinv[ql + 1 < QB ? ql + 1 : ql] : q_rinv[ql], __builtin_bit_cast(float, (unsigned)cbq[0]));
          }
          weigh(1, cb_y, cr);
        }
      }
      // A batch of fewer than QB quads (the last one when nq % QB != 0) ends with its last quad's re-read of half 0 in flight, and nobody
      // weighs it.  It has to land while ra[0] / rb[0] are still its registers: to the compiler they are free from the read's statement
      // on, and unwaited the eight records land in whatever they hold by then — the addresses and sums of the pass below (2048^2 with
      // two quads: ~100 pixels per apply that change from run to run, some of them table bits read as floats).
      if (nql < QB) {
        ring_wait();
#pragma unroll
        for (int k = 0; k < PX; ++k) {
          ring_tie(ra[0][k]);
          ring_tie(rb[0][k]);
        }
      }
    }
    // the sub-phase's sums meet the other one's in LDS: pixel (row, col) of tile set h, interpolated index col_k (h = 0) or its mirror
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int k = 0; k < PX; ++k) {
        const int c = h ? N - 1 - (v0 + cl + k * TS) : v0 + cl + k * TS;
        const int row = colmode ? c : tt, col = colmode ? tt : c;
        float* dst = &sum[2 * (row >= N / 2 ? 1 : 0) + (col >= N / 2 ? 1 : 0)][row & (T - 1)][col & (T - 1)];
        const float v = ac[h][k] + (an[h][k][0] + an[h][k][1]);
        *dst = colmode ? *dst + v : v;
      }
    __syncthreads();
  }

  // ---- the four tiles leave: rows of 32 contiguous pixels per quarter-wave, the epilogue of trk_op_apply_axpby on the way
  const bool lead = blockIdx.x == 0 && blockIdx.y == 0;
  float ca, cb;
  double pend_sum = 0.0, cad, cbd;
  img += (int64_t)frame * N * N;
  const int pc = tid & 31, pr = tid >> 5;
  float zv[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = ((t >> 1) ? N - T - i0 : i0) + pr + 8 * k, j = ((t & 1) ? N - T - j0 : j0) + pc;
      zv[t][k] = (epi.on && epi.z) ? epi.z[((int64_t)frame * N + i) * N + j] : 0.f;
    }
  epi_coefs(epi, lead, &lds[0], ca, cb, &pend_sum, &cad, &cbd);
  double q = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = ((t >> 1) ? N - T - i0 : i0) + pr + 8 * k, j = ((t & 1) ? N - T - j0 : j0) + pc;
      float o = sum[t][pr + 8 * k][pc];
      if (epi.on) o = epi_combine(epi.on, ca, cb, cad, cbd, o, zv[t][k], epi.z != nullptr);
      img[(int64_t)i * N + j] = o;
      if (xT_out) sum[t][pr + 8 * k][pc] = o;
      q += (double)o * o;
    }
  if (xT_out) {
    xT_out += (int64_t)frame * N * N;
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = ((t >> 1) ? N - T - i0 : i0) + pc, j = ((t & 1) ? N - T - j0 : j0) + pr + 8 * k;
        xT_out[(int64_t)j * N + i] = sum[t][pc][pr + 8 * k];
      }
  }
  if (ssq_part) {
    q = block_sum<256>(q, lds);
    if (tid == 0) ssq_part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = q;
  }
}

// The same arithmetic without LDS (one thread per pixel, records and table pairs read from memory): the reference form the
// tiled kernel is tested against (TRK_RADON_ADJ_SIMPLE=1 selects it) and the path for frames too small to tile.
__global__ __launch_bounds__(256) void k_radon_adj_simple(const uint4* __restrict__ rec, float* __restrict__ img, int N, int nd, int na,
                                                          const AdjAngle* __restrict__ ang, const int* __restrict__ n_mode0,
                                                          const uint2* __restrict__ CB, int npad) {
  const int64_t idx_raw = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool inside = idx_raw < (int64_t)N * N;
  const int64_t idx = inside ? idx_raw : (int64_t)N * N - 1;
  const int i = (int)(idx / N), j = (int)(idx - (int64_t)i * N);
  const int frame = blockIdx.y;
  const int ndp = nd + 2 * A32_PAD;
  ang += (int64_t)frame * na;
  rec += (int64_t)frame * na * ndp;
  CB += (int64_t)frame * na * npad;
  const int n0 = n_mode0[frame];
  float acc0 = 0.f;
  f2v accn = {0.f, 0.f};
  f2v sc2 = {5.9604644775390625e-8f, 5.9604644775390625e-8f};
  float nsc = -5.9604644775390625e-8f;
  asm("" : "+v"(sc2));
  asm("" : "+s"(nsc));
  for (int a = 0; a < na; ++a) {
    const AdjAngle p = ang[a];
    const int tt = a < n0 ? i : j, col = a < n0 ? j : i;
    const uint2 cb = CB[(int64_t)p.orig * npad + tt];
    int d0 = (int)rintf(fmaf((float)col, p.rinv, __builtin_bit_cast(float, cb.x)));
    int e = d0 + A32_PAD;
    e = e < 0 ? 0 : (e > ndp - 1 ? ndp - 1 : e);
    const uint4 rr = rec[(int64_t)a * ndp + e];
    f2v cr = {p.c1m, p.c1p};
    asm("" : "+s"(cr));
    adj_gather((u4r){rr.x, rr.y, rr.z, rr.w}, cb.y, 0u - ((unsigned)col << QF), sc2, nsc, cr, accn, acc0);
  }
  const float acc = acc0 + (accn[0] + accn[1]);
  if (inside) img[(int64_t)frame * N * N + idx] = acc;
}

}  // namespace

namespace trk {
namespace radon {

AdjPath adj_path(const RadonImpl* im, int batch, bool riders) {
  const int N = im->N, na = im->na, nt = im->nt;
  if (getenv("TRK_RADON_ADJ_SIMPLE") != nullptr || N < 16) return AdjPath{AdjKind::simple, true, 1, 0, ceil_div((int64_t)N * N, 256)};
  AdjPath a{AdjKind::tile32_b8, na > 32, 1, 0, 0};     // few angles per frame: the tile kernel makes its records itself
  // 32 x 32 tiles with 4 pixels per thread (fewest instructions per pixel) need enough tiles to fill the chip (frames of a
  // dynamic problem count); below that 16 x 16 tiles with one pixel per thread (4 x the waves)
  // measured: 512^2 x 180 (one frame: 256 / 1024 tiles) 51 vs 42 us; 32 frames x 256^2 x 15 (2048 / 8192 tiles) 21 vs 34 us
  const int64_t tiles32 = (int64_t)ceil_div(N, 32) * ceil_div(N, 32) * nt;
  // Too few 32 x 32 tiles to fill the chip, many angles: the angles of a tile are SPLIT over nsplit workgroups whose partial tiles
  // meet in the one that finishes last (k_radon_adj_tile) — the instructions per pixel and angle of the 32 x 32 form (10.25 against
  // 14.5 for 16 x 16 tiles with one pixel per thread, where the staging of a batch is shared by a quarter of the pixels) at the
  // same number of waves.
  // measured (us per apply, 180 angles; 16 x 16 tiles -> split 2 / 4 / 8): 256^2 24.1 -> 32.6 / 21.4 / 16.3, 512^2 32.9 -> 36.5 / 29.8 /
  // 29.8, 768^2 63.2 -> 54.8 / 50.4 / 50.9; 1024^2 (1024 tiles: 32 x 32 unsplit already) 83 with or without
  if (batch == 1 && tiles32 < 1024 && na > 32 && N >= 64) a.nsplit = tiles32 <= 128 ? 8 : 4;
  const int T = (tiles32 >= 1024 || a.nsplit > 1) ? 32 : 16;
  a.tiles_x = ceil_div(N, T);
  a.blocks = (int64_t)a.tiles_x * a.tiles_x;
  const int64_t wgs = a.blocks * nt;
  if (T == 32) {
    // round 6: the adjoint by mirrored tile pairs where the handle allows it (whole 64 x 64 super-tiles, mostly complete quads) and
    // no rider travels on the epilogue (the damped-LSQR update and the mailbox post stay with k_radon_adj_tile);
    // TRK_RADON_NO_ADJQ=1: k_radon_adj_tile everywhere (read per call: the tests switch it)
    if (a.nsplit == 1 && im->adjq_ok && !riders && getenv("TRK_RADON_NO_ADJQ") == nullptr) {
      a.kind = AdjKind::quad;
      a.prep = true;
      a.blocks = (int64_t)(N / 64) * (N / 64);
    } else if (a.nsplit == 4 && wgs <= cu_count() && wgs * 4 >= 3 * cu_count()) {
      a.kind = AdjKind::groups;    // the parts of a tile as groups of ONE workgroup where that gives about one workgroup per CU (512^2: 256 tiles)
    }
    // (16 angles per batch — half the barriers, twice the rings — measured at 512^2 x 180: 34.7 us against 29.9; and one batch for a
    //  15-angle frame, measured again in round 6 on C5's shape, 32 frames of 256^2 x 15 angles: see profiles/r06/adj_ab16.txt)
  } else if (na > 32 || wgs <= 4 * (int64_t)cu_count()) {
    // 16 angles per batch also for the few frames of a dynamic problem one rank of eight holds — 4 frames of 256^2 x 15 angles, 1 024
    // workgroups: 10.2 -> 9.1 us per apply, profiles/r06/adj_ab16.txt; with more workgroups than that the shorter batches win
    a.kind = AdjKind::tile16_b16;
  } else {
    a.kind = AdjKind::tile16_b4;   // few angles per frame (dynamic problems: 15): short batches, so that staging and gathering still overlap
  }
  return a;
}


int radon_adjoint(RadonImpl* im, const AdjPath& ap, const float* xb, float* yb, int hints, int batch, const Epi& epi, double* ssq_part,
                  hipStream_t s) {
  const int N = im->N, nd = im->nd, na = im->na, nt = im->nt;
  const int ndp = nd + 2 * A32_PAD;
  const bool tile = ap.kind != AdjKind::simple;
  float* xT_out = ((hints & HINT_OUT_FEEDS_OPPOSITE) && tile && im->n_mode1 > 0 && batch == 1) ? im->xT : nullptr;
  if (ap.kind == AdjKind::quad) {
    hipLaunchKernelGGL(k_radon_adj_prepq, dim3(ceil_div((int64_t)im->nq * 4 * ndp, 256), nt), dim3(256), 0, s, xb, im->recq, nd, na, im->nq,
                           im->quad_dev, im->wq, im->A32q);
    im->rec_src = nullptr;
  } else if (ap.prep) {
    if (!((hints & HINT_INPUT_FROM_OPPOSITE) && im->rec_src == xb))   // else: the forward that produced xb left its records
      hipLaunchKernelGGL(k_radon_adj_prep, dim3(ceil_div((int64_t)na * ndp, 256), nt), dim3(256), 0, s, xb, im->rec, nd, na,
                             im->adj_ang, im->adj_wgt, im->A32);
    im->rec_src = nullptr;
  }
  if (ap.nsplit > 1) {
    const int64_t need = (int64_t)ap.nsplit * nt * ap.blocks * 1024, need_c = (int64_t)nt * ap.blocks;
    if (im->adj_part_cap < need) {
      if (im->adj_part) (void)hipFree(im->adj_part);
      im->adj_part = nullptr;
      im->adj_part_cap = 0;
      if (hipMalloc((void**)&im->adj_part, sizeof(float) * (size_t)need) != hipSuccess) return fail(TRK_EHIP, "radon: hipMalloc (adjoint partial tiles) failed");
      im->adj_part_cap = need;
    }
    if (im->adj_cnt_cap < need_c) {
      if (im->adj_cnt) (void)hipFree(im->adj_cnt);
      im->adj_cnt = nullptr;
      im->adj_cnt_cap = 0;
      if (hipMalloc((void**)&im->adj_cnt, sizeof(unsigned) * (size_t)need_c) != hipSuccess) return fail(TRK_EHIP, "radon: hipMalloc (adjoint tile counters) failed");
      if (hipMemsetAsync(im->adj_cnt, 0, sizeof(unsigned) * (size_t)need_c, s) != hipSuccess) return fail(TRK_EHIP, "radon: hipMemsetAsync failed");
      im->adj_cnt_cap = need_c;
    }
  }
  // groups: the four parts of a tile in one workgroup of 1024 threads (nsplit = 1 to the kernel); else nsplit workgroups per tile
#define ADJ_TILE(TT, PP, BB, PR, G, NSPLIT)                                                                                          \
  hipLaunchKernelGGL((k_radon_adj_tile<TT, PP, BB, PR, G>), dim3((unsigned)(ap.blocks * NSPLIT), nt), dim3(256 * G), 0, s, xb, im->rec, \
                     yb, N, nd, na, im->adj_ang, im->adj_wgt, im->A32, im->adj_n0, im->CB, im->npad, ap.tiles_x, ssq_part, epi, xT_out,  \
                     NSPLIT, im->adj_part, im->adj_cnt)
  switch (ap.kind) {
    case AdjKind::quad:
      hipLaunchKernelGGL(k_radon_adj_quad, dim3((unsigned)ap.blocks, nt), dim3(256), 0, s, im->recq, yb, N, nd, im->nq, im->adjq,
                             im->CBq, im->npad, N / 64, ssq_part, epi, xT_out);
      break;
    case AdjKind::groups:
      if (ap.prep) ADJ_TILE(32, 4, 8, true, 4, 1); else ADJ_TILE(32, 4, 8, false, 4, 1);
      break;
    case AdjKind::tile32_b8:
      if (ap.prep) ADJ_TILE(32, 4, 8, true, 1, ap.nsplit); else ADJ_TILE(32, 4, 8, false, 1, ap.nsplit);
      break;
    case AdjKind::tile16_b16:
      if (ap.prep) ADJ_TILE(16, 1, 16, true, 1, 1); else ADJ_TILE(16, 1, 16, false, 1, 1);
      break;
    case AdjKind::tile16_b4:
      if (ap.prep) ADJ_TILE(16, 1, 4, true, 1, 1); else ADJ_TILE(16, 1, 4, false, 1, 1);
      break;
    case AdjKind::simple:
      hipLaunchKernelGGL(k_radon_adj_simple, dim3((unsigned)ap.blocks, nt), dim3(256), 0, s, im->rec, yb, N, nd, na, im->adj_ang,
                             im->adj_n0, im->CB, im->npad);
      break;
  }
#undef ADJ_TILE
  if (xT_out) im->xT_src = yb;
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

}  // namespace radon
}  // namespace trk
