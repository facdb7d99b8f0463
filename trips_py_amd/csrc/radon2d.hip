// radon2d.hip — parallel-beam Radon transform (Joseph / linear-interpolation projector) and its matched adjoint.
//
// Replaces astra.OpTomo over create_proj_geom('parallel', 1, N, theta) + create_projector('linear', ...) and the
// 1/N scaling of trips/utilities/io.py:392-399.  astra-toolbox is not installable in the build image; the convention below
// (oracle/cpu_ref.py, Radon2D) is pinned to the ASTRA outputs the reference holds as images — through the fan-beam operator whose
// far-source limit this one is (tests/test_oracle_golden.py, tests/test_gpu_operators.py) — and by the adjoint identity, analytic
// line integrals and the axis-aligned views; the interpolation weights are Joseph's published kernel.
//
// Geometry: pixel (i,j) centre (x,y) = (j - h, h - i), h = (N-1)/2; detector bin d at s = d - (n_det-1)/2 along
// (cos t, sin t); rays run along (sin t, -cos t).  Per angle one of two marching modes:
//   mode 0 (|cos| >= |sin|): march image rows  tt = i, coordinate q = column:  q = s/cos + (h - h tan) + i tan
//   mode 1 (otherwise)     : march image cols  tt = j, coordinate q = row   :  q = -s/sin + (h - h cot) + j cot
// i.e.  q(d, tt) = A(d) + B(tt),  A(d) = s_d inv + k0,  B(tt) = tt dq;  taps at floor(q), floor(q)+1, weights (1-f), f,
// times wgt = scale/|cos| (or /|sin|).
//
// FIXED-POINT RAY COORDINATE (round 2).  Evaluated in fp32, q — a number up to N — carries an error of ~6e-8 N, i.e. an
// interpolation weight off by 2e-4 at N = 4096 (measured 1.9e-4 relative on white noise).  Here the two terms come from
// TABLES made once per operator in float64 and rounded to 24 fractional bits, A32[a][d] = round(A(d) 2^24) mod 2^32 and
// B32[a][tt] = round(B(tt) 2^24) mod 2^32, and the kernels add them as INTEGERS:
//     Q = A32 + B32 (mod 2^32):   column mod 256 = Q >> 24,   f = (Q & 0xFFFFFF) 2^-24   (exact in fp32, as is 1 - f).
// Every weight is within 2^-24 of its float64 value whatever N; forward and adjoint read the same tables, so the nearest
// ray's weight in the adjoint is bit-identical to the forward's; the absolute column comes from where the tap is looked
// for (the LDS window start, the gathering pixel) — 8 integer bits are plenty for that.  The march costs what it did
// (7 vector instructions per step); measured against the float64 oracle: DESIGN.md §4.4.
//
// Forward: mode-1 angles read a transposed copy of the image so that both modes read ROWS: the 64 adjacent detectors of
// a wave touch 64..90 contiguous floats per marching step.  The grid runs over bands of 128 marching rows (see
// k_radon_fwd); a workgroup is 64 detectors x 4 neighbouring angles.
// Adjoint: gather form, no atomics (k_radon_adj_tile): per pixel and angle the nearest ray d0 and its two neighbours —
// every ray within one pixel is among them, because |dq/dd| = 1/|cos| >= 1 — from 16-byte records staged in LDS.
//
// Roofline note: algorithmic bytes are only 4(N^2 + n_ang n_det) against 2 N n_det n_ang taps, so this
// operator is bound by LDS reads / vector issue, not HBM; bench.py reports taps/s next to GB/s.
//
// This file: the handle and its float64 table construction (radon_create_impl), the apply's bookkeeping for fused, deferred and raw
// norms (radon_run), the C entry points.  The kernels and their dispatch: radon_fwd.hip, radon_adj.hip; what the three share:
// radon_internal.h.
#include "radon_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

using namespace trk;
using namespace trk::radon;

namespace {

int radon_flush(trk_op* op, hipStream_t s) {
  auto* im = static_cast<RadonImpl*>(op->impl);
  if (!im->pend_target) return TRK_OK;
  double* target = im->pend_target;
  im->pend_target = nullptr;
  return finalize_sums(im->pend_part, im->pend_n, 1, 1, target, s);
}

// Plain apply (epi.on = 0, hints = 0) and the fused form of trk_op_apply_axpby (batch 1) share this.
// ext_part / ext_cap / ext_n (trk_op_apply_fused with x2 = NULL): the fused norm is LEFT as block partials in the caller's buffer
// (*ext_n of them; one finished value if they do not fit) for a consumer kernel to add up — no finalize launch.
int radon_run(trk_op* op, int tr, const float* x, int64_t ldx, float* y, int64_t ldy, int batch, double* sumsq, Epi epi,
              int hints, hipStream_t s, double* ext_part = nullptr, int ext_cap = 0, int* ext_n = nullptr) {
  auto* im = static_cast<RadonImpl*>(op->impl);
  const int N = im->N, nd = im->nd, na = im->na, nt = im->nt;
  TimerScope tm(op->timer, op->timer_which, tr, s);
  // a norm the previous fused apply left unfinished: this apply's epilogue kernel finishes it if the caller chained the two
  // (it reads the partials for its coefficients), anything else gets it finished first
  epi.pend_target = nullptr;
  epi.pend_part = nullptr;
  epi.pend_n = 0;
  epi.dotv = nullptr;
  epi.dot_part = nullptr;
  if (im->pend_target) {
    if (epi.on && (hints & HINT_INPUT_FROM_OPPOSITE)) {
      epi.pend_target = im->pend_target;
      epi.pend_part = im->pend_part;
      epi.pend_n = im->pend_n;
      im->pend_target = nullptr;
    } else if (int rc = radon_flush(op, s)) {
      return rc;
    }
  }
  const AdjPath ap = adj_path(im, batch, epi.on && (op->post.on || op->lsqr.on));
  const bool tile = ap.kind != AdjKind::simple;
  const int ndp = nd + 2 * A32_PAD;
  // fused ||y||^2 (batch 1): block partials from the kernel that writes y (band reduction / gather), then one finalize —
  // or none, when the caller lets the next chained apply finish it (TRK_HINT_SUMSQ_DEFERRED)
  double* ssq_part = nullptr;
  if (epi.on && (batch != 1 || (tr && !tile))) return fail(TRK_EUNSUPPORTED, "radon: fused epilogue needs batch 1 and the tiled adjoint");
  // the forward's band reduction carries the epilogue / the fused norm / the adjoint's records
  const bool post = epi.on || im->n_bands > 1 || ext_part;
  if (ext_part) sumsq = ext_part;          // where a finished value goes when the partials do not fit / no kernel makes any
  const bool fuse_ssq = sumsq && batch == 1 && (tr ? tile : post);
  const int64_t post_blocks = ceil_div((int64_t)nt * na * ndp, 256);
  const int64_t n_part = tr ? ap.blocks * nt : post_blocks;
  epi.pq = PostReq{};
  if (tr && tile && batch == 1 && epi.on && op->post.on) {
    epi.pq = op->post;                         // trk_gk_step_post: the mailbox post on the adjoint kernel's first workgroup
    op->post_taken = 1;
  }
  epi.lq = LsqrReq{};
  if (tr && tile && batch == 1 && epi.on && epi.z && op->lsqr.on && (!op->lsqr.ref || n_part <= op->lsqr.err_cap)) {
    epi.lq = op->lsqr;                         // trk_gk_step_lsqr: the iterate's update on the adjoint's pixel pass (z = its vk)
    op->lsqr_blocks = (int)n_part;
  }
  if (!tr && post && batch == 1 && op->probe_vec && post_blocks <= op->probe_cap) {      // trk_gk_step_proj: <out, probe_vec> partials
    epi.dotv = op->probe_vec;
    epi.dot_part = op->probe_part;
    op->probe_n = (int)post_blocks;
  }
  const bool defer = fuse_ssq && epi.on && (hints & HINT_SUMSQ_DEFERRED) && n_part <= im->pend_cap;
  const bool raw_out = ext_part && fuse_ssq && n_part <= ext_cap;
  if (ext_n) *ext_n = raw_out ? (int)n_part : 1;
  if (raw_out) {
    ssq_part = ext_part;
  } else if (defer) {
    ssq_part = im->pend_buf[im->pend_which];        // not the buffer a pending norm of the previous apply is read from
    im->pend_which ^= 1;
  } else if (fuse_ssq) {
    if (int rc = scratch_doubles(s, (size_t)n_part, &ssq_part)) return rc;
  }
  auto finish_norm = [&]() -> int {
    if (raw_out) return TRK_OK;
    if (defer) {
      im->pend_target = sumsq;
      im->pend_part = ssq_part;
      im->pend_n = (int)n_part;
      return TRK_OK;
    }
    return finalize_sums(ssq_part, (int)n_part, 1, 1, sumsq, s);
  };
  if (!tr) {
    // a hinted forward leaves the records for the adjoint that follows where that adjoint reads k_radon_adj_prep's records (the
    // mirrored-pair adjoint reads records of its own kind, made by its own pre-pass: nothing to leave behind for it).  The plan is
    // asked without riders: an adjoint that carries them takes a tile route all the same and then makes its records itself.
    bool want_rec = false;
    if ((hints & HINT_OUT_FEEDS_OPPOSITE) && batch == 1) {
      const AdjPath next = adj_path(im, 1, /*riders=*/false);
      want_rec = next.prep && next.kind != AdjKind::quad && next.kind != AdjKind::simple;
    }
    for (int b = 0; b < batch; ++b)   // the transposed copy is per vector
      if (int rc = radon_forward(im, x + (int64_t)b * ldx, y + (int64_t)b * ldy, hints, post, want_rec, epi, ssq_part, post_blocks, s)) return rc;
  } else {
    for (int b = 0; b < batch; ++b)   // the record array is per vector
      if (int rc = radon_adjoint(im, ap, x + (int64_t)b * ldx, y + (int64_t)b * ldy, hints, batch, epi, ssq_part, s)) return rc;
  }
  if (ssq_part) {
    tm.stop();
    return finish_norm();
  }
  tm.stop();
  if (sumsq) {
    // the output is small next to the tap work: one extra streaming pass for the fused norm
    const int64_t nout = tr ? (int64_t)nt * N * N : (int64_t)nt * na * nd;
    if (batch == 1 || ldy == nout) return trk_nrm2sq(y, nout * batch, sumsq, (trk_stream)s);
    return fail(TRK_EUNSUPPORTED, "radon: fused sum of squares needs contiguous batch outputs");
  }
  return TRK_OK;
}

// ref_mode != 0 (trk_radon2d_set_arithmetic): every apply of the handle through ref64.hip's float64-arithmetic kernels
int radon_ref_geom_of(RadonImpl* im, RadonRefGeom* g) {
  *g = RadonRefGeom{im->N, im->nd, im->na, im->nt, im->npad, im->ref_ang, im->A32, im->B32, im->ref_chunk_fwd, im->ref_chunk_adj};
  return TRK_OK;
}
int radon_apply_refmode(trk_op* op, int tr, const float* x, int64_t ldx, float* y, int64_t ldy, int batch, double* sumsq, hipStream_t s) {
  auto* im = static_cast<RadonImpl*>(op->impl);
  if (int rc = radon_flush(op, s)) return rc;
  im->rec_src = nullptr;
  im->xT_src = nullptr;
  RadonRefGeom g;
  radon_ref_geom_of(im, &g);
  for (int bi = 0; bi < batch; ++bi)
    if (int rc = radon_ref_apply_f32(g, tr, im->ref_mode - 1, x + (int64_t)bi * ldx, y + (int64_t)bi * ldy, s)) return rc;
  if (sumsq) {
    const int64_t nout = tr ? op->cols : op->rows;
    if (batch == 1 || ldy == nout) return trk_nrm2sq(y, nout * batch, sumsq, (trk_stream)s);
    return fail(TRK_EUNSUPPORTED, "radon: fused sum of squares needs contiguous batch outputs");
  }
  return TRK_OK;
}

int radon_apply(trk_op* op, int tr, const float* x, int64_t ldx, float* y, int64_t ldy, int batch, double* sumsq,
                hipStream_t s) {
  if (static_cast<RadonImpl*>(op->impl)->ref_mode) return radon_apply_refmode(op, tr, x, ldx, y, ldy, batch, sumsq, s);
  return radon_run(op, tr, x, ldx, y, ldy, batch, sumsq, Epi{}, 0, s);
}

// trk_op_apply_fused for the projector: only its one-operand form (x2 = NULL) — y = Op(x1) with sum(y^2) left as the block
// partials of the kernel that writes y (band reduction / tile gather), which the CGLS update kernels add up themselves
// (trk_cgls_update_xr_src, trk_cgls_p_update): the two reduction launches of a CGLS iteration disappear.
int radon_apply_fused(trk_op* op, int tr, const float* x1, const float* x2, double, ScalarSrc, ScalarSrc, float*, float* y,
                      double* partials, int cap, int* n_partials, hipStream_t s) {
  if (x2) return fail(TRK_EUNSUPPORTED, "radon: the two-operand fused apply is not available (trk_op_fused_caps reports 2)");
  if (cap < 1) return fail(TRK_EINVAL, "radon: fused apply needs room for at least one partial");
  if (static_cast<RadonImpl*>(op->impl)->ref_mode) {          // the instrument: one finished partial
    if (n_partials) *n_partials = 1;
    return radon_apply_refmode(op, tr, x1, tr ? op->rows : op->cols, y, tr ? op->cols : op->rows, 1, partials, s);
  }
  return radon_run(op, tr, x1, tr ? op->rows : op->cols, y, tr ? op->cols : op->rows, 1, nullptr, Epi{}, 0, s, partials, cap,
                   n_partials);
}

// out = a * Op(x) + b * z (+ ||out||^2) inside the kernel that writes the output: the band reduction (forward) or the tile
// gather (adjoint).  Small frames the tiled adjoint does not take fall back to apply + trk_axpby.
int radon_apply_axpby(trk_op* op, int tr, const float* x, Coef a, Coef b, const float* z, float* out, double* sumsq, int hints,
                      hipStream_t s) {
  auto* im = static_cast<RadonImpl*>(op->impl);
  if (im->ref_mode) {
    // the instrument: Op(x) by the float64-arithmetic kernels, then the half step's combination as the product's epilogue forms
    // it (float64 coefficients and products, one rounding) with the norm finished at once; the riders of trk_gk_step_* are not
    // taken (their callers run them in launches of their own)
    const int64_t nout = tr ? op->cols : op->rows;
    if (!im->ref_tmp) {
      const int64_t cap = op->rows > op->cols ? op->rows : op->cols;
      TRK_HIP(hipMalloc((void**)&im->ref_tmp, sizeof(float) * (size_t)cap));
    }
    if (int rc = radon_apply_refmode(op, tr, x, tr ? op->rows : op->cols, im->ref_tmp, nout, 1, nullptr, s)) return rc;
    return ref_axpby_f32(nout, a, im->ref_tmp, b, z, out, sumsq, s);
  }
  if (tr && adj_path(im, 1, op->post.on || op->lsqr.on).kind == AdjKind::simple) {
    if (int rc = radon_run(op, tr, x, op->rows, out, op->cols, 1, nullptr, Epi{}, 0, s)) return rc;
    return trk_axpby(op->cols, a.c, a.num, a.den, a.flags, out, b.c, b.num, b.den, b.flags, z, out, sumsq, (trk_stream)s);
  }
  // The half step's combination a Op(x) + b z in float64 (coefficients as they are, one rounding of the result) — not in trk_axpby's
  // fp32 arithmetic, whose rounded coefficients perturb EVERY entry of a Golub-Kahan vector the same way: un-reorthogonalised
  // Lanczos amplified that 4.5 x at C3's semi-convergence transient (iterate 7 of Hybrid-LSQR at 512^2 x 180 against the float64
  // oracle: 1.57e-3 -> 3.5e-4; profiles/r04/c3_parity_epilogue.txt).  The kernels that write the output are far from the vector
  // unit's float64 rate.  TRK_RADON_EPI_F32=1 restores apply + trk_axpby to the bit.
  static const int epi_mode = getenv("TRK_RADON_EPI_F32") ? 1 : 2;
  return radon_run(op, tr, x, tr ? op->rows : op->cols, out, tr ? op->cols : op->rows, 1, sumsq, Epi{epi_mode, a, b, z, nullptr, nullptr, 0}, hints, s);
}

void radon_destroy(trk_op* op) {
  auto* im = static_cast<RadonImpl*>(op->impl);
  void* ptrs[] = {im->ref_ang, im->ref_tmp, im->quad_dev, im->A32q, im->B32q, im->ang_dev, im->xT, im->part, im->fidx, im->A32, im->B32, im->CB, im->adj_ang, im->adj_wgt, im->adj_n0, im->rec, im->adj_pos, im->pend_buf[0], im->pend_buf[1], im->adj_part, im->adj_cnt, im->qplan, im->qslow, im->adjq, im->CBq, im->wq, im->recq};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  delete im;
}

}  // namespace

static int radon_create_impl(int N, int n_det, const double* angles, int nt, int na, double scale, trk_op** out) {
  // the kernels address a frame through one buffer descriptor with 32-bit byte offsets
  if ((int64_t)N * N >= ((int64_t)1 << 29) || (int64_t)n_det >= ((int64_t)1 << 22))
    return fail(TRK_EUNSUPPORTED, "radon2d: frames of %d x %d pixels / %d detectors exceed the addressing of the kernels", N, N, n_det);
  if ((int64_t)nt * na > (int64_t)INT32_MAX / 4) return fail(TRK_EUNSUPPORTED, "radon2d: too many angles");
  const int n_ang = nt * na;
  const int ndp = n_det + 2 * A32_PAD;
  const int npad = ((N + ADJ_T - 1) / ADJ_T) * ADJ_T + 32;         // whole adjoint tiles + the forward's 16-entry scalar reads
  if ((int64_t)na * ndp * 16 >= ((int64_t)1 << 31) || (int64_t)na * npad * 8 >= ((int64_t)1 << 31))
    return fail(TRK_EUNSUPPORTED, "radon2d: %d angles x %d detectors per frame exceed the 2 GiB record addressing of the adjoint", na, n_det);
  std::vector<AngleParam> h(n_ang);
  std::vector<RadonRefAngle> href(n_ang);
  std::vector<float> wadj(n_ang);
  std::vector<unsigned> a32((size_t)n_ang * ndp), b32((size_t)n_ang * npad);
  std::vector<uint2> cb((size_t)n_ang * npad);
  const double half = 0.5 * (N - 1), sdh = 0.5 * (n_det - 1), one = (double)(1 << QF);
  auto fx = [&](double v) -> unsigned {                                   // round(v 2^24) mod 2^32
    return (unsigned)((uint64_t)(int64_t)std::llrint(v * one) & 0xFFFFFFFFull);
  };
  int n1 = 0;
  for (int a = 0; a < n_ang; ++a) {
    const double ct = std::cos(angles[a]), st = std::sin(angles[a]);
    double inv, dq, k0, w, rinv;
    AngleParam p;
    if (std::fabs(ct) >= std::fabs(st)) {
      p.mode = 0;
      inv = 1.0 / ct; dq = st / ct; k0 = half - half * st / ct; w = scale / std::fabs(ct); rinv = ct;
    } else {
      p.mode = 1;
      inv = -1.0 / st; dq = ct / st; k0 = half - half * ct / st; w = scale / std::fabs(st); rinv = -st;
      ++n1;
    }
    href[a] = RadonRefAngle{inv, dq, k0, w, p.mode, 0};
    p.inv = (float)inv; p.dq = (float)dq; p.k0 = (float)k0; p.rinv = (float)rinv;
    p.wgt = (float)(w / 4294967296.0);        // the forward kernels' weights are in units of 2^-32
    h[a] = p;
    wadj[a] = (float)w;                       // the adjoint's are plain
    for (int e = 0; e < ndp; ++e) a32[(size_t)a * ndp + e] = fx(((double)(e - A32_PAD) - sdh) * inv + k0);
    for (int t = 0; t < npad; ++t) {
      const unsigned B = fx((double)t * dq);
      b32[(size_t)a * npad + t] = B;
      const float C = (float)(sdh - (k0 + (double)t * dq) * rinv);      // d* = col rinv + C
      cb[(size_t)a * npad + t] = uint2{__builtin_bit_cast(unsigned, C), B};
    }
  }
  // ---- quads (k_radon_fwd_quad): per frame, angles that are images of one base angle beta in [0, 45 deg] under the symmetries of the
  // square grid share one wave.  With ctb = max(|cos|, |sin|), t = min / max (= tan beta), q_b(s, i) = s / ctb + h (1 - t) + i t:
  //   marching rows (|cos| >= |sin|):  cos > 0, sin >= 0: q = q_b(s, i)            cos < 0, sin >= 0: q = (N-1) - q_b(s, i)
  //                                    cos > 0, sin <  0: q = (N-1) - q_b(-s, i)   cos < 0, sin <  0: q = q_b(-s, i)
  //   marching columns (rows of xT):   sin > 0, cos >= 0: q = q_b(-s, j)           sin > 0, cos <  0: q = (N-1) - q_b(s, j)
  //                                    sin < 0, cos >= 0: q = (N-1) - q_b(-s, j)   sin < 0, cos <  0: q = q_b(s, j)
  // slot = 2 [xT] + 1 [mirrored]; -s = the detector index flipped.  The members' tables are then DERIVED from the base's, so that
  // the forward (base tables) and the adjoint (member tables) weigh every tap with the same bits:
  //   plain: A_m[e] = A_b[e'], B_m = B_b;   mirrored: A_m[e] = (N-1) 2^24 - A_b[e'], B_m = -B_b   (e' = e, or ndp-1-e when flipped).
  std::vector<QuadParam> quads;
  std::vector<unsigned> a32q, b32q;
  std::vector<AdjQuad> adjq_h;
  std::vector<uint2> cbq_h;
  std::vector<float> wq_h;
  bool adjq_mostly_full = false;
  int nq = 0;
  {
    struct Cand { double beta, ctb, t; int a, slot, flip; };
    std::vector<std::vector<QuadParam>> per_frame(nt);
    std::vector<std::vector<std::pair<double, double>>> geo(nt);          // (ctb, t) of every quad
    for (int f = 0; f < nt; ++f) {
      std::vector<Cand> c(na);
      for (int a = 0; a < na; ++a) {
        const double ct = std::cos(angles[(size_t)f * na + a]), st = std::sin(angles[(size_t)f * na + a]);
        Cand k;
        k.a = a;
        if (std::fabs(ct) >= std::fabs(st)) {
          k.ctb = std::fabs(ct); k.t = std::fabs(st) / std::fabs(ct);
          const bool cp = ct > 0, sp = st >= 0;
          k.slot = (cp == sp) ? 0 : 1;
          k.flip = sp ? 0 : 1;
        } else {
          k.ctb = std::fabs(st); k.t = std::fabs(ct) / std::fabs(st);
          const bool sp = st > 0, cp = ct >= 0;
          k.slot = 2 + ((sp == cp) ? 0 : 1);
          k.flip = (sp == cp) ? (sp ? 1 : 0) : (sp ? 0 : 1);
        }
        k.beta = std::atan2(k.t, 1.0);
        c[a] = k;
      }
      std::stable_sort(c.begin(), c.end(), [](const Cand& x, const Cand& y) { return x.beta < y.beta; });
      size_t i = 0;
      while (i < c.size()) {
        size_t j = i;
        while (j < c.size() && c[j].beta - c[i].beta <= 1e-12) ++j;
        // members i .. j-1 share the base; a slot met twice (the same angle given twice) opens another quad of the same base
        std::vector<char> used(j - i, 0);
        size_t left = j - i;
        while (left > 0) {
          QuadParam q{};
          q.inv = (float)(1.0 / c[i].ctb); q.dq = (float)c[i].t; q.k0 = (float)(half - half * c[i].t); q.rinv = (float)c[i].ctb;
          for (int m = 0; m < 4; ++m) q.am[m] = -1;
          for (size_t k = i; k < j; ++k) {
            if (used[k - i] || q.am[c[k].slot] >= 0) continue;
            q.am[c[k].slot] = c[k].a;
            q.mask |= 1 << c[k].slot;
            q.flip |= c[k].flip << c[k].slot;
            used[k - i] = 1;
            --left;
          }
          per_frame[f].push_back(q);
          geo[f].push_back({c[i].ctb, c[i].t});
        }
        i = j;
      }
      nq = std::max(nq, (int)per_frame[f].size());
    }
    quads.assign((size_t)nt * nq, QuadParam{});
    a32q.assign((size_t)nt * nq * ndp, 0u);
    b32q.assign((size_t)nt * nq * npad, 0u);
    const unsigned KN = (unsigned)(((uint64_t)(N - 1) << QF) & 0xFFFFFFFFull);
    for (int f = 0; f < nt; ++f) {
      for (size_t k = 0; k < per_frame[f].size(); ++k) {
        const size_t qr = (size_t)f * nq + k;
        quads[qr] = per_frame[f][k];
        const double ctb = geo[f][k].first, t = geo[f][k].second;
        const double inv = 1.0 / ctb, k0 = half - half * t;
        unsigned* Ab = &a32q[qr * ndp];
        unsigned* Bb = &b32q[qr * npad];
        for (int e = 0; e < ndp; ++e) Ab[e] = fx(((double)(e - A32_PAD) - sdh) * inv + k0);
        for (int tt = 0; tt < npad; ++tt) Bb[tt] = fx((double)tt * t);
        for (int m = 0; m < 4; ++m) {
          const int am = quads[qr].am[m];
          if (am < 0) continue;
          const size_t ar = (size_t)f * na + am;
          const bool mir = (m & 1) != 0, flp = ((quads[qr].flip >> m) & 1) != 0;
          for (int e = 0; e < ndp; ++e) {
            const unsigned v = Ab[flp ? ndp - 1 - e : e];
            a32[ar * ndp + e] = mir ? KN - v : v;
          }
          for (int tt = 0; tt < npad; ++tt) {
            const unsigned v = mir ? 0u - Bb[tt] : Bb[tt];
            b32[ar * npad + tt] = v;
            cb[ar * npad + tt].y = v;
          }
        }
      }
      for (size_t k = per_frame[f].size(); k < (size_t)nq; ++k)
        for (int m = 0; m < 4; ++m) quads[(size_t)f * nq + k].am[m] = -1;
    }
    // the adjoint by mirrored tile pairs (k_radon_adj_quad): base geometry per quad, its locator offsets and the members' weights
    adjq_h.assign((size_t)nt * nq, AdjQuad{0.f, 0.f, 1.f, 0.f, 0.f, 0});
    cbq_h.assign((size_t)nt * nq * npad, uint2{0u, 0u});
    wq_h.assign((size_t)nt * nq * 4, 0.f);
    int64_t members = 0;
    for (int f = 0; f < nt; ++f) {
      double carry = 0.0;                             // c1 on the 2^-24 grid, its rounding diffused over the quads in order of beta (see adj_ang below)
      for (size_t k = 0; k < per_frame[f].size(); ++k) {
        const size_t qr = (size_t)f * nq + k;
        const double ctb = geo[f][k].first, t = geo[f][k].second, k0 = half - half * t;
        const double c1x = (1.0 - 1.0 / ctb) * one, c1lo = std::floor(c1x), c1hi = std::ceil(c1x);
        const double cm = std::fabs(carry + (c1lo - c1x)) <= std::fabs(carry + (c1hi - c1x)) ? c1lo : c1hi, cp = cm;
        carry += cm - c1x;
        adjq_h[qr] = AdjQuad{(float)(cm / one), (float)(cp / one), (float)ctb, (float)t, (float)k0, 0};
        for (int tt = 0; tt < npad; ++tt) {
          const float C = (float)(sdh - (k0 + (double)tt * t) * ctb);
          cbq_h[qr * npad + tt] = uint2{__builtin_bit_cast(unsigned, C), b32q[qr * npad + tt]};
        }
        for (int m = 0; m < 4; ++m)
          if (quads[qr].am[m] >= 0) {
            wq_h[qr * 4 + m] = wadj[(size_t)f * na + quads[qr].am[m]];
            ++members;
          }
      }
    }
    adjq_mostly_full = 4 * members >= 3 * 4 * (int64_t)nt * nq;
  }
  int band = RADON_BAND;
  {
    // small frames (dynamic problems: 256^2 x 15 angles): 64-row bands double the workgroups of a grid that cannot fill the chip —
    // measured per apply: 4 frames (one rank's share of 32 on 8 GPUs) 13.2 -> 10.7 us, 8 frames 14.5 -> 11.6, 16 frames 17.7 -> 17.4,
    // 32 frames 24.6 -> 25.4.  Decided per FRAME, so that a dynamic handle and its frames' own handles sum in the same order.
    const int64_t wgs128 = (int64_t)((n_det + 63) / 64) * ((na + 3) / 4) * ((N + RADON_BAND - 1) / RADON_BAND);
    if (wgs128 < 64 && N > 64) band = 64;
  }
  // large images (the quad kernels): 256-row bands — half the band partials to clear, write and add up (4096^2 x 180: 94 -> 47 MB each
  // way; measured per apply 0.760 -> 0.725 ms with k_radon_fwd_quad, round 6), the four quads of a workgroup still inside one window
  if (N >= 2048 && N % QD_R == 0) band = 2 * RADON_BAND;
  // small images: a 64-row band of the image fits the LDS of a CU (k_radon_fwd_band).  TRK_RADON_NO_BANDRES=1: the per-wave windows
  const bool band_res = N % BR_ROWS == 0 && N >= 2 * BR_ROWS && N <= BR_NMAX && getenv("TRK_RADON_NO_BANDRES") == nullptr;
  if (band_res) band = br_rows(N);
  const int nb = (N + band - 1) / band;
  auto* im = new RadonImpl{};
  im->N = N; im->nd = n_det; im->na = na; im->nt = nt; im->n_mode1 = n1; im->npad = npad; im->n_bands = nb; im->band = band;
  im->band_res = band_res ? 1 : 0;
  hipError_t e = hipSuccess;
  auto up = [&](void** dst, const void* src, size_t bytes) {
    if (e == hipSuccess) e = hipMalloc(dst, bytes);
    if (e == hipSuccess && src) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
  };
  up((void**)&im->ang_dev, h.data(), sizeof(AngleParam) * n_ang);
  up((void**)&im->ref_ang, href.data(), sizeof(RadonRefAngle) * n_ang);
  if (n1 > 0) up((void**)&im->xT, nullptr, sizeof(float) * (size_t)nt * N * N);
  up((void**)&im->part, nullptr, sizeof(float) * (size_t)nb * n_ang * n_det);   // nb = 1: used by the fused epilogue form
  {
    std::vector<float> fi((size_t)N + 16);
    for (size_t i = 0; i < fi.size(); ++i) fi[i] = (float)i;
    up((void**)&im->fidx, fi.data(), sizeof(float) * fi.size());
  }
  up((void**)&im->A32, a32.data(), sizeof(unsigned) * a32.size());
  up((void**)&im->B32, b32.data(), sizeof(unsigned) * b32.size());
  up((void**)&im->CB, cb.data(), sizeof(uint2) * cb.size());
  im->nq = nq;
  up((void**)&im->quad_dev, quads.data(), sizeof(QuadParam) * quads.size());
  up((void**)&im->A32q, a32q.data(), sizeof(unsigned) * a32q.size());
  up((void**)&im->B32q, b32q.data(), sizeof(unsigned) * b32q.size());
  // the mirrored-pair adjoint: images of whole 64 x 64 super-tiles, mostly complete quads (single angles would pay for four), from
  // 2048^2 on (measured per apply, 180 angles, k_radon_adj_tile -> k_radon_adj_quad: 4096^2 1.009 -> 0.794 ms, 2048^2 0.263 -> 0.222,
  // 1024^2 0.084 -> 0.101: 256 workgroups of four sub-phases leave the chip half empty there).  TRK_RADON_ADJQ_MIN: the tests' knob
  const char* adjq_min_env = getenv("TRK_RADON_ADJQ_MIN");
  const int adjq_min = adjq_min_env ? atoi(adjq_min_env) : 2048;
  im->adjq_ok = (nq > 0 && N % 64 == 0 && N >= adjq_min && adjq_mostly_full && (int64_t)nq * 4 * ndp * 16 < ((int64_t)1 << 31)) ? 1 : 0;
  if (im->adjq_ok) {
    up((void**)&im->adjq, adjq_h.data(), sizeof(AdjQuad) * adjq_h.size());
    up((void**)&im->CBq, cbq_h.data(), sizeof(uint2) * cbq_h.size());
    up((void**)&im->wq, wq_h.data(), sizeof(float) * wq_h.size());
    up((void**)&im->recq, nullptr, sizeof(uint4) * (size_t)nt * nq * 4 * ndp);
  }
  {
    // adjoint tables: per frame, the angles with marching mode 0 first
    std::vector<AdjAngle> aa(n_ang);
    std::vector<int> n0(nt);
    std::vector<float> wg(n_ang);
    std::vector<int4> pos_of(n_ang);
    // What is left of that mismatch is rounding again, and again one value per angle.  The neighbour weights are formed as
    // clamp(c1 -+ t0 2^-24) by ONE fp32 FMA: t0 2^-24 lies on the 2^-24 grid, so whatever c1 holds below that grid is rounded away in
    // the result (exactly so for the weights in [0.5, 1), the ones that matter) — always the same way for an angle.  The float64
    // instrument separates it (profiles/r06/c3_instrument.txt: the product's neighbour RULE with unrounded weights sits on the fp32-
    // storage floor, the product 6-10 x above it).  So c1 is put ON the grid — the FMA is then exact, no rounding at all — and WHICH of
    // its two grid neighbours an angle gets is chosen by error diffusion over the angles in order of their direction: neighbouring
    // views back-project nearly the same field, so their biases (< 6e-8, alternating) cancel instead of adding up over 180 views.
    // (The kernels take the addend per SIDE — c1m for the neighbour on the smaller-q side, c1p for the other — so that a split
    //  {floor, ceil} with half the mean bias could be dealt as a third level.  Measured on C3, distance of iterates 5 / 6 / 7 / 8 from
    //  the float64 oracle: fp32 c1 from the fp32 inv 6.4e-6 / 4.5e-5 / 3.6e-4 / 1.06e-3 (round 5), fp32 c1 from the float64 inv
    //  7.9e-7 / 5.5e-6 / 3.3e-5 / 2.3e-4, on the grid with diffusion 3.2e-7 / 2.0e-6 / 1.2e-5 / 6.9e-5, with the split levels 3.8e-7 /
    //  2.5e-6 / 1.5e-5 / 8.9e-5; the fp32-storage floor 1.2e-7 / 6.5e-7 / 3.9e-6 / 2.0e-5 — so both sides get the same value.)
    std::vector<float> c1m_d(n_ang), c1p_d(n_ang);
    for (int f = 0; f < nt; ++f) {
      std::vector<int> order(na);
      for (int a = 0; a < na; ++a) order[a] = a;
      auto dir = [&](int a) { double t = std::fmod(angles[(size_t)f * na + a], M_PI); return t < 0 ? t + M_PI : t; };
      std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return dir(x) < dir(y); });
      double carry = 0.0;
      for (int a : order) {
        const double exact = (1.0 - std::fabs(href[(size_t)f * na + a].inv)) * one;       // in units of 2^-24 (<= 0)
        const double lo = std::floor(exact), hi = std::ceil(exact);
        const double pick = std::fabs(carry + (lo - exact)) <= std::fabs(carry + (hi - exact)) ? lo : hi;
        carry += pick - exact;
        c1m_d[(size_t)f * na + a] = c1p_d[(size_t)f * na + a] = (float)(pick / one);        // |pick| < 2^23: exact
      }
    }
    // A handle that has the mirrored-pair adjoint takes it for a plain apply and k_radon_adj_tile for one that carries a rider: both must
    // be ONE matrix.  k_radon_adj_quad weighs the four members of a quad with the quad's c1 (one packed FMA serves them all), so here the
    // members take that value too — with their own, from the diffusion over the angles above, every neighbour weight of about half the
    // angles differed between the two routes by one grid step (2048^2, two quads: up to 1.5 x 2^-24 w scale on ~450 pixels of a ray).
    if (im->adjq_ok)
      for (int f = 0; f < nt; ++f)
        for (int k = 0; k < nq; ++k)
          for (int m = 0; m < 4; ++m) {
            const int am = quads[(size_t)f * nq + k].am[m];
            if (am < 0) continue;
            c1m_d[(size_t)f * na + am] = adjq_h[(size_t)f * nq + k].c1m;
            c1p_d[(size_t)f * na + am] = adjq_h[(size_t)f * nq + k].c1p;
          }
    for (int f = 0; f < nt; ++f) {
      int pos = 0;
      for (int pass = 0; pass < 2; ++pass) {
        for (int a = 0; a < na; ++a) {
          const AngleParam& q = h[(size_t)f * na + a];
          if (q.mode != pass) continue;
          // c1 = 1 - |inv| from the float64 inv (round 6).  Formed from the fp32-rounded inv it was off by up to 7e-8 — the same
          // amount for EVERY neighbour weight of the angle, while the forward's weights are exact: a systematic mismatch between A
          // and A^T of the size the float64 instrument showed to cost C3's transient iterates 50 x (profiles/r06/c3_instrument.txt)
          aa[(size_t)f * na + pos] = AdjAngle{c1m_d[(size_t)f * na + a], c1p_d[(size_t)f * na + a], q.rinv, q.dq, q.k0, a, q.inv < 0.f ? 1 : 0, 0};
          wg[(size_t)f * na + pos] = wadj[(size_t)f * na + a];
          const float wa = wadj[(size_t)f * na + a];
          const int wbits = __builtin_bit_cast(int, wa);
          pos_of[(size_t)f * na + a] = int4{f * na + pos, wbits, q.inv < 0.f ? 1 : 0, 0};
          ++pos;
        }
        if (pass == 0) n0[f] = pos;
      }
    }
    up((void**)&im->adj_ang, aa.data(), sizeof(AdjAngle) * n_ang);
    up((void**)&im->adj_wgt, wg.data(), sizeof(float) * n_ang);
    up((void**)&im->adj_n0, n0.data(), sizeof(int) * nt);
    up((void**)&im->rec, nullptr, sizeof(uint4) * (size_t)n_ang * ndp);
    up((void**)&im->adj_pos, pos_of.data(), sizeof(int4) * n_ang);
    const int64_t t16 = (int64_t)ceil_div(N, 16) * ceil_div(N, 16) * nt, pb = ceil_div((int64_t)n_ang * ndp, 256);
    im->pend_cap = t16 > pb ? t16 : pb;
    up((void**)&im->pend_buf[0], nullptr, sizeof(double) * (size_t)im->pend_cap);
    up((void**)&im->pend_buf[1], nullptr, sizeof(double) * (size_t)im->pend_cap);
  }
  if (e != hipSuccess) {
    trk_op tmp{2, 0, 0, im, nullptr, nullptr, nullptr, 0};
    radon_destroy(&tmp);
    return fail(TRK_EHIP, "trk_radon2d_create: %s", hipGetErrorString(e));
  }
  *out = new trk_op{2, (int64_t)n_ang * n_det, (int64_t)nt * N * N, im, radon_apply, radon_destroy, nullptr, 0};
  (*out)->apply_axpby = radon_apply_axpby;
  (*out)->flush = radon_flush;
  (*out)->apply_fused = radon_apply_fused;
  (*out)->fused_caps = 2;                  // raw block partials only, no two-operand form
  return TRK_OK;
}

namespace trk {
bool radon_ref_geometry(trk_op* op, RadonRefGeom* g) {
  if (!op || op->kind != 2 || op->apply != radon_apply) return false;
  radon_ref_geom_of(static_cast<RadonImpl*>(op->impl), g);
  return true;
}
}  // namespace trk

extern "C" int trk_radon2d_set_arithmetic(trk_op* op, int mode) {
  TRK_REQUIRE(op && op->kind == 2 && op->apply == radon_apply, "trk_radon2d_set_arithmetic: not a parallel-beam handle");
  TRK_REQUIRE(mode >= 0 && mode <= 2, "trk_radon2d_set_arithmetic: mode 0 (product), 1 (float64 geometry and sums) or 2 (table weights, float64 sums)");
  auto* im = static_cast<RadonImpl*>(op->impl);
  if (im->pend_target) return fail(TRK_EINVAL, "trk_radon2d_set_arithmetic: a deferred norm is pending (trk_op_flush first)");
  im->ref_mode = mode;
  im->rec_src = nullptr;
  im->xT_src = nullptr;
  return TRK_OK;
}

extern "C" int trk_radon2d_set_ref_sums(trk_op* op, int chunk_fwd, int chunk_adj) {
  TRK_REQUIRE(op && op->kind == 2 && op->apply == radon_apply, "trk_radon2d_set_ref_sums: not a parallel-beam handle");
  TRK_REQUIRE(chunk_fwd >= 0 && chunk_adj >= -2, "trk_radon2d_set_ref_sums: chunk_fwd >= 0, chunk_adj >= 0 (0 = float64 sums) or -1 / -2 (the product's neighbour rule)");
  auto* im = static_cast<RadonImpl*>(op->impl);
  im->ref_chunk_fwd = chunk_fwd;
  im->ref_chunk_adj = chunk_adj;
  return TRK_OK;
}

extern "C" int trk_radon2d_create(int N, int n_det, const double* angles, int n_ang, double scale, trk_op** out) {
  TRK_REQUIRE(out && angles, "trk_radon2d_create: NULL argument");
  TRK_REQUIRE(N >= 1 && n_det >= 1 && n_ang >= 1, "trk_radon2d_create: sizes must be >= 1");
  return radon_create_impl(N, n_det, angles, 1, n_ang, scale, out);
}

extern "C" int trk_radon2d_dynamic_create(int N, int n_det, const double* angles, int n_frames, int n_ang_per_frame,
                                          double scale, trk_op** out) {
  TRK_REQUIRE(out && angles, "trk_radon2d_dynamic_create: NULL argument");
  TRK_REQUIRE(N >= 1 && n_det >= 1 && n_frames >= 1 && n_ang_per_frame >= 1, "trk_radon2d_dynamic_create: sizes must be >= 1");
  return radon_create_impl(N, n_det, angles, n_frames, n_ang_per_frame, scale, out);
}