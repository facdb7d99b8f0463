// cgls_update.hip — the vector updates of a CGLS iteration (CGLS.py:64-79), streaming kernels in the style of vecops.hip that
// carry the iteration's scalars on the device; cgls_loop.hip chains them with the operator's launches.
#include "vec_internal.h"

using namespace trk;

namespace {

// ------------------------------------------------------------------ one CGLS iterate step on values held in registers
// x' = fl32(x + step * p): ONE rounding, fmaf(step, p, x) — and d = fl32(step * p), rounded on its own, for ||d||^2 alone (x' is NOT
// x + d: the two differ in the last bit on about a fifth of general data).  The iterate's three norms are fed from x', d and
// x' - x_true (x_norms).  Every kernel of this file forms x' this way, vector body and scalar tail alike, spelled fmaf so that the
// compiler's contraction setting decides nothing (tests/test_gpu_vec_entrywise.py pins the form per kernel, body and tail).  ONE
// definition for k_cgls_xp_update and k_cgls_xs_update: the batched kernel has to leave the bits of the one-step kernel
// (tests/test_gpu_cgls_xbatch.py compares exactly).
// d = fl32(step * p) on four lanes, as two packed products
typedef float f2pk __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 d_step4(float4 pv, float step) {
  const f2pk lo = (f2pk){pv.x, pv.y} * step, hi = (f2pk){pv.z, pv.w} * step;
  return make_float4(lo[0], lo[1], hi[0], hi[1]);
}
__device__ __forceinline__ float x_step(float x, float p, float step, float& d) {
  d = step * p;
  return fmaf(step, p, x);
}
__device__ __forceinline__ float4 x_step4(float4 xv, float4 pv, float step, float4& d) {
  d = d_step4(pv, step);
  return make_float4(fmaf(step, pv.x, xv.x), fmaf(step, pv.y, xv.y), fmaf(step, pv.z, xv.z), fmaf(step, pv.w, xv.w));
}
template <bool HAS_XT>
__device__ __forceinline__ void x_norms(float xn, float d, float xt, double& s0, double& s1, double& s2) {
  s0 += (double)xn * xn;
  s1 += (double)d * d;
  if (HAS_XT) {
    const double e = (double)xn - xt;
    s2 += e * e;
  }
}
template <bool HAS_XT>
__device__ __forceinline__ void x_norms4(float4 xn, float4 d, float4 tt, double& s0, double& s1, double& s2) {
  s0 += (double)xn.x * xn.x + (double)xn.y * xn.y + (double)xn.z * xn.z + (double)xn.w * xn.w;
  s1 += (double)d.x * d.x + (double)d.y * d.y + (double)d.z * d.z + (double)d.w * d.w;
  if (HAS_XT) {
    const double e0 = (double)xn.x - tt.x, e1 = (double)xn.y - tt.y, e2 = (double)xn.z - tt.z, e3 = (double)xn.w - tt.w;
    s2 += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
  }
}
// p' = fl32(t + b * p): ONE rounding as well, fmaf(b, p, t) (trk_axpby(1, t, b, p) rounds b * p on its own)
__device__ __forceinline__ float p_step(float t, float p, float b) { return fmaf(b, p, t); }
__device__ __forceinline__ float4 p_step4(float4 tv, float4 pv, float b) {
  return make_float4(fmaf(b, pv.x, tv.x), fmaf(b, pv.y, tv.y), fmaf(b, pv.z, tv.z), fmaf(b, pv.w, tv.w));
}

// ------------------------------------------------------------------ fused CGLS update (CGLS.py:64-67,76,79)
// x_new = fmaf(step, p, x) and r = fmaf(-step, w, r) with step = (float)(gamma / delta): one rounding each
// partials layout: [block][3] = ||x_new||^2, ||fl32(step*p)||^2, ||x_new - x_true||^2
template <bool HAS_XT, bool VEC>
__global__ __launch_bounds__(NT) void k_cgls_update(int64_t n, int64_t m, ScalarSrc gamma, ScalarSrc delta,
                                                    const float* x, const float* p, float* x_new, float* r,
                                                    const float* w, const float* x_true, double* __restrict__ partials,
                                                    double* pub_delta, int nt) {
  __shared__ double lds[NT / 64];
  __shared__ double bc;
  float step;
  if (gamma.n == 1 && delta.n == 1) {                // finished scalars (grid-uniform)
    step = (float)(*gamma.p / *delta.p);
    if (blockIdx.x == 0 && threadIdx.x == 0 && pub_delta && pub_delta != delta.p) *pub_delta = *delta.p;   // a one-block producer
  } else {                                           // block partials of the producing kernel: one wave sums them
    if (threadIdx.x < 64) {
      const double g = scalar_from_wave(gamma, threadIdx.x), d = scalar_from_wave(delta, threadIdx.x);
      if (threadIdx.x == 0) {
        bc = g / d;
        if (blockIdx.x == 0 && pub_delta) *pub_delta = d;
      }
    }
    __syncthreads();
    step = (float)bc;
  }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t ntail = 0, mtail = 0;
  if (VEC) {
    const int64_t n4 = n >> 2, m4 = m >> 2;
    ntail = n4 << 2;
    mtail = m4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 xv = ld4(x, i), pv = ld4(p, i);
      const float4 d = d_step4(pv, step);
      const float4 xn = make_float4(fmaf(step, pv.x, xv.x), fmaf(step, pv.y, xv.y), fmaf(step, pv.z, xv.z), fmaf(step, pv.w, xv.w));
      if (nt & 2) st4_nt(x_new, i, xn); else st4(x_new, i, xn);
      s0 += (double)xn.x * xn.x + (double)xn.y * xn.y + (double)xn.z * xn.z + (double)xn.w * xn.w;
      s1 += (double)d.x * d.x + (double)d.y * d.y + (double)d.z * d.z + (double)d.w * d.w;
      if (HAS_XT) {
        const float4 t = ld4(x_true, i);
        const double e0 = (double)xn.x - t.x, e1 = (double)xn.y - t.y, e2 = (double)xn.z - t.z, e3 = (double)xn.w - t.w;
        s2 += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
      }
    }
    for (int64_t i = tid; i < m4; i += nth) {
      float4 rv = ld4(r, i);
      const float4 wv = ld4(w, i);
      rv.x = fmaf(-step, wv.x, rv.x);
      rv.y = fmaf(-step, wv.y, rv.y);
      rv.z = fmaf(-step, wv.z, rv.z);
      rv.w = fmaf(-step, wv.w, rv.w);
      st4(r, i, rv);
    }
  }
  for (int64_t i = ntail + tid; i < n; i += nth) {
    const float pi = p[i], d = step * pi;
    const float xn = fmaf(step, pi, x[i]);
    x_new[i] = xn;
    s0 += (double)xn * xn;
    s1 += (double)d * d;
    if (HAS_XT) {
      const double e = (double)xn - x_true[i];
      s2 += e * e;
    }
  }
  for (int64_t i = mtail + tid; i < m; i += nth) r[i] = fmaf(-step, w[i], r[i]);
  s0 = block_sum<NT>(s0, lds);
  s1 = block_sum<NT>(s1, lds);
  if (HAS_XT) s2 = block_sum<NT>(s2, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x * 3 + 0] = s0;
    partials[blockIdx.x * 3 + 1] = s1;
    partials[blockIdx.x * 3 + 2] = HAS_XT ? s2 : 0.0;
  }
}

// ------------------------------------------------------------------ CGLS direction update (CGLS.py:72)
// p_out = fmaf(b, p, t), b = (float)(gamma_new / gamma_old), with gamma_new possibly still the block partials of the adjoint kernel that produced
// t; block 0 publishes the finished gamma_new.  One rounding (trk_axpby(1, t, b, p) rounds b p on its own).  p_out may be p.
// nt: bit 0 loads t, bit 1 loads p non-temporally — set when p_out is another buffer (the ring of trk_cgls_iterate_xbatch): neither
// input is read again soon, and kept out of the caches they leave p_out there for the forward blur that follows (4096^2, s = 8: that
// blur launch 26.3 -> 23.0 us, what it takes behind the in-place update; 7.68 k -> 7.82 k iterations/s, 5120^2 4.64 k -> 5.05 k).
template <bool VEC>
__global__ __launch_bounds__(NT) void k_cgls_p_update(int64_t n, const float* __restrict__ t, const float* p, float* p_out,
                                                      ScalarSrc gnew, const double* gold, double* pub_gamma, int nt) {
  __shared__ double bc;
  if (threadIdx.x < 64) {
    const double g = scalar_from_wave(gnew, threadIdx.x);
    if (threadIdx.x == 0) {
      bc = g / *gold;
      if (blockIdx.x == 0 && pub_gamma) *pub_gamma = g;
    }
  }
  __syncthreads();
  const float b = (float)bc;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail0 = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 v = (nt & 1) ? ld4_nt(t, i) : ld4(t, i), w = (nt & 2) ? ld4_nt(p, i) : ld4(p, i);
      if (nt & 4) st4_nt(p_out, i, p_step4(v, w, b)); else st4(p_out, i, p_step4(v, w, b));
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += nth) p_out[i] = p_step(t[i], p[i], b);
}

// ------------------------------------------------------------------ CGLS residual update alone (CGLS.py:67)
// r -= (gamma_old / S(delta)) w with delta possibly still the block partials of the forward kernel; block 0 publishes it.
template <bool VEC>
__global__ __launch_bounds__(NT) void k_cgls_r_update(int64_t m, const double* gold, ScalarSrc delta, float* r,
                                                      const float* __restrict__ w, double* pub_delta) {
  __shared__ double bc;
  if (threadIdx.x < 64) {
    const double d = scalar_from_wave(delta, threadIdx.x);
    if (threadIdx.x == 0) {
      bc = *gold / d;
      if (blockIdx.x == 0 && pub_delta) *pub_delta = d;
    }
  }
  __syncthreads();
  const float step = (float)bc;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail0 = 0;
  if (VEC) {
    const int64_t m4 = m >> 2;
    tail0 = m4 << 2;
    for (int64_t i = tid; i < m4; i += nth) {
      float4 rv = ld4(r, i);
      const float4 wv = ld4(w, i);
      rv.x = fmaf(-step, wv.x, rv.x);
      rv.y = fmaf(-step, wv.y, rv.y);
      rv.z = fmaf(-step, wv.z, rv.z);
      rv.w = fmaf(-step, wv.w, rv.w);
      st4(r, i, rv);
    }
  }
  for (int64_t i = tail0 + tid; i < m; i += nth) r[i] = fmaf(-step, w[i], r[i]);
}

// ------------------------------------------------------------------ CGLS iterate + direction update in one pass over p
// x_new = fmaf((float)(gamma_old/delta), p, x) (CGLS.py:64-65; one rounding) and p = fmaf((float)(S(gamma_new)/gamma_old), p, t) (:72): p is read once for both
// (20n bytes instead of 12n + 12n); norms as k_cgls_update: [block][3] raw partials; block 0 publishes gamma_new.
template <bool HAS_XT>
__global__ __launch_bounds__(NT) void k_cgls_xp_update(int64_t n, const double* gold, const double* delta, ScalarSrc gnew,
                                                       const float* __restrict__ x, float* p, const float* __restrict__ t,
                                                       float* __restrict__ x_new, const float* __restrict__ x_true,
                                                       double* pub_gamma, double* __restrict__ partials, int nt) {
  __shared__ double lds[NT / 64];
  __shared__ double bc[2];
  if (threadIdx.x < 64) {
    const double g = scalar_from_wave(gnew, threadIdx.x);
    if (threadIdx.x == 0) {
      bc[0] = *gold / *delta;
      bc[1] = g / *gold;
      if (blockIdx.x == 0 && pub_gamma) *pub_gamma = g;
    }
  }
  __syncthreads();
  const float step = (float)bc[0], b = (float)bc[1];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  const int64_t n4 = n >> 2;
  for (int64_t i = tid; i < n4; i += nth) {
    const float4 xv = (nt & 16) ? ld4_nt(x, i) : ld4(x, i), pv = ld4(p, i), tv = (nt & 32) ? ld4_nt(t, i) : ld4(t, i);
    float4 d;
    const float4 xn = x_step4(xv, pv, step, d);
    if (nt & 2) st4_nt(x_new, i, xn); else st4(x_new, i, xn);
    st4(p, i, p_step4(tv, pv, b));
    x_norms4<HAS_XT>(xn, d, HAS_XT ? ld4(x_true, i) : make_float4(0.f, 0.f, 0.f, 0.f), s0, s1, s2);
  }
  for (int64_t i = (n4 << 2) + tid; i < n; i += nth) {
    const float pv = p[i];
    float d;
    const float xn = x_step(x[i], pv, step, d);
    x_new[i] = xn;
    p[i] = p_step(t[i], pv, b);
    x_norms<HAS_XT>(xn, d, HAS_XT ? x_true[i] : 0.f, s0, s1, s2);
  }
  s0 = block_sum<NT>(s0, lds);
  s1 = block_sum<NT>(s1, lds);
  if (HAS_XT) s2 = block_sum<NT>(s2, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x * 3 + 0] = s0;
    partials[blockIdx.x * 3 + 1] = s1;
    partials[blockIdx.x * 3 + 2] = HAS_XT ? s2 : 0.0;
  }
}

// ------------------------------------------------------------------ C deferred iterate steps + direction update in one pass
// Without a history nobody reads x_{k-C+1} .. x_{k-1}, and x never feeds back into the recurrence: the directions of C iterations are
// kept (trk_cgls_p_update_to writes each new one beside the old) and this kernel forms x_{k-C+1} .. x_k from x_{k-C} in registers —
// the same fp32 operations in the same order as C launches of k_cgls_xp_update (x_step4) — accumulates the three norms of every one of
// them and writes x ONCE: (C-1) of C writes of x are not made.  step_j = gamma_{j-1} / delta_j from the finished scalars in S (rows
// k-C+1 .. k, all published by earlier launches); the direction update p_out = fmaf((float)(S(gamma_new) / gamma_{k-1}), p_k, t) and the published
// gamma_k as k_cgls_xp_update.  Partials: iteration j's [block][3] at partials + (j - (k-C+1)) * slice.  x_new may be x and p_out any of
// the directions (an element is read and then written by the same thread): no __restrict__ on them.
// Cache hints of its own (bits beside those of stream_nontemporal(), set when C > 1): 256 = the directions before the last are loaded
// non-temporally (each is read here for the last time); 512 / 1024 = so is the last one, and p_out is stored non-temporally — unless
// p_out IS the last direction: updated in place like k_cgls_xp_update's p it stays cached for the forward blur that follows.
// Measured, iterations/s at s = 8 with the p-update's load hints on, 4096^2 / 5120^2: no hints 7.82 k / 5.05 k, 256: 7.99 k / 5.17 k,
// 256 | 512 | 1024 with p_out in another slot 8.04 k / 5.20 k (k_cgls_xs_update<8> itself 164 -> 135 us at 4096^2 = 12 x 67 MB at
// 6.0 TB/s); x and t loaded non-temporally below stream_nontemporal()'s size as well: 7.97 k, no gain.
// In place instead (the slots used round-robin): the same rate, 8.09 k at 4096^2, and the forward blur behind the kernel back from 30.3 to
// 23.5 us (k_cgls_xs_update<8> 135 -> 140 us).
// With p_out in place, t (bit 5 of stream_nontemporal()'s mask) loaded non-temporally too: the blur behind the kernel 23.8 -> 22.9 us,
// the kernel 141 -> 136 us, 8.01 k -> 8.09 k at 4096^2 (3072^2 12.70 k -> 12.69 k, 4608^2 6.42 k -> 6.39 k); x as well: 8.07 k.
constexpr int kXsOldDirs = 256 | 32, kXsLastDirAndOut = 512 | 1024;
constexpr int XS_MAX = 8;
struct XsDirs {
  const float* p[XS_MAX];                 // p_{k-C+1} .. p_k
};

// XONLY (trk_cgls_xs_update_x, the recomputing loop): the x updates and their norms alone — no t is loaded, no p_out stored, no gamma_new
// summed or published; the last direction is read again soon (the adjoint's epilogue) and is loaded plainly.
template <bool HAS_XT, int C, bool XONLY = false>
__global__ __launch_bounds__(NT) void k_cgls_xs_update(int64_t n, const double* S, int k, ScalarSrc gnew, const float* x, XsDirs dirs,
                                                       const float* __restrict__ t, float* x_new, float* p_out,
                                                       const float* __restrict__ x_true, double* pub_gamma,
                                                       double* __restrict__ partials, int64_t slice, int nt) {
  __shared__ double lds[NT / 64];
  __shared__ double bc[C + 1];
  if (threadIdx.x < 64) {
    const double g = XONLY ? 0.0 : scalar_from_wave(gnew, threadIdx.x);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int j = k - C + 1 + c;
        const double* gold = (j == 1) ? S : S + 5 * (int64_t)(j - 1) + 1;
        bc[c] = *gold / S[5 * (int64_t)j];
      }
      if (!XONLY) {
        bc[C] = g / *((k == 1) ? S : S + 5 * (int64_t)(k - 1) + 1);
        if (blockIdx.x == 0 && pub_gamma) *pub_gamma = g;
      }
    }
  }
  __syncthreads();
  float step[C];
#pragma unroll
  for (int c = 0; c < C; ++c) step[c] = (float)bc[c];
  const float b = XONLY ? 0.f : (float)bc[C];
  double s0[C], s1[C], s2[C];
#pragma unroll
  for (int c = 0; c < C; ++c) s0[c] = s1[c] = s2[c] = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  const int64_t n4 = n >> 2;
  for (int64_t i = tid; i < n4; i += nth) {
    float4 xv = (nt & 16) ? ld4_nt(x, i) : ld4(x, i);
    float4 pv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) pv[c] = (nt & (c < C - 1 ? 256 : 512)) ? ld4_nt(dirs.p[c], i) : ld4(dirs.p[c], i);
    float4 tv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!XONLY) tv = (nt & 32) ? ld4_nt(t, i) : ld4(t, i);
    const float4 tt = HAS_XT ? ld4(x_true, i) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float4 d;
      xv = x_step4(xv, pv[c], step[c], d);
      x_norms4<HAS_XT>(xv, d, tt, s0[c], s1[c], s2[c]);
    }
    if (nt & 2) st4_nt(x_new, i, xv); else st4(x_new, i, xv);
    if (!XONLY) {
      if (nt & 1024) st4_nt(p_out, i, p_step4(tv, pv[C - 1], b)); else st4(p_out, i, p_step4(tv, pv[C - 1], b));
    }
  }
  for (int64_t i = (n4 << 2) + tid; i < n; i += nth) {
    float xv = x[i];
    float pv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) pv[c] = dirs.p[c][i];
    const float tv = XONLY ? 0.f : t[i], tt = HAS_XT ? x_true[i] : 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float d;
      xv = x_step(xv, pv[c], step[c], d);
      x_norms<HAS_XT>(xv, d, tt, s0[c], s1[c], s2[c]);
    }
    x_new[i] = xv;
    if (!XONLY) p_out[i] = p_step(tv, pv[C - 1], b);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double a0 = block_sum<NT>(s0[c], lds), a1 = block_sum<NT>(s1[c], lds);
    const double a2 = HAS_XT ? block_sum<NT>(s2[c], lds) : 0.0;
    if (threadIdx.x == 0) {
      double* out = partials + c * slice + blockIdx.x * 3;
      out[0] = a0;
      out[1] = a1;
      out[2] = a2;
    }
  }
}

// ------------------------------------------------------------------ CGLS x-update of the fused fast path
// x_new = fmaf((float)(gamma/delta), p, x) (one rounding) with gamma, delta possibly still block partials of the producing blur kernels; block 0
// publishes the two finished scalars; the three norms are left as raw partials [block][3] (summed once, after the solve).
template <bool HAS_XT>
__global__ __launch_bounds__(NT) void k_cgls_x_update(int64_t n, ScalarSrc gamma, ScalarSrc delta, const float* __restrict__ x,
                                                      const float* __restrict__ p, float* __restrict__ x_new,
                                                      const float* __restrict__ x_true, double* pub_delta,
                                                      double* pub_gamma, double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  __shared__ double bc[2];
  if (threadIdx.x < 64) {                          // one wave evaluates both scalars (fixed summation order)
    const double g = scalar_from_wave(gamma, threadIdx.x), d = scalar_from_wave(delta, threadIdx.x);
    if (threadIdx.x == 0) {
      bc[0] = g;
      bc[1] = d;
      if (blockIdx.x == 0) {
        if (pub_gamma) *pub_gamma = g;
        if (pub_delta) *pub_delta = d;
      }
    }
  }
  __syncthreads();
  const float step = (float)(bc[0] / bc[1]);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  const int64_t n4 = n >> 2;
  for (int64_t i = tid; i < n4; i += nth) {
    const float4 xv = ld4(x, i), pv = ld4(p, i);
    const float4 d = d_step4(pv, step);
    const float4 xn = make_float4(fmaf(step, pv.x, xv.x), fmaf(step, pv.y, xv.y), fmaf(step, pv.z, xv.z), fmaf(step, pv.w, xv.w));
    st4(x_new, i, xn);
    s0 += (double)xn.x * xn.x + (double)xn.y * xn.y + (double)xn.z * xn.z + (double)xn.w * xn.w;
    s1 += (double)d.x * d.x + (double)d.y * d.y + (double)d.z * d.z + (double)d.w * d.w;
    if (HAS_XT) {
      const float4 t = ld4(x_true, i);
      const double e0 = (double)xn.x - t.x, e1 = (double)xn.y - t.y, e2 = (double)xn.z - t.z, e3 = (double)xn.w - t.w;
      s2 += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
    }
  }
  for (int64_t i = (n4 << 2) + tid; i < n; i += nth) {
    const float pi = p[i], d = step * pi;
    const float xn = fmaf(step, pi, x[i]);
    x_new[i] = xn;
    s0 += (double)xn * xn;
    s1 += (double)d * d;
    if (HAS_XT) {
      const double e = (double)xn - x_true[i];
      s2 += e * e;
    }
  }
  s0 = block_sum<NT>(s0, lds);
  s1 = block_sum<NT>(s1, lds);
  if (HAS_XT) s2 = block_sum<NT>(s2, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x * 3 + 0] = s0;
    partials[blockIdx.x * 3 + 1] = s1;
    partials[blockIdx.x * 3 + 2] = HAS_XT ? s2 : 0.0;
  }
}

// the C = count instantiation of k_cgls_xs_update (count in 1 .. XS_MAX)
template <int C = XS_MAX, class... Args>
void launch_xs(int count, bool has_xt, int grid, hipStream_t s, Args... args) {
  if (count == C) {
    with_bools([&](auto HAS_XT) { hipLaunchKernelGGL((k_cgls_xs_update<HAS_XT, C>), dim3(grid), dim3(NT), 0, s, args...); }, has_xt);
  } else if constexpr (C > 1) {
    launch_xs<C - 1>(count, has_xt, grid, s, args...);
  }
}
template <int C = XS_MAX, class... Args>
void launch_xs_x(int count, bool has_xt, int grid, hipStream_t s, Args... args) {
  if (count == C) {
    with_bools([&](auto HAS_XT) { hipLaunchKernelGGL((k_cgls_xs_update<HAS_XT, C, true>), dim3(grid), dim3(NT), 0, s, args...); }, has_xt);
  } else if constexpr (C > 1) {
    launch_xs_x<C - 1>(count, has_xt, grid, s, args...);
  }
}

}  // namespace

// ======================================================================================= C ABI
extern "C" {

int trk_cgls_update_xr(int64_t n, int64_t m, const double* gamma, const double* delta, const float* x, const float* p,
                       float* x_new, float* r, const float* w, const float* x_true, double* sums, trk_stream st) {
  TRK_REQUIRE(gamma && delta && x && p && x_new && r && w && sums, "trk_cgls_update_xr: NULL argument");
  TRK_REQUIRE(n >= 0 && m >= 0, "trk_cgls_update_xr: negative size");
  hipStream_t s = (hipStream_t)st;
  const int grid = stream_grid(n > m ? n : m);
  double* part = nullptr;
  if (int rc = scratch_doubles(s, (size_t)grid * 3, &part)) return rc;
  const bool vec = aligned16(x) && aligned16(p) && aligned16(x_new) && aligned16(r) && aligned16(w) &&
                   (!x_true || aligned16(x_true));
  with_bools([&](auto HAS_XT, auto VEC) {
    hipLaunchKernelGGL((k_cgls_update<HAS_XT, VEC>), dim3(grid), dim3(NT), 0, s, n, m, ScalarSrc{gamma, 1}, ScalarSrc{delta, 1}, x, p, x_new,
                       r, w, x_true, part, (double*)nullptr, stream_nontemporal(n));
  }, x_true != nullptr, vec);
  TRK_LAUNCH_CHECK();
  return finalize_sums(part, grid, 3, 3, sums, s);
}

int trk_cgls_update_xr_deferred(int64_t n, int64_t m, const double* gamma, const double* delta, const float* x,
                                const float* p, float* x_new, float* r, const float* w, const float* x_true,
                                double* norm_partials, int capacity_blocks, int* n_blocks, trk_stream st) {
  return trk_cgls_update_xr_src(n, m, gamma, 1, delta, 1, x, p, x_new, r, w, x_true, nullptr, norm_partials,
                                capacity_blocks, n_blocks, st);
}

int trk_cgls_update_xr_src(int64_t n, int64_t m, const double* gamma, int gamma_n, const double* delta, int delta_n,
                           const float* x, const float* p, float* x_new, float* r, const float* w, const float* x_true,
                           double* publish_delta, double* norm_partials, int capacity_blocks, int* n_blocks,
                           trk_stream st) {
  TRK_REQUIRE(gamma && delta && gamma_n >= 1 && delta_n >= 1 && x && p && x_new && r && w && norm_partials && n_blocks,
              "trk_cgls_update_xr_src: NULL argument");
  TRK_REQUIRE(n >= 0 && m >= 0, "trk_cgls_update_xr_src: negative size");
  hipStream_t s = (hipStream_t)st;
  const int grid = stream_grid(n > m ? n : m);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_cgls_update_xr_src: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  const bool vec = aligned16(x) && aligned16(p) && aligned16(x_new) && aligned16(r) && aligned16(w) &&
                   (!x_true || aligned16(x_true));
  const ScalarSrc g{gamma, gamma_n}, d{delta, delta_n};
  with_bools([&](auto HAS_XT, auto VEC) {
    hipLaunchKernelGGL((k_cgls_update<HAS_XT, VEC>), dim3(grid), dim3(NT), 0, s, n, m, g, d, x, p, x_new, r, w, x_true, norm_partials,
                       publish_delta, stream_nontemporal(n));
  }, x_true != nullptr, vec);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_cgls_p_update_to(int64_t n, const float* t, const float* p, float* p_out, const double* gamma_new, int gamma_new_n,
                         const double* gamma_old, double* publish_gamma, trk_stream st) {
  TRK_REQUIRE(t && p && p_out && gamma_new && gamma_new_n >= 1 && gamma_old && n >= 0, "trk_cgls_p_update_to: bad argument");
  const int grid = stream_grid(n);
  const ScalarSrc g{gamma_new, gamma_new_n};
  hipStream_t s = (hipStream_t)st;
  with_bools([&](auto VEC) {
    hipLaunchKernelGGL((k_cgls_p_update<VEC>), dim3(grid), dim3(NT), 0, s, n, t, p, p_out, g, gamma_old, publish_gamma,
                       p == p_out ? 0 : 3);
  }, aligned16(t) && aligned16(p) && aligned16(p_out));
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_cgls_p_update(int64_t n, const float* t, float* p, const double* gamma_new, int gamma_new_n,
                      const double* gamma_old, double* publish_gamma, trk_stream st) {
  TRK_REQUIRE(t && p && gamma_new && gamma_new_n >= 1 && gamma_old && n >= 0, "trk_cgls_p_update: bad argument");
  return trk_cgls_p_update_to(n, t, p, p, gamma_new, gamma_new_n, gamma_old, publish_gamma, st);
}

int trk_cgls_r_update(int64_t m, const double* gamma_old, const double* delta, int delta_n, float* r, const float* w,
                      double* publish_delta, trk_stream st) {
  TRK_REQUIRE(gamma_old && delta && delta_n >= 1 && r && w && m >= 0, "trk_cgls_r_update: bad argument");
  const int grid = stream_grid(m);
  const ScalarSrc d{delta, delta_n};
  hipStream_t s = (hipStream_t)st;
  with_bools([&](auto VEC) { hipLaunchKernelGGL((k_cgls_r_update<VEC>), dim3(grid), dim3(NT), 0, s, m, gamma_old, d, r, w, publish_delta); },
             aligned16(r) && aligned16(w));
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_cgls_xp_update(int64_t n, const double* gamma_old, const double* delta, const double* gamma_new, int gamma_new_n,
                       const float* x, float* p, const float* t, float* x_new, const float* x_true, double* publish_gamma,
                       double* norm_partials, int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(gamma_old && delta && gamma_new && gamma_new_n >= 1 && x && p && t && x_new && norm_partials && n_blocks && n >= 0,
              "trk_cgls_xp_update: bad argument");
  TRK_REQUIRE(aligned16(x) && aligned16(p) && aligned16(t) && aligned16(x_new) && (!x_true || aligned16(x_true)),
              "trk_cgls_xp_update: vectors must be 16-byte aligned");
  const int grid = stream_grid(n);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_cgls_xp_update: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  const ScalarSrc g{gamma_new, gamma_new_n};
  hipStream_t s = (hipStream_t)st;
  with_bools([&](auto HAS_XT) {
    hipLaunchKernelGGL((k_cgls_xp_update<HAS_XT>), dim3(grid), dim3(NT), 0, s, n, gamma_old, delta, g, x, p, t, x_new, x_true, publish_gamma,
                       norm_partials, stream_nontemporal(n));
  }, x_true != nullptr);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_cgls_xs_update(int64_t n, int count, int k_last, double* S, const double* gamma_new, int gamma_new_n, const float* x,
                       const float* p, const float* ring, int64_t ring_ld, int s_slots, int first, const float* t, float* x_new,
                       float* p_out, const float* x_true, double* NP, int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(S && gamma_new && gamma_new_n >= 1 && x && p && t && x_new && p_out && NP && n_blocks && n >= 0,
              "trk_cgls_xs_update: bad argument");
  TRK_REQUIRE(count >= 1 && count <= XS_MAX && count <= k_last, "trk_cgls_xs_update: need 1 <= count <= %d and count <= k_last", XS_MAX);
  TRK_REQUIRE(s_slots >= count && first >= 0 && first < s_slots && (s_slots == 1 || (ring && ring_ld >= n)),
              "trk_cgls_xs_update: need count <= s_slots, 0 <= first < s_slots and a ring of s_slots - 1 directions");
  XsDirs dirs{};
  for (int c = 0; c < count; ++c) {
    const int slot = (first + c) % s_slots;                  // slot 0 is p, slot j the ring's row j - 1
    dirs.p[c] = slot == 0 ? p : ring + (int64_t)(slot - 1) * ring_ld;
  }
  bool al = aligned16(x) && aligned16(t) && aligned16(x_new) && aligned16(p_out) && (!x_true || aligned16(x_true));
  for (int c = 0; c < count; ++c) al = al && aligned16(dirs.p[c]);
  TRK_REQUIRE(al, "trk_cgls_xs_update: vectors must be 16-byte aligned");
  const int grid = stream_grid(n);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_cgls_xs_update: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  const ScalarSrc g{gamma_new, gamma_new_n};
  hipStream_t s = (hipStream_t)st;
  const int64_t slice = 3 * (int64_t)grid;
  double* part = NP + slice * (k_last - count);              // iteration j's slice: NP + 3 * grid * (j - 1)
  double* pub = S + 5 * (int64_t)k_last + 1;
  const int nt = stream_nontemporal(n) | (count > 1 ? kXsOldDirs | (p_out == dirs.p[count - 1] ? 0 : kXsLastDirAndOut) : 0);
  launch_xs(count, x_true != nullptr, grid, s, n, (const double*)S, k_last, g, x, dirs, t, x_new, p_out, x_true, pub, part, slice, nt);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_cgls_xs_update_x(int64_t n, int count, int k_last, const double* S, const float* x, const float* p, const float* ring,
                         int64_t ring_ld, int s_slots, int first, float* x_new, const float* x_true, double* NP,
                         int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(S && x && p && x_new && NP && n_blocks && n >= 0, "trk_cgls_xs_update_x: bad argument");
  TRK_REQUIRE(count >= 1 && count <= XS_MAX && count <= k_last, "trk_cgls_xs_update_x: need 1 <= count <= %d and count <= k_last", XS_MAX);
  TRK_REQUIRE(s_slots >= count && first >= 0 && first < s_slots && (s_slots == 1 || (ring && ring_ld >= n)),
              "trk_cgls_xs_update_x: need count <= s_slots, 0 <= first < s_slots and a ring of s_slots - 1 directions");
  XsDirs dirs{};
  for (int c = 0; c < count; ++c) {
    const int slot = (first + c) % s_slots;                  // slot 0 is p, slot j the ring's row j - 1
    dirs.p[c] = slot == 0 ? p : ring + (int64_t)(slot - 1) * ring_ld;
  }
  bool al = aligned16(x) && aligned16(x_new) && (!x_true || aligned16(x_true));
  for (int c = 0; c < count; ++c) al = al && aligned16(dirs.p[c]);
  TRK_REQUIRE(al, "trk_cgls_xs_update_x: vectors must be 16-byte aligned");
  const int grid = stream_grid(n);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_cgls_xs_update_x: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  hipStream_t s = (hipStream_t)st;
  const int64_t slice = 3 * (int64_t)grid;
  double* part = NP + slice * (k_last - count);              // iteration j's slice: NP + 3 * grid * (j - 1)
  // the directions before the last are read here for the last time; the last one is the z of the adjoint's epilogue two launches on
  const int nt = (stream_nontemporal(n) & ~32) | (count > 1 ? 256 : 0);
  launch_xs_x(count, x_true != nullptr, grid, s, n, S, k_last, ScalarSrc{nullptr, 0}, x, dirs, (const float*)nullptr, x_new,
              (float*)nullptr, x_true, (double*)nullptr, part, slice, nt);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_cgls_x_update(int64_t n, const double* gamma, int gamma_n, const double* delta, int delta_n, const float* x,
                      const float* p, float* x_new, const float* x_true, double* publish_delta, double* publish_gamma,
                      double* norm_partials, int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(gamma && delta && gamma_n >= 1 && delta_n >= 1 && x && p && x_new && norm_partials && n_blocks,
              "trk_cgls_x_update: NULL argument");
  TRK_REQUIRE(aligned16(x) && aligned16(p) && aligned16(x_new) && (!x_true || aligned16(x_true)),
              "trk_cgls_x_update: vectors must be 16-byte aligned");
  const int grid = stream_grid(n);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_cgls_x_update: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  const ScalarSrc g{gamma, gamma_n}, d{delta, delta_n};
  hipStream_t s = (hipStream_t)st;
  with_bools([&](auto HAS_XT) {
    hipLaunchKernelGGL((k_cgls_x_update<HAS_XT>), dim3(grid), dim3(NT), 0, s, n, g, d, x, p, x_new, x_true, publish_delta, publish_gamma,
                       norm_partials);
  }, x_true != nullptr);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

}  // extern "C"
