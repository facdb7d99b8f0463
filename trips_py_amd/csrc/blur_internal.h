// blur_internal.h — what the blur's kernel files share (blur2d.hip: sliding, strip and generic kernels, the handle;
// blur_tile.hip: the LDS tile kernel for any PSF up to 64x64): the handle's data, the boundary index maps, the path rule.
#pragma once
#include "trk_internal.h"

#include <type_traits>

namespace trk {

typedef float f4 __attribute__((ext_vector_type(4)));  // one 16-byte register quad: keeps loads/stores as b128

__host__ __device__ constexpr int rup4(int v) { return (v + 3) & ~3; }

__device__ __forceinline__ int reflect(int i, int n) {
  // half-sample symmetric extension, any distance; in-range indices (the common case) skip the division
  if ((unsigned)i < (unsigned)n) return i;
  const int p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return (i >= n) ? (p - 1 - i) : i;
}

// boundary modes: the values of trk.h's TRK_BOUNDARY_*
enum Bc : int { BC_REFLECT = 0, BC_CONSTANT = 1, BC_NEAREST = 2, BC_MIRROR = 3, BC_WRAP = 4 };

// image index of sample i of a length-n line extended by mode BC, at any distance; -1 for a constant-mode sample outside
// (the caller reads 0 there and forms no address)
template <int BC>
__device__ __forceinline__ int bmap(int i, int n) {
  if constexpr (BC == BC_REFLECT) {
    return reflect(i, n);
  } else {
    if ((unsigned)i < (unsigned)n) return i;
    if constexpr (BC == BC_CONSTANT) {
      return -1;
    } else if constexpr (BC == BC_NEAREST) {
      return i < 0 ? 0 : n - 1;
    } else if constexpr (BC == BC_WRAP) {
      i %= n;
      return i < 0 ? i + n : i;
    } else {   // BC_MIRROR: whole-sample symmetric, period 2n-2 (n = 1: the one sample)
      if (n == 1) return 0;
      const int p = 2 * n - 2;
      i %= p;
      if (i < 0) i += p;
      return (i >= n) ? (p - i) : i;
    }
  }
}

// one sample of row `row` (length n) at column j under mode BC
template <int BC>
__device__ __forceinline__ float bload(const float* row, int j, int n) {
  const int g = bmap<BC>(j, n);
  if constexpr (BC == BC_CONSTANT)
    if (g < 0) return 0.f;
  return row[g];
}

template <class F>
int bc_dispatch(int bc, F&& f) {   // run f with the mode as a compile-time constant
  switch (bc) {
    case BC_CONSTANT: return f(std::integral_constant<int, BC_CONSTANT>{});
    case BC_NEAREST: return f(std::integral_constant<int, BC_NEAREST>{});
    case BC_MIRROR: return f(std::integral_constant<int, BC_MIRROR>{});
    case BC_WRAP: return f(std::integral_constant<int, BC_WRAP>{});
    default: return f(std::integral_constant<int, BC_REFLECT>{});
  }
}

struct BlurImpl {
  int nx, ny, kh, kw;
  int bc;              // boundary mode (Bc)
  bool separable;
  bool tiled;          // a k_blur_strip instantiation exists for (kh,kw)
  float* w_dev[2];     // [kh*kw] correlation weights: 0 forward, 1 "transpose" (flipped PSF)
  float* sep_dev[2];   // [kw row weights | kh column weights]
  int forced;          // TRK_BLUR_PATH_AUTO, or the path trk_blur2d_set_path asked for (TILE / GENERIC)
};

// strips of `tw` columns x row bands: about 4 workgroups per CU, bands a whole number of `th`-row steps
inline void strip_grid(int nx, int ny, int batch, int tw, int th, int* strips_x, int* rows_per_band, int* nband) {
  const int sx = ceil_div(ny, tw), steps = ceil_div(nx, th);
  int want = (4 * cu_count()) / (sx * (batch > 0 ? batch : 1));
  if (want < 1) want = 1;
  if (want > steps) want = steps;
  const int steps_per_band = ceil_div(steps, want);
  *strips_x = sx;
  *rows_per_band = steps_per_band * th;
  *nband = ceil_div(nx, *rows_per_band);
}

// ------------------------------------------------------------------------------------------------ path rule
constexpr int kBlurTileMaxSide = 64;   // k_blur_tile: 1 <= kh, kw <= 64

// the sliding kernel's shapes: separable odd square PSFs up to 9x9, whole 4-column groups, 32-bit byte offsets
inline bool blur_slide_shape(int kh, int kw, bool separable, int nx, int ny) {
  return separable && kh == kw && (kh & 1) && kh >= 3 && kh <= 9 && (ny & 3) == 0 && ny >= 8 &&
         (int64_t)nx * ny < ((int64_t)1 << 29);
}
inline bool blur_strip_shape(int kh, int kw) { return kh == kw && (kh & 1) && kh >= 3 && kh <= 15; }

// The kernel a contiguous, 16-byte-aligned one-vector apply of such a blur runs on (TRK_BLUR_PATH_*; trk_blur2d_plan):
// slide and strip where they apply, otherwise the tile kernel up to 64x64, otherwise the generic kernel.
inline int blur_plan(int kh, int kw, bool separable, int nx, int ny) {
  if (blur_slide_shape(kh, kw, separable, nx, ny)) return TRK_BLUR_PATH_SLIDE;
  if (blur_strip_shape(kh, kw)) return TRK_BLUR_PATH_STRIP;
  if (kh <= kBlurTileMaxSide && kw <= kBlurTileMaxSide) return TRK_BLUR_PATH_TILE;
  return TRK_BLUR_PATH_GENERIC;
}

// blur_tile.hip: y = Op(x) for `batch` vectors by k_blur_tile (either form, by im->separable), optional sum of squares
int blur_tile_apply(trk_op* op, const BlurImpl* im, int tr, const float* x, int64_t ldx, float* y, int64_t ldy, int batch,
                    double* sumsq, hipStream_t s);

}  // namespace trk
