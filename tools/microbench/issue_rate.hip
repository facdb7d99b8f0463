// issue_rate.hip — what does a gfx950 SIMD sustain for the instruction streams the parallel-beam projector is made of?
//
// bench.py priced a wave64 vector instruction at 4 cycles; MI355X_MICROARCH.md gives 2 cycles of
// throughput at more than one wave per SIMD ("one wave alone: 4").  This program measures, on the chip, at the clock the
// chip holds, for 1 / 2 / 4 / 7 waves per SIMD:
//   * independent v_fma_f32, v_add_u32, v_and_b32, v_lshrrev_b32, v_cvt_f32_u32, v_pk_fma_f32 streams,
//   * the forward projector's 7-instruction march (k_radon_fwd_lds, radon_fwd.hip; what bounds it: docs/kernels/radon.md 4.4c) without its LDS read,
//   * the same march WITH its ds_read2_b32 tap, for ray spacings inv = 1.0 (conflict-free), 1.2, 1.414 columns per lane,
//   * the bare LDS taps: ds_read2_b32, ds_read_b64 (pair layout), and dword-aligned (i.e. MISALIGNED) ds_read_b64 /
//     ds_read_b128 — first checked for what they return, then timed.
// Output: one line per (stream, waves per SIMD): wave-instructions per cycle per SIMD (by s_memtime, the shader clock),
// the clock (s_memtime / s_memrealtime) and the wall time.  Build: hipcc --offload-arch=gfx950 -O3 issue_rate.hip -o issue_rate
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                      \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f3v __attribute__((ext_vector_type(3)));

enum Mode {
  M_FMA = 0, M_ADD, M_AND, M_SHR, M_CVT, M_PKFMA, M_MARCH_NOLDS,
  M_MARCH_10, M_MARCH_12, M_MARCH_14,
  M_READ2_10, M_READ2_14, M_READ64_PAIR_10, M_READ64_PAIR_14,
  M_READ64_MIS, M_READ128_MIS_10, M_READ128_MIS_14, M_READ128_AL,
  M_SUB_V, M_SUB_S, M_LSHLADD_V, M_LSHLADD_S, M_BFE, M_QUAD_10, M_QUAD_14, M_QUAD_14H,
  M_COUNT
};
static const char* mode_name[M_COUNT] = {
  "v_fma_f32 x32 independent", "v_add_u32 x32 independent (VGPR operands)", "v_and_b32 x32 independent (one SGPR operand)", "v_lshrrev_b32 x32 independent",
  "v_cvt_f32_u32 x32 independent", "v_pk_fma_f32 x32 independent", "march 7 VALU/step, no LDS",
  "march 7 VALU + ds_read2_b32, inv=1.0", "march 7 VALU + ds_read2_b32, inv=1.2", "march 7 VALU + ds_read2_b32, inv=1.414",
  "ds_read2_b32 only, inv=1.0", "ds_read2_b32 only, inv=1.414", "ds_read_b64 pair layout, inv=1.0", "ds_read_b64 pair layout, inv=1.414",
  "ds_read_b64 dword-aligned (misaligned), inv=1.414", "ds_read_b128 dword-aligned, 2 rays/lane, inv=1.0", "ds_read_b128 dword-aligned, 2 rays/lane, inv=1.414",
  "ds_read_b128 16-byte aligned, lane-linear",
  "v_sub_f32 x128 independent (VGPR operands)", "v_sub_f32 x128 independent (one SGPR operand)",
  "v_lshl_add_u32 x128 independent (VGPR operands)", "v_lshl_add_u32 x128 independent (one SGPR operand)", "v_bfe_u32 x128 independent (inline constants)",
  "quad march: 7 VALU + 4 ds_read2_b32 + 4 v_pk_fma, inv=1.0", "quad march, inv=1.414 (64 rays: 2-way conflicts)",
  "quad march, inv=1.414, half-waves of <=31 columns",
};
// vector instructions per loop trip (for the rate), LDS instructions per loop trip
static const int mode_valu[M_COUNT] = {128, 128, 128, 128, 128, 128, 112, 112, 112, 112, 0, 0, 0, 0, 0, 0, 0, 0, 128, 128, 128, 128, 128, 176, 176, 176};
static const int mode_lds[M_COUNT] = {0, 0, 0, 0, 0, 0, 0, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0, 64, 64, 64};

struct Stamp { unsigned long long c0, c1, r0, r1; };

#define REP8(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)

template <int MODE>
__global__ __launch_bounds__(1024) void k_issue(int trips, float inv, const unsigned* __restrict__ Btab, float* __restrict__ out,
                                               Stamp* __restrict__ stamps) {
  extern __shared__ __attribute__((aligned(16))) float T[];      // 16 rows x 256 floats (pair layout uses 2x) + padding for occupancy
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < 16 * 512; i += blockDim.x) T[i] = (float)(i & 1023) * 0.001f;
  __syncthreads();
  float a[8];
  unsigned ui[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { a[i] = 1.0f + lane * 0.01f + i; ui[i] = lane * 2654435761u + i; }
  float m1 = 0.999f, m2 = 0.001f;
  unsigned su = 0x00fff0f0u;
  asm volatile("" : "+v"(m1), "+v"(m2), "+s"(su));
  f2v p[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i] = (f2v){a[i], a[i] + 0.5f};
  f2v pm = {0.999f, 1.001f}, pa = {0.001f, -0.001f};
  asm volatile("" : "+v"(pm), "+v"(pa));

  // the march's state: Ac = the ray's column (24 fractional bits) inside the window, per lane
  const float colf = (float)lane * inv + 1.25f;
  unsigned Ac = (unsigned)(colf * 16777216.0f);
  float two32 = 4294967296.0f;
  asm volatile("" : "+s"(two32));
  const unsigned tbase = (unsigned)(size_t)(__attribute__((address_space(3))) void*)T;
  f2v acc2 = {0.f, 0.f}, accB = {0.f, 0.f}, accC = {0.f, 0.f}, accD = {0.f, 0.f};
  // half-wave windows: each 32-lane group spans at most 31 columns (unowned lanes repeat the group's first ray)
  const int li = lane & 31;
  const float colh = (float)(li < (int)(31.0f / inv) ? li : 0) * inv + 1.25f + (lane >= 32 ? 31.0f : 0.f);
  unsigned AcH = (unsigned)(colh * 16777216.0f);
  float two32v = 4294967296.0f;
  unsigned Cm = tbase + 4u * (7u * 256u + 126u + 256u * 8u);   // mirrored tile: rows descending behind the forward tile
  asm volatile("" : "+v"(two32v), "+v"(Cm), "+v"(AcH));
  f4v acc4 = {0.f, 0.f, 0.f, 0.f};
  // bare-read addresses
  const unsigned c_lane = (unsigned)floorf(colf);
  const unsigned c_lane2 = (unsigned)floorf((float)(2 * lane) * inv + 1.25f);   // two rays per lane: the first ray's column
  unsigned addr_r2 = tbase + 4u * c_lane;                         // ds_read2_b32 / misaligned ds_read_b64: dword aligned
  unsigned addr_p = tbase + 8u * c_lane;                          // pair layout: 8-byte slots
  unsigned addr_m4 = tbase + 4u * c_lane2;                        // dword-aligned ds_read_b128
  unsigned addr_al = tbase + 16u * lane;
  asm volatile("" : "+v"(addr_r2), "+v"(addr_p), "+v"(addr_m4), "+v"(addr_al));

  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
#pragma unroll 1
  for (int it = 0; it < trips; ++it) {
    if constexpr (MODE == M_FMA) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#define X(i) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(m1), "v"(m2));
        REP8(X)
#undef X
      }
    } else if constexpr (MODE == M_ADD) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#define X(i) asm volatile("v_add_u32 %0, %0, %1" : "+v"(ui[i]) : "v"(Ac));
        REP8(X)
#undef X
      }
    } else if constexpr (MODE == M_AND) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#define X(i) asm volatile("v_and_b32 %0, %1, %0" : "+v"(ui[i]) : "s"(su));
        REP8(X)
#undef X
      }
    } else if constexpr (MODE == M_SHR) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#define X(i) asm volatile("v_lshrrev_b32 %0, 1, %0" : "+v"(ui[i]));
        REP8(X)
#undef X
      }
    } else if constexpr (MODE == M_CVT) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#define X(i) asm volatile("v_cvt_f32_u32 %0, %1" : "=v"(a[i]) : "v"(ui[i]));
        REP8(X)
#undef X
      }
    } else if constexpr (MODE == M_PKFMA) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#define X(i) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(p[i]) : "v"(pm), "v"(pa));
        REP8(X)
#undef X
      }
    } else if constexpr (MODE == M_MARCH_NOLDS || MODE == M_MARCH_10 || MODE == M_MARCH_12 || MODE == M_MARCH_14) {
      // 16 steps, instruction kinds in the order the compiler schedules the real kernel: all Q, then fractions, columns, addresses,
      // (the taps), then the packed FMAs.  Btab through the scalar cache: one s_load_dwordx16 per 16 steps, as in the kernel.
      const unsigned* __restrict__ Brow = Btab + ((it & 7) << 4);
      unsigned Q[16], adr[16];
      f2v w[16], t2[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const unsigned b = Brow[u];
        asm volatile("v_add_u32 %0, %1, %2" : "=v"(Q[u]) : "v"(Ac), "s"(b));
      }
      unsigned t[16];
      float f1[16], f0[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) asm volatile("v_lshlrev_b32 %0, 8, %1" : "=v"(t[u]) : "v"(Q[u]));
#pragma unroll
      for (int u = 0; u < 16; ++u) asm volatile("v_cvt_f32_u32 %0, %1" : "=v"(f1[u]) : "v"(t[u]));
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        asm volatile("v_sub_f32 %0, %1, %2" : "=v"(f0[u]) : "s"(two32), "v"(f1[u]));
        w[u] = (f2v){f0[u], f1[u]};
      }
      unsigned c[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) asm volatile("v_lshrrev_b32 %0, 24, %1" : "=v"(c[u]) : "v"(Q[u]));
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        int rowoff = u * 1024 + (int)tbase;
        asm volatile("" : "+s"(rowoff));
        asm volatile("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(adr[u]) : "v"(c[u]), "s"(rowoff));
      }
      if constexpr (MODE == M_MARCH_NOLDS) {
#pragma unroll
        for (int u = 0; u < 16; ++u) t2[u] = (f2v){__builtin_bit_cast(float, adr[u]), 1.0f};
      } else {
#pragma unroll
        for (int u = 0; u < 16; ++u) asm volatile("ds_read2_b32 %0, %1 offset1:1" : "=v"(t2[u]) : "v"(adr[u]));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int u = 0; u < 16; ++u) asm volatile("" : "+v"(t2[u]));
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(acc2) : "v"(w[u]), "v"(t2[u]));
    } else if constexpr (MODE == M_READ2_10 || MODE == M_READ2_14) {
      f2v t2[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) asm volatile("ds_read2_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(t2[u]) : "v"(addr_r2), "n"(u * 8), "n"(u * 8 + 1));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int u = 0; u < 16; ++u) asm volatile("" : "+v"(t2[u]));
#pragma unroll
      for (int u = 0; u < 16; ++u) acc2 += t2[u];
    } else if constexpr (MODE == M_READ64_PAIR_10 || MODE == M_READ64_PAIR_14 || MODE == M_READ64_MIS) {
      f2v t2[16];
      const unsigned ad = (MODE == M_READ64_MIS) ? addr_r2 : addr_p;
#pragma unroll
      for (int u = 0; u < 16; ++u) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(t2[u]) : "v"(ad), "n"(u * 2048));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int u = 0; u < 16; ++u) asm volatile("" : "+v"(t2[u]));
#pragma unroll
      for (int u = 0; u < 16; ++u) acc2 += t2[u];
    } else if constexpr (MODE == M_READ128_MIS_10 || MODE == M_READ128_MIS_14 || MODE == M_READ128_AL) {
      f4v t4[16];
      const unsigned ad = (MODE == M_READ128_AL) ? addr_al : addr_m4;
#pragma unroll
      for (int u = 0; u < 16; ++u) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(t4[u]) : "v"(ad), "n"(u * 1024));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int u = 0; u < 16; ++u) asm volatile("" : "+v"(t4[u]));
#pragma unroll
      for (int u = 0; u < 16; ++u) acc4 += t4[u];
    } else if constexpr (MODE == M_SUB_V) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#define X(i) asm volatile("v_sub_f32 %0, %1, %0" : "+v"(a[i]) : "v"(m1));
        REP8(X)
#undef X
      }
    } else if constexpr (MODE == M_SUB_S) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#define X(i) asm volatile("v_sub_f32 %0, %1, %0" : "+v"(a[i]) : "s"(two32));
        REP8(X)
#undef X
      }
    } else if constexpr (MODE == M_LSHLADD_V) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#define X(i) asm volatile("v_lshl_add_u32 %0, %0, 2, %1" : "+v"(ui[i]) : "v"(Ac));
        REP8(X)
#undef X
      }
    } else if constexpr (MODE == M_LSHLADD_S) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#define X(i) asm volatile("v_lshl_add_u32 %0, %0, 2, %1" : "+v"(ui[i]) : "s"(su));
        REP8(X)
#undef X
      }
    } else if constexpr (MODE == M_BFE) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#define X(i) asm volatile("v_bfe_u32 %0, %0, 1, 23" : "+v"(ui[i]));
        REP8(X)
#undef X
      }
    } else if constexpr (MODE == M_QUAD_10 || MODE == M_QUAD_14 || MODE == M_QUAD_14H) {
      // the march of a wave that serves FOUR symmetric angles from one set of taps (k_radon_fwd_quad): per step one Q, one weight
      // pair, one address and its mirror; four ds_read2_b32 (two tiles per address through the offset fields), four packed FMAs.
      // 16 steps = two chunks of 8; every operand a VGPR except the table entry and the row offset
      const unsigned* __restrict__ Brow = Btab + ((it & 7) << 4);
      const unsigned AcQ = (MODE == M_QUAD_14H) ? AcH : Ac;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        unsigned Q[8], adr[8], adm[8], t[8], c[8];
        float f1[8], f0[8];
        f2v w[8], ta[8], tb2[8], tc[8], td[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const unsigned b = Brow[8 * h + u];
          asm volatile("v_add_u32 %0, %1, %2" : "=v"(Q[u]) : "v"(AcQ), "s"(b));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) asm volatile("v_lshlrev_b32 %0, 8, %1" : "=v"(t[u]) : "v"(Q[u]));
#pragma unroll
        for (int u = 0; u < 8; ++u) asm volatile("v_cvt_f32_u32 %0, %1" : "=v"(f1[u]) : "v"(t[u]));
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          asm volatile("v_sub_f32 %0, %1, %2" : "=v"(f0[u]) : "v"(two32v), "v"(f1[u]));
          w[u] = (f2v){f0[u], f1[u]};
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) asm volatile("v_lshrrev_b32 %0, 24, %1" : "=v"(c[u]) : "v"(Q[u]));
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          int rowoff = u * 1024 + (int)tbase;
          asm volatile("" : "+s"(rowoff));
          asm volatile("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(adr[u]) : "v"(c[u]), "s"(rowoff));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) asm volatile("v_sub_u32 %0, %1, %2" : "=v"(adm[u]) : "v"(Cm), "v"(adr[u]));
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          asm volatile("ds_read2_b32 %0, %1 offset1:1" : "=v"(ta[u]) : "v"(adr[u]));
          asm volatile("ds_read2_b32 %0, %1 offset0:128 offset1:129" : "=v"(tb2[u]) : "v"(adr[u]));
          if (u == 3 || u == 7) {
#pragma unroll
            for (int v = u - 3; v <= u; ++v) {
              asm volatile("ds_read2_b32 %0, %1 offset1:1" : "=v"(tc[v]) : "v"(adm[v]));
              asm volatile("ds_read2_b32 %0, %1 offset0:128 offset1:129" : "=v"(td[v]) : "v"(adm[v]));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int v = u - 3; v <= u; ++v) {
              asm volatile("" : "+v"(ta[v]), "+v"(tb2[v]), "+v"(tc[v]), "+v"(td[v]));
              asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(acc2) : "v"(w[v]), "v"(ta[v]));
              asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(accB) : "v"(w[v]), "v"(tb2[v]));
              asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[0,1,1]" : "+v"(accC) : "v"(w[v]), "v"(tc[v]));
              asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[0,1,1]" : "+v"(accD) : "v"(w[v]), "v"(td[v]));
            }
          }
        }
      }
    }
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  float s = accB[0] + accB[1] + accC[0] + accC[1] + accD[0] + accD[1] + acc2[0] + acc2[1] + acc4[0] + acc4[1] + acc4[2] + acc4[3];
#pragma unroll
  for (int i = 0; i < 8; ++i) s += a[i] + (float)ui[i] + p[i][0] + p[i][1];
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
  if (lane == 0) stamps[(size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)] = Stamp{c0, c1, r0, r1};
}

// what do dword-aligned wide LDS reads return on this chip?
__global__ void k_misaligned_check(int* __restrict__ res) {
  __shared__ __attribute__((aligned(16))) float T[1024];
  for (int i = threadIdx.x; i < 1024; i += 64) T[i] = (float)i;
  __syncthreads();
  const unsigned tbase = (unsigned)(size_t)(__attribute__((address_space(3))) void*)T;
  int bad64 = 0, bad128 = 0, bad96 = 0;
  for (int off = 0; off < 8; ++off) {
    const unsigned c = (unsigned)threadIdx.x * 3u + (unsigned)off;      // all residues mod 4 across lanes and offsets
    unsigned ad = tbase + 4u * c;
    f2v v2;
    f4v v4;
    asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v2) : "v"(ad) : "memory");
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v4) : "v"(ad) : "memory");
    if (v2[0] != (float)c || v2[1] != (float)(c + 1)) ++bad64;
    if (v4[0] != (float)c || v4[1] != (float)(c + 1) || v4[2] != (float)(c + 2) || v4[3] != (float)(c + 3)) ++bad128;
    f3v v3;
    asm volatile("ds_read_b96 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v3) : "v"(ad) : "memory");
    if (v3[0] != (float)c || v3[1] != (float)(c + 1) || v3[2] != (float)(c + 2)) ++bad96;
  }
  res[threadIdx.x * 3 + 0] = bad64;
  res[threadIdx.x * 3 + 1] = bad128;
  res[threadIdx.x * 3 + 2] = bad96;
}

typedef void (*kern_t)(int, float, const unsigned*, float*, Stamp*);
template <int M>
static kern_t pick() { return k_issue<M>; }

int main(int argc, char** argv) {
  const int trips = argc > 1 ? atoi(argv[1]) : 4000;
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int ncu = prop.multiProcessorCount;
  printf("# device %s, %d CUs, trips %d (x %s)\n", prop.gcnArchName, ncu, trips, "32 VALU / 16 steps per trip");

  {
    int* res;
    CK(hipMalloc(&res, 64 * 3 * sizeof(int)));
    hipLaunchKernelGGL(k_misaligned_check, dim3(1), dim3(64), 0, 0, res);
    CK(hipDeviceSynchronize());
    std::vector<int> h(64 * 3);
    CK(hipMemcpy(h.data(), res, h.size() * sizeof(int), hipMemcpyDeviceToHost));
    int b64 = 0, b128 = 0, b96 = 0;
    for (int i = 0; i < 64; ++i) { b64 += h[3 * i]; b128 += h[3 * i + 1]; b96 += h[3 * i + 2]; }
    printf("# dword-aligned wide LDS reads, wrong results out of 512: ds_read_b64 %d, ds_read_b128 %d, ds_read_b96 %d\n", b64, b128, b96);
    CK(hipFree(res));
  }

  kern_t kern[M_COUNT] = {pick<0>(), pick<1>(), pick<2>(), pick<3>(), pick<4>(), pick<5>(), pick<6>(), pick<7>(), pick<8>(),
                          pick<9>(), pick<10>(), pick<11>(), pick<12>(), pick<13>(), pick<14>(), pick<15>(), pick<16>(), pick<17>(), pick<18>(), pick<19>(), pick<20>(),
                          pick<21>(), pick<22>(), pick<23>(), pick<24>(), pick<25>()};
  const float mode_inv[M_COUNT] = {1, 1, 1, 1, 1, 1, 1.2f, 1.0f, 1.2f, 1.41421f, 1.0f, 1.41421f, 1.0f, 1.41421f, 1.41421f, 1.0f, 1.41421f, 1.0f, 1, 1, 1, 1, 1, 1.0f, 1.41421f, 1.41421f};
  unsigned hB[128];
  for (int i = 0; i < 128; ++i) hB[i] = (unsigned)((double)(i & 15) * 0.37 * 16777216.0);
  unsigned* Btab;
  CK(hipMalloc(&Btab, sizeof(hB)));
  CK(hipMemcpy(Btab, hB, sizeof(hB), hipMemcpyHostToDevice));
  // waves per SIMD made certain: B workgroups of 4 k waves per CU (a workgroup's waves go round the four SIMDs), LDS sized so
  // that exactly B fit; the co-residency actually reached is measured (waves alive at the middle of the run / SIMDs)
  const int wps_list[5] = {1, 2, 4, 6, 8};
  const int cfgB[5] = {1, 1, 1, 2, 2}, cfgK[5] = {1, 2, 4, 3, 4};
  float* out;
  Stamp* stamps;
  CK(hipMalloc(&out, (size_t)ncu * 2 * 1024 * sizeof(float)));
  CK(hipMalloc(&stamps, (size_t)ncu * 2 * 16 * sizeof(Stamp)));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  printf("%-56s %4s %6s %12s %12s %10s %10s %10s\n", "stream", "w/S", "alive", "VALU/cyc/SIMD", "LDSop/cyc/CU", "cyc/trip(wave)", "clock GHz", "wall ms");
  for (int m = 0; m < M_COUNT; ++m) {
    for (int wi = 0; wi < 5; ++wi) {
      const int wps = wps_list[wi], B = cfgB[wi], K = cfgK[wi];
      const size_t lds = (size_t)(B == 1 ? 100 * 1024 : 70 * 1024);
      CK(hipFuncSetAttribute((const void*)kern[m], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      const int grid = ncu * B, block = 256 * K;
      hipLaunchKernelGGL(kern[m], dim3(grid), dim3(block), lds, 0, trips / 10 + 1, mode_inv[m], Btab, out, stamps);   // warm-up
      CK(hipDeviceSynchronize());
      CK(hipEventRecord(e0, 0));
      hipLaunchKernelGGL(kern[m], dim3(grid), dim3(block), lds, 0, trips, mode_inv[m], Btab, out, stamps);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms = 0.f;
      CK(hipEventElapsedTime(&ms, e0, e1));
      std::vector<Stamp> h((size_t)grid * 4 * K);
      CK(hipMemcpy(h.data(), stamps, h.size() * sizeof(Stamp), hipMemcpyDeviceToHost));
      std::vector<double> cyc, clk;
      unsigned long long rmin = ~0ull, rmax = 0;
      for (auto& s : h) {
        cyc.push_back((double)(s.c1 - s.c0));
        clk.push_back((double)(s.c1 - s.c0) / ((double)(s.r1 - s.r0) * 10.0));   // s_memrealtime ticks at 100 MHz -> GHz
        rmin = std::min(rmin, s.r0);
        rmax = std::max(rmax, s.r1);
      }
      const unsigned long long rmid = rmin + (rmax - rmin) / 2;
      size_t alive = 0;
      for (auto& s : h) alive += (s.r0 <= rmid && rmid < s.r1) ? 1 : 0;
      std::sort(cyc.begin(), cyc.end());
      std::sort(clk.begin(), clk.end());
      const double cmed = cyc[cyc.size() / 2], ghz = clk[clk.size() / 2];
      // rates over the whole run (all waves' instructions / the cycles between the first wave's start and the last wave's end):
      // a SIMD serves its oldest waves first, so the per-wave cycle count alone says little at more than two waves per SIMD
      const double span_cyc = (double)(rmax - rmin) * 10.0 * ghz;
      const double valu = (double)wps * mode_valu[m] * trips / span_cyc;
      const double ldsr = (double)wps * 4 * mode_lds[m] * trips / span_cyc;
      printf("%-56s %4d %6.2f %12.3f %12.3f %10.1f %10.3f %10.3f   span %.3f ms\n", mode_name[m], wps, (double)alive / (4.0 * ncu), valu, ldsr,
             cmed / trips, ghz, ms, (double)(rmax - rmin) * 1e-5);
    }
  }
  return 0;
}
