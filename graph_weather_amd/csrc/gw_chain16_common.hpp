// gw_chain16_common.hpp - what the 16-bit chain kernels share: chain16_kernel (gw_bf16.hip, GW_DTYPE_BF16), chainx3_kernel and
// bwd_chainx3_kernel (gw_split.hip, GW_DTYPE_BF16X3), and the split helpers of the row-split node update (gw_noders.hip).  The
// two chain kernels are one skeleton - column coordinates, operand schedule, raw-row loader, bias, LayerNorm, residual, row
// store, HEAD tail, POST stores, segment sum - around a pass function each (pass16 / pass_x3), which stays in its file with the
// conversion of a B operand (pack8 / split-operand pairs).  Whether a shared piece is a function or a macro was decided by the
// generated code ("16-bit chain kernels"): a function where every kernel compiles to the same instructions
// as with the text in place, a token-identical macro otherwise.
#ifndef GW_CHAIN16_COMMON_HPP
#define GW_CHAIN16_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gw_device.hpp"
#include "gw_internal.hpp"

namespace gw {
namespace chain16 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// the segment-sum stage of the edge epilogue: 64 columns x 260 floats (65 x 16 B: conflict-free b128 writes) + 64 destination ids
constexpr int kStageLd = 260;
constexpr int kStageFloats = 64 * kStageLd;

template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// LDS-only workgroup barrier (gw_edge_common.hpp: __syncthreads() would drain the weight DMA in flight)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// DMA `bytes` (multiple of 1 KiB) of the packed weight stream into LDS at byte offset lds_off; pieces round-robin over the waves.
template <int NW>
__device__ __forceinline__ void issue_bytes(const char* __restrict__ g, int bytes, unsigned lds_off, int lane, int wave) {
  const int npieces = bytes >> 10;
  for (int p = wave; p < npieces; p += NW)
    glds16_asm_s((const float*)(g + (size_t)p * 1024), (unsigned)lane * 16u,
                 __builtin_amdgcn_readfirstlane(lds_off + (unsigned)p * 1024u));
}

// x -> (bf16(x), bf16(x - bf16(x))) for the 8 values of one B fragment
__device__ __forceinline__ void split8(f32x4 a, f32x4 b, bf16x8& h, bf16x8& l) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const __bf16 ha = (__bf16)a[r];
    h[r] = ha;
    l[r] = (__bf16)(a[r] - (float)ha);
    const __bf16 hb = (__bf16)b[r];
    h[4 + r] = hb;
    l[4 + r] = (__bf16)(b[r] - (float)hb);
  }
}
__device__ __forceinline__ f32x4 relu4(f32x4 v) {
  return f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
}

template <int NG, int NT>
__device__ __forceinline__ void init_bias(f32x4 (&acc)[NG][NT], const float* __restrict__ bias, int q) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const f32x4 bv = bias ? ldg4(bias + 16 * t + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g][t] = bv;
  }
}

__device__ __forceinline__ const float* operand_row(const float* ptr, const int* idx, int rows_pb, int ld, int b, int k) {
  const int r = idx ? ldgi(idx + k) : k;
  return ptr + ((size_t)b * (size_t)rows_pb + (size_t)r) * (size_t)ld;
}

// One raw operand row (valid features [0, kvalid)) in K order: put(s, lo, hi) receives row[k(s, q, 0..3)] and row[k(s, q, 4..7)]
// of K-step s and makes the lane's B fragment of them (pack8 / split8).
template <int KS, bool FULL, int DEPTH, typename Put>
__device__ __forceinline__ void load_raw_steps(const float* __restrict__ row, int kvalid, int q, Put put) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const bool pairs = !FULL && (kvalid & 1) == 0 && ((size_t)row & 7) == 0;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    f32x4 lo, hi;
    if (FULL) {
      lo = ldg4(row + 32 * s + 4 * q);
      hi = ldg4(row + 32 * s + 16 + 4 * q);
    } else if (pairs) {
      // rows of an even number of floats at an 8-byte aligned base (the 102 input features of the node encoder: 408-byte rows):
      // 8-byte loads - half the load instructions of the scalar form, which is what this launch's input phase is made of
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        const int k0 = 32 * s + 4 * q + r, k1 = k0 + 16;
        const f32x2 a = k0 < kvalid ? *(const GW_AS1 f32x2*)(row + k0) : f32x2{0.f, 0.f};
        const f32x2 b = k1 < kvalid ? *(const GW_AS1 f32x2*)(row + k1) : f32x2{0.f, 0.f};
        lo[r] = a.x;
        lo[r + 1] = a.y;
        hi[r] = b.x;
        hi[r + 1] = b.y;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k0 = 32 * s + 4 * q + r, k1 = k0 + 16;
        lo[r] = k0 < kvalid ? ldg1(row + k0) : 0.f;
        hi[r] = k1 < kvalid ? ldg1(row + k1) : 0.f;
      }
    }
    put(s, lo, hi);
    // at most 2 DEPTH row pieces in flight per group (DEPTH = 4 where registers are scarce: one wave per SIMD with two groups)
    if ((s & (DEPTH - 1)) == DEPTH - 1) __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- the skeleton around the passes --------------------------------------------------------------------------------
// the first chunk of the kernel's first pass into buffer 0
template <int NW>
__device__ __forceinline__ void issue_first_chunk(const bool (&on)[3], const char* const (&w1)[3], int k1_first, const char* after_l1,
                                                  int after_l1_bytes, int lane, int wave) {
  const char* first = on[0] ? w1[0] : (on[1] ? w1[1] : (on[2] ? w1[2] : after_l1));
  const int first_bytes = (on[0] || on[1] || on[2]) ? k1_first : after_l1_bytes;
  issue_bytes<NW>(first, first_bytes, 0u, lane, wave);
}

// features f0 .. f0 + 3 of an output row
template <int EPI>
__device__ __forceinline__ void store_tile(float* orow, int f0, f32x4 v, int out_cols) {
  if (EPI == EPI_DEC) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (f0 + r < out_cols) stg1(orow + f0 + r, v[r]);
  } else {
    stg4(orow + f0, v);
  }
}
// NT row tiles of a lane's share of a full row
template <int NT>
__device__ __forceinline__ void store_tiles(float* row, const f32x4 (&v)[NT], int q) {
#pragma unroll
  for (int t = 0; t < NT; ++t) stg4(row + 16 * t + 4 * q, v[t]);
}

// The pieces below are macros: as an inlined function each of them compiled to other instructions in some kernel (other
// registers and schedules; in the LayerNorm other contractions).  DESIGN.md section 4 has the counts.
//
// GW_CHAIN16_COLUMN_COORDS(NW, NG): where the lane's NG columns live - declares cc, bb, kk, valid: group g of wave `wave` holds
// column cc[g] = tile_c0 + g * (NW * 16) + wave * 16 + j = row kk[g] of sample bb[g]; columns past the end (valid[g] == false)
// compute on the last column and store nothing.  Expected in scope: a, tile_c0, wave, j.
#define GW_CHAIN16_COLUMN_COORDS(NW, NG)                                     \
  int cc[NG], bb[NG], kk[NG];                                                \
  bool valid[NG];                                                            \
  _Pragma("unroll") for (int g = 0; g < (NG); ++g) {                         \
    const int c_raw = tile_c0 + g * ((NW) * 16) + wave * 16 + j;             \
    valid[g] = c_raw < a.n_cols;                                             \
    cc[g] = valid[g] ? c_raw : a.n_cols - 1;                                 \
    bb[g] = cc[g] / a.cols_per_batch;                                        \
    kk[g] = cc[g] - bb[g] * a.cols_per_batch;                                \
  }

// GW_CHAIN16_OPERAND_SCHEDULE(NSEG, SINGLE): the layer-1 operands - declares on (raw: one matrix pass each), prj (projected:
// gather-adds), their packed slices w1, and w_mid, w_out.  Expected in scope: a.
#define GW_CHAIN16_OPERAND_SCHEDULE(NSEG, SINGLE)                                            \
  bool on[3], prj[3];                                                                        \
  _Pragma("unroll") for (int i = 0; i < 3; ++i) {                                            \
    on[i] = (i < (NSEG)) && (a.seg_k[i] > 0) && (a.seg_proj[i] == 0);                        \
    prj[i] = (i < (NSEG)) && (a.seg_k[i] > 0) && (a.seg_proj[i] != 0);                       \
  }                                                                                          \
  const char* w1[3] = {(const char*)a.w1[0], (const char*)a.w1[1], (const char*)a.w1[2]};    \
  if (SINGLE) w1[0] = (const char*)a.proj_w[blockIdx.y];                                     \
  const char* w_mid = (const char*)a.w_mid;                                                  \
  const char* w_out = (const char*)a.w_out;

// GW_CHAIN16_ADD_RESIDUAL(O, NG, OT, EPI): O += the residual rows (EPI_DEC: a.out_cols <= OT * 16 real features, rows of any
// alignment).  Expected in scope: a, bb, kk, q.
#define GW_CHAIN16_ADD_RESIDUAL(O, NG, OT, EPI)                                                                \
  _Pragma("unroll") for (int g = 0; g < (NG); ++g) {                                                           \
    const float* rrow = operand_row(a.res_ptr, a.res_idx, a.res_rows_pb, a.res_ld, bb[g], kk[g]);              \
    _Pragma("unroll") for (int t = 0; t < (OT); ++t) {                                                         \
      const int f0 = 16 * t + 4 * q;                                                                           \
      if ((EPI) == EPI_DEC) {                                                                                  \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) if (f0 + r < a.out_cols) O[g][t][r] += ldg1(rrow + f0 + r); \
      } else {                                                                                                 \
        O[g][t] += ldg4(rrow + f0);                                                                            \
        if ((t & 7) == 7) __builtin_amdgcn_sched_barrier(0);                                                   \
      }                                                                                                        \
    }                                                                                                          \
  }

// GW_CHAIN16_ZERO_FILL(NG): POST - zero-fill of the 256-wide rows of a.zero_rows.  Expected in scope: a, valid, cc, q.
#define GW_CHAIN16_ZERO_FILL(NG)                                                                               \
  _Pragma("unroll") for (int g = 0; g < (NG); ++g) if (valid[g]) {                                             \
    float* zrow = a.zero_rows + (size_t)cc[g] * 256;                                                           \
    _Pragma("unroll") for (int t = 0; t < 16; ++t) stg4(zrow + 16 * t + 4 * q, f32x4{0.f, 0.f, 0.f, 0.f});     \
  }

// GW_CHAIN16_STORE_HEAD_ROWS(Y, NG): HEAD tail - the head's a.out_cols <= 80 outputs Y[NG][5] (+ residual rows) of every
// column.  Rows of an even number of floats at 8-byte aligned bases (78 outputs, 102-float feature rows): 8-byte accesses.
// Expected in scope: a, valid, cc, bb, kk, q.
#define GW_CHAIN16_STORE_HEAD_ROWS(Y, NG)                                                                      \
  _Pragma("unroll") for (int g = 0; g < (NG); ++g) {                                                           \
    if (valid[g]) {                                                                                            \
      const float* rrow = a.res_ptr ? operand_row(a.res_ptr, a.res_idx, a.res_rows_pb, a.res_ld, bb[g], kk[g]) : nullptr; \
      float* orow = a.out + (size_t)cc[g] * (size_t)a.out_ld;                                                  \
      typedef float f32x2 __attribute__((ext_vector_type(2)));                                                 \
      const bool pairs = (a.out_cols & 1) == 0 && ((size_t)orow & 7) == 0 && ((size_t)rrow & 7) == 0;          \
      _Pragma("unroll") for (int t = 0; t < 5; ++t) {                                                          \
        const int f0 = 16 * t + 4 * q;                                                                         \
        if (pairs) {                                                                                           \
          _Pragma("unroll") for (int r = 0; r < 4; r += 2) if (f0 + r < a.out_cols) {                          \
            const f32x2 rv = rrow ? *(const GW_AS1 f32x2*)(rrow + f0 + r) : f32x2{0.f, 0.f};                   \
            *(GW_AS1 f32x2*)(orow + f0 + r) = f32x2{Y[g][t][r] + rv.x, Y[g][t][r + 1] + rv.y};                 \
          }                                                                                                    \
        } else {                                                                                               \
          _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                        \
              if (f0 + r < a.out_cols) stg1(orow + f0 + r, Y[g][t][r] + (rrow ? ldg1(rrow + f0 + r) : 0.f));   \
        }                                                                                                      \
      }                                                                                                        \
    }                                                                                                          \
  }

// GW_CHAIN16_LAYERNORM(O, NG, OT, MASKED): LayerNorm over the OT * 16 features of each column (eps 1e-5, biased variance), fp32,
// of the accumulator tiles O[NG][OT].  MASKED (compile time): heads and zero-padded narrow models normalise over their
// a.ln_width <= OT * 16 real features (gw_mlp_weights.ln_width): the padding rows of the last Linear are zero, so they drop out
// of the sum and are masked out of the variance; without it the width is OT * 16 (the host keeps such launches at ln_width ==
// OT * 16).  Expected in scope: a, q.
#define GW_CHAIN16_LAYERNORM(O, NG, OT, MASKED)                                                                 \
  {                                                                                                            \
    const int nfeat = (MASKED) ? a.ln_width : (OT) * 16;                                                       \
    const float inv_n = 1.0f / (float)nfeat;                                                                   \
    const bool full = nfeat == (OT) * 16;                                                                      \
    float mean[NG], rstd[NG];                                                                                  \
    _Pragma("unroll") for (int g = 0; g < (NG); ++g) {                                                         \
      float s = 0.f;                                                                                           \
      _Pragma("unroll") for (int t = 0; t < (OT); ++t) s += (O[g][t].x + O[g][t].y) + (O[g][t].z + O[g][t].w); \
      s += __shfl_xor(s, 16);                                                                                  \
      s += __shfl_xor(s, 32);                                                                                  \
      mean[g] = s * inv_n;                                                                                     \
      float v = 0.f;                                                                                           \
      _Pragma("unroll") for (int t = 0; t < (OT); ++t) _Pragma("unroll") for (int r = 0; r < 4; ++r) {         \
        const float d = O[g][t][r] - mean[g];                                                                  \
        v += (full || 16 * t + 4 * q + r < nfeat) ? d * d : 0.f;                                               \
      }                                                                                                        \
      v += __shfl_xor(v, 16);                                                                                  \
      v += __shfl_xor(v, 32);                                                                                  \
      rstd[g] = 1.0f / sqrtf(v * inv_n + 1e-5f);                                                               \
    }                                                                                                          \
    _Pragma("unroll") for (int t = 0; t < (OT); ++t) {                                                         \
      const f32x4 gm = ldg4(a.gamma + 16 * t + 4 * q);                                                         \
      const f32x4 bt = ldg4(a.beta + 16 * t + 4 * q);                                                          \
      _Pragma("unroll") for (int g = 0; g < (NG); ++g) _Pragma("unroll") for (int r = 0; r < 4; ++r)           \
          O[g][t][r] = (O[g][t][r] - mean[g]) * rstd[g] * gm[r] + bt[r];                                       \
    }                                                                                                          \
  }

// GW_CHAIN16_SEGMENT_SUM(O, LDS0, NW, NG, OT, HALF, WAVE4): segment sum of the rows O[NG][OT] over destination-sorted columns, 64
// columns at a time through LDS (see gw_edge.hip).  Every 4 waves (256 threads = 256 features) own one 64-column chunk of a
// round: stage + destination ids per chunk, from LDS0 (a float pointer; every pass of the workgroup is complete where the stage
// lies over the weight buffers).  HALF = chunk of this thread's wave within the round, WAVE4 = the wave's place in its chunk:
// (threadIdx.x >> 8, wave & 3), or (0, wave) where a workgroup is 4 waves by construction - hipcc does not derive the second
// form from the first.  Expected in scope: a, lane, wave, j, q, tile_c0, valid, bb, kk.
#define GW_CHAIN16_SEGMENT_SUM(O, LDS0, NW, NG, OT, HALF, WAVE4)                                               \
  {                                                                                                            \
    const int half = (HALF);                                                                                   \
    float* stage = (LDS0) + half * (kStageFloats + 64);                                                        \
    int* gdl = (int*)(stage + kStageFloats);                                                                   \
    _Pragma("unroll 1") for (int g = 0; g < (NG); ++g) {                                                       \
      __syncthreads(); /* the last pass's fragment reads / the previous round's readers are done */            \
      {                                                                                                        \
        float* srow = stage + ((WAVE4) * 16 + j) * kStageLd + 4 * q;                                        \
        /* (dynamic g: select the group's registers with a fully unrolled compare chain) */                    \
        _Pragma("unroll") for (int g2 = 0; g2 < (NG); ++g2) if (g2 == g) {                                     \
          _Pragma("unroll") for (int t = 0; t < (OT); ++t) *(f32x4*)(srow + 16 * t) = O[g2][t];                \
          if (q == 0) gdl[(WAVE4) * 16 + j] = valid[g2] ? bb[g2] * a.agg_rows_pb + ldgi(a.agg_idx + kk[g2]) : -1; \
        }                                                                                                      \
      }                                                                                                        \
      __syncthreads();                                                                                         \
      /* all 64 LDS reads first; run ends are a 64-bit scalar mask (lane i compares column i with column i + 1): the walk */ \
      /* is straight-line code testing one bit per column (see gw_edge.hip) */                                 \
      const int f = threadIdx.x & 255;                                                                         \
      float vv[64];                                                                                            \
      _Pragma("unroll") for (int i = 0; i < 64; ++i) vv[i] = stage[i * kStageLd + f];                          \
      const int gdv = gdl[lane];                                                                               \
      const int gdn = gdl[lane < 63 ? lane + 1 : lane];                                                        \
      const unsigned long long ends = __ballot(lane == 63 || gdn != gdv);                                      \
      /* deterministic mode: carry records instead of atomics (gw_internal.hpp; same scheme as gw_edge.hip) */ \
      bool open_lo = true, open_hi = true;                                                                     \
      float* rec = nullptr;                                                                                    \
      if (a.carry != nullptr) {                                                                                \
        const int chunk_c0 = tile_c0 + g * ((NW) * 16) + half * 64;                                            \
        rec = a.carry + (size_t)(chunk_c0 >> 6) * kCarryFloats;                                                \
        const int c_prev = chunk_c0 - 1, c_next = chunk_c0 + 64;                                               \
        int gd_prev = -2, gd_next = -2;                                                                        \
        if (c_prev >= 0 && c_prev < a.n_cols) {                                                                \
          const int bp = c_prev / a.cols_per_batch;                                                            \
          gd_prev = bp * a.agg_rows_pb + ldgi(a.agg_idx + (c_prev - bp * a.cols_per_batch));                   \
        }                                                                                                      \
        if (c_next < a.n_cols) {                                                                               \
          const int bn = c_next / a.cols_per_batch;                                                            \
          gd_next = bn * a.agg_rows_pb + ldgi(a.agg_idx + (c_next - bn * a.cols_per_batch));                   \
        }                                                                                                      \
        open_lo = gd_prev == __builtin_amdgcn_readlane(gdv, 0);                                                \
        open_hi = gd_next == __builtin_amdgcn_readlane(gdv, 63);                                               \
        if (f == 0 && chunk_c0 < a.n_cols) {                                                                   \
          rec[512] = __int_as_float(-1);                                                                       \
          rec[513] = __int_as_float(-1);                                                                       \
          rec[514] = __int_as_float(0);                                                                        \
        }                                                                                                      \
      }                                                                                                        \
      float run = 0.f;                                                                                         \
      bool first = true;                                                                                       \
      _Pragma("unroll") for (int i = 0; i < 64; ++i) {                                                         \
        run += vv[i];                                                                                          \
        if (__builtin_expect((ends >> i) & 1ull, 0)) {                                                         \
          const int cur = __builtin_amdgcn_readlane(gdv, i);                                                   \
          if (cur >= 0) {                                                                                      \
            float* dstp = a.agg + (size_t)cur * 256 + f;                                                       \
            if (rec != nullptr) {                                                                              \
              const bool lo = first && open_lo, hi = i == 63 && open_hi;                                       \
              if (lo) {                                                                                        \
                rec[f] = run;                                                                                  \
                if (f == 0) {                                                                                  \
                  rec[512] = __int_as_float(cur);                                                              \
                  if (hi) rec[514] = __int_as_float(1);                                                        \
                }                                                                                              \
              } else if (hi) {                                                                                 \
                rec[256 + f] = run;                                                                            \
                if (f == 0) rec[513] = __int_as_float(cur);                                                    \
              } else {                                                                                         \
                stg1(dstp, run);                                                                               \
              }                                                                                                \
            } else if (first || i == 63) {                                                                     \
              __hip_atomic_fetch_add((GW_AS1 float*)dstp, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    \
            } else {                                                                                           \
              stg1(dstp, run);                                                                                 \
            }                                                                                                  \
          }                                                                                                    \
          first = false;                                                                                       \
          run = 0.f;                                                                                           \
        }                                                                                                      \
      }                                                                                                        \
    }                                                                                                          \
  }

// ---- host side -----------------------------------------------------------------------------------------------
// K-steps (32 input features each) of a packed 16-bit slice: the layer-1 kernels exist for 1, 4 and 8 steps (k <= 32, k <= 128,
// 256) and stream exactly that many, so a narrower slice is zero-padded to its variant's step count (see gw_packed_floats).
inline int packed_steps16(int kseg) { return kseg <= 32 ? 1 : (kseg <= 128 ? 4 : (kseg + 31) / 32); }
// row tiles per K-step of a packed slice: the 16-row tiles of n_out rows, rounded up to 4
inline int padded_tiles(int n_out) { return (((n_out + 15) / 16) + 3) / 4 * 4; }

// One workgroup of `threads` threads per `cols` columns.  (K is the same type for every instantiation of a kernel template, so
// the dynamic-LDS limit is raised once per file and device, for the instantiation launched first; static: one DeviceOnce per
// file, as before.)
template <typename K>
static int launch_chain16(K kernel, ChainArgs& a, void* stream, int grid_y, int lds_bytes, int threads, int cols, int lds_cap, const char* what) {
  static DeviceOnce once;
  if (once.first()) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap);
  const int grid = (a.n_cols + cols - 1) / cols;
  hipLaunchKernelGGL(kernel, dim3(grid, grid_y), dim3(threads), lds_bytes, (hipStream_t)stream, a);
  return check_launch(what);
}

}  // namespace chain16
}  // namespace gw

#endif  // GW_CHAIN16_COMMON_HPP
