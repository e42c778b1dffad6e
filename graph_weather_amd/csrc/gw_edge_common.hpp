// gw_edge_common.hpp - what the hand-scheduled fp32 edge-update kernels share (gw_edge.hip: edge_kernel, gw_edge_lds.hip: its
// inference form with the constants in LDS, gw_edge_stream.hip: the decoder form without residual, gw_encoder_fused.hip: node
// encoder + edge update in one launch; one workgroup per 64-column tile in all four).  Device side: loads hipcc must not count
// and their counted waits, the LDS weight ring (asm-issued LDS-DMA pieces, the LDS-only barrier), the chunk macro with the
// hand-over in front of a chunk's last MFMAs, and the tile code around the matrix passes - tile coordinates, constants in LDS,
// LayerNorm, staging, e' store, segment sum.  Host side: the launch and the tile schedule.  Whether a shared piece is a function
// or a macro was decided by the generated code: a function where the kernels compile to the same
// instructions as with the text in place, a macro where inlining changed the floating-point contraction.
#ifndef GW_EDGE_COMMON_HPP
#define GW_EDGE_COMMON_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gw_device.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

constexpr int kStageLd = 260;                                  // floats per staged row: 65 x 16 B -> conflict-free b128 writes
constexpr int kStageFloats = kColsPerWG * kStageLd;            // 64 rows
constexpr int kEdgeLdsBytes = (kStageFloats + kColsPerWG) * 4;  // staging (overlays the 64 KiB weight buffers) + 64 dst ids
static_assert(kStageFloats * 4 >= kLdsBytes, "staging area must cover the weight double buffer");
constexpr int kChunkFloats = kChunkSteps * 1024;               // one weight chunk: 8 K-steps x 256 rows x 4 k = 32 KiB
constexpr int kChunksPerLayer = 64 / kChunkSteps;              // K = 256

#ifdef GW_TUNING
#define GW_DMA6(a) ((a).dma6)
#else
#define GW_DMA6(a) 0
#endif

template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- loads hipcc must not count -------------------------------------------------------------------------------
// global_load_lds is a FLAT-class instruction: while one is pending in hipcc's model, every s_waitcnt it generates
// for a VMEM result is vmcnt(0) - which would drain the weight DMA of the NEXT chunk each time a gathered register is
// first used.  The loads whose results are consumed inside the chunk loops are therefore issued from asm statements
// (invisible to that bookkeeping) and completed by explicit counted waits that name their destination registers
// ("+v"), so no consumer can be scheduled above the wait (cdna_hip_programming.md 5.7, form ii).
template <int OFF>
__device__ __forceinline__ f32x4 hld4(const float* p) {
  f32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(v) : "v"(p), "i"(OFF) : "memory");
  return v;
}
__device__ __forceinline__ int hldi(const int* p) {
  int v;
  asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
template <int N>
__device__ __forceinline__ void wait_regs(int& a, int& b) {
  asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(a), "+v"(b) : [n] "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_regs(f32x4 (&r)[1][2]) {
  asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(r[0][0]), "+v"(r[0][1]) : [n] "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_regs(f32x4 (&r)[2][2]) {
  asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(r[0][0]), "+v"(r[0][1]), "+v"(r[1][0]), "+v"(r[1][1]) : [n] "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_regs(f32x4 (&r)[3][2]) {
  asm volatile("s_waitcnt vmcnt(%[n])"
               : "+v"(r[0][0]), "+v"(r[0][1]), "+v"(r[1][0]), "+v"(r[1][1]), "+v"(r[2][0]), "+v"(r[2][1])
               : [n] "n"(N)
               : "memory");
}
template <int N>
__device__ __forceinline__ void wait_regs(f32x4 (&r)[4][2]) {
  asm volatile("s_waitcnt vmcnt(%[n])"
               : "+v"(r[0][0]), "+v"(r[0][1]), "+v"(r[1][0]), "+v"(r[1][1]), "+v"(r[2][0]), "+v"(r[2][1]), "+v"(r[3][0]),
                 "+v"(r[3][1])
               : [n] "n"(N)
               : "memory");
}
template <int N>
__device__ __forceinline__ void wait_regs(f32x4 (&r)[16]) {
  asm volatile("s_waitcnt vmcnt(%[n])"
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]), "+v"(r[8]),
                 "+v"(r[9]), "+v"(r[10]), "+v"(r[11]), "+v"(r[12]), "+v"(r[13]), "+v"(r[14]), "+v"(r[15])
               : [n] "n"(N)
               : "memory");
}
// 16 x 16 B of one 256-float row (accumulator layout: tile t at +16t floats; p already includes the 4q lane offset)
__device__ __forceinline__ void hld_row(f32x4 (&r)[16], const float* p) {
  r[0] = hld4<0>(p);     r[1] = hld4<64>(p);    r[2] = hld4<128>(p);   r[3] = hld4<192>(p);
  r[4] = hld4<256>(p);   r[5] = hld4<320>(p);   r[6] = hld4<384>(p);   r[7] = hld4<448>(p);
  r[8] = hld4<512>(p);   r[9] = hld4<576>(p);   r[10] = hld4<640>(p);  r[11] = hld4<704>(p);
  r[12] = hld4<768>(p);  r[13] = hld4<832>(p);  r[14] = hld4<896>(p);  r[15] = hld4<960>(p);
}

// one half (tiles 8h .. 8h+7) of such a row
template <int H>
__device__ __forceinline__ void hld_half_row(f32x4 (&r)[16], const float* p) {
  r[8 * H + 0] = hld4<512 * H + 0>(p);    r[8 * H + 1] = hld4<512 * H + 64>(p);
  r[8 * H + 2] = hld4<512 * H + 128>(p);  r[8 * H + 3] = hld4<512 * H + 192>(p);
  r[8 * H + 4] = hld4<512 * H + 256>(p);  r[8 * H + 5] = hld4<512 * H + 320>(p);
  r[8 * H + 6] = hld4<512 * H + 384>(p);  r[8 * H + 7] = hld4<512 * H + 448>(p);
}

// Workgroup barrier for the LDS weight ring.  __syncthreads() carries a workgroup-scope release fence, which hipcc
// lowers to s_waitcnt vmcnt(0): that would drain the gathers this kernel deliberately keeps in flight.  Here only
// LDS traffic has to be ordered: this wave's LDS reads are complete (lgkmcnt(0)) and its share of the weight DMA
// has landed (the caller's counted wait) before it arrives.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

extern __shared__ __attribute__((aligned(16))) float gw_edge_lds[];
__device__ __forceinline__ float* lds_base() { return gw_edge_lds; }
// LDS byte address of the dynamic segment (0 unless the kernel also had static LDS; taken from the pointer, not assumed)
__device__ __forceinline__ unsigned lds_base_bytes() {
  return (unsigned)(size_t)(__attribute__((address_space(3))) float*)gw_edge_lds;
}

// Each wave DMAs its 8 KiB share of one 32 KiB weight chunk into an LDS buffer: exactly 8 x global_load_lds (1 KiB
// each), no branches - the vmcnt(N) bookkeeping of the kernel counts on that.
__device__ __forceinline__ void issue_chunk32k(const float* __restrict__ g, float* ldsbuf, int lane, int wave) {
  const unsigned base = __builtin_amdgcn_readfirstlane(lds_base_bytes() + (unsigned)(ldsbuf - lds_base()) * 4u + (unsigned)wave * 1024u);
#pragma unroll
  for (int i = 0; i < 8; ++i) glds16_asm_s(g + (size_t)(wave + 4 * i) * 256, (unsigned)lane * 16u, base + (unsigned)i * 4096u);
}

// N of this wave's 8 pieces (first..first+N-1) of a chunk; buf_floats = float offset of the destination LDS buffer.
constexpr int kDmaSteps = 4;  // the 8 pieces of the next chunk are issued 2 per K-step during the first 4 steps of a chunk
template <int N>
__device__ __forceinline__ void issue_pieces(const float* __restrict__ g, int buf_floats, int first, int lane, int wave) {
  const unsigned base = __builtin_amdgcn_readfirstlane(lds_base_bytes() + (unsigned)buf_floats * 4u + (unsigned)wave * 1024u);
#pragma unroll
  for (int i = 0; i < N; ++i)
    glds16_asm_s(g + (size_t)(wave + 4 * (first + i)) * 256, (unsigned)lane * 16u, base + (unsigned)(first + i) * 4096u);
}

// GW_CHUNK(ACC, IN8, NEXT_EXISTS, WAIT_STMT, NEXT_SRC): NEXT_SRC = source of the weight chunk after this one.  Expected in scope:
// the launch arguments `a` (tuning builds read a.skip / a.dma6), lds, lane, wave, the chunk counter ci (chunk i lives in LDS
// buffer i & 1) and the A fragments a_cur[4] of the next K-step to run.
// One weight chunk (8 K-steps x 16 row tiles): ACC[t] += W[16t.., k(s)] * IN8[s].
// The A fragments of a step are read from LDS one step ahead (a_cur / a_nxt), ACROSS chunk boundaries: during the
// last step of chunk ci the boundary work for chunk ci+1 is done - counted wait WAIT_STMT (this wave's share of chunk
// ci+1 has landed), workgroup barrier (everybody's share has, and everybody is done reading chunk ci), DMA of chunk
// ci+2 into the buffer chunk ci vacates, first fragments of chunk ci+1 - and only then the step's 16 MFMAs are
// issued, so barrier skew and LDS latency sit underneath 16 MFMAs instead of draining the matrix pipe.
#define GW_CHUNK(ACC, IN8, NEXT_EXISTS, WAIT_STMT, NEXT_SRC)                                                            \
  {                                                                                                            \
    const float* bl_ = lds + (ci & 1) * kLdsBufFloats + lane * 4;                                              \
    const float* nsrc_ = (NEXT_SRC);                                                                            \
    _Pragma("unroll") for (int s_ = 0; s_ < kChunkSteps; ++s_) {                                               \
      f32x4 a_nxt_[4];                                                                                         \
      if ((NEXT_EXISTS) && GW_DMA6(a)) { /* tuning: the 8 pieces over SIX K-steps (2, 1, 1, 2, 1, 1) */                    \
        if (s_ == 0) issue_pieces<2>(nsrc_, ((ci + 1) & 1) * kLdsBufFloats, 0, lane, wave);                    \
        if (s_ == 1) issue_pieces<1>(nsrc_, ((ci + 1) & 1) * kLdsBufFloats, 2, lane, wave);                    \
        if (s_ == 2) issue_pieces<1>(nsrc_, ((ci + 1) & 1) * kLdsBufFloats, 3, lane, wave);                    \
        if (s_ == 3) issue_pieces<2>(nsrc_, ((ci + 1) & 1) * kLdsBufFloats, 4, lane, wave);                    \
        if (s_ == 4) issue_pieces<1>(nsrc_, ((ci + 1) & 1) * kLdsBufFloats, 6, lane, wave);                    \
        if (s_ == 5) issue_pieces<1>(nsrc_, ((ci + 1) & 1) * kLdsBufFloats, 7, lane, wave);                    \
      } else if ((NEXT_EXISTS) && s_ < kDmaSteps && GW_SKIP(a) != 4) {                                              \
        issue_pieces<8 / kDmaSteps>(nsrc_, ((ci + 1) & 1) * kLdsBufFloats, s_ * (8 / kDmaSteps), lane, wave);  \
      }                                                                                                        \
      if (s_ + 1 < kChunkSteps) {                                                                              \
        _Pragma("unroll") for (int b4 = 0; b4 < 4; ++b4) a_nxt_[b4] = *(const f32x4*)(bl_ + (s_ + 1) * 1024 + b4 * 256); \
      } else if (NEXT_EXISTS) {                                                                                \
        WAIT_STMT;                                                                                             \
        if (GW_SKIP(a) != 5) lds_barrier();                                                                        \
        const float* bn_ = lds + ((ci + 1) & 1) * kLdsBufFloats + lane * 4;                                    \
        _Pragma("unroll") for (int b4 = 0; b4 < 4; ++b4) a_nxt_[b4] = *(const f32x4*)(bn_ + b4 * 256);          \
      }                                                                                                        \
      const float b_ = IN8[s_];                                                                                \
      __builtin_amdgcn_sched_barrier(0);                                                                       \
      _Pragma("unroll") for (int t = 0; t < 16; ++t)                                                           \
          ACC[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[t >> 2][t & 3], b_, ACC[t], 0, 0, 0);             \
      __builtin_amdgcn_sched_barrier(0);                                                                       \
      if (s_ + 1 < kChunkSteps || (NEXT_EXISTS)) {                                                             \
        _Pragma("unroll") for (int b4 = 0; b4 < 4; ++b4) a_cur[b4] = a_nxt_[b4];                                \
      }                                                                                                        \
    }                                                                                                          \
    ++ci;                                                                                                      \
  }

// GW_REQUEST_SLICE(slot, slice): request slice `slice` (features 32 slice + 16 h + 4q .. +3, h = 0, 1) of the NPROJ projected
// operands' rows prow[p] into ring[slot][p][h].  Expected in scope: NPROJ, prow, ring.
#define GW_REQUEST_SLICE(slot, slice)                                          \
  {                                                                            \
    _Pragma("unroll") for (int p = 0; p < NPROJ; ++p) {                        \
      ring[slot][p][0] = hld4<128 * (slice)>(prow[p]);                         \
      ring[slot][p][1] = hld4<128 * (slice) + 64>(prow[p]);                    \
    }                                                                          \
  }

// ---- the tile around the matrix passes --------------------------------------------------------------------------
// Where a thread works: workgroup -> tile (XCD-aware order, see EdgeArgs), lane (j, q) of wave `wave` -> column c = edge k of
// sample b; columns past the end (valid == false) compute on the last column and store nothing.
// GW_TILE_COORDS declares lane, wave, j, q, tile, tile_c0, valid, c, b, k in the kernel's scope.  A macro: returned from a
// function (a struct of the ten values) the same text compiled to other code in the kernels' epilogues.
#define GW_TILE_COORDS(N_COLS, N_EDGES, XCD_BASE, XCD_REM)                                \
  const int lane = threadIdx.x & 63;                                                      \
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                      \
  const int j = lane & 15;                                                                \
  const int q = lane >> 4;                                                                \
  int tile = blockIdx.x;                                                                  \
  if ((XCD_BASE) > 0) {                                                                   \
    const int xcd = tile & 7, idx = tile >> 3;                                            \
    tile = xcd * (XCD_BASE) + (xcd < (XCD_REM) ? xcd : (XCD_REM)) + idx;                  \
  }                                                                                       \
  const int tile_c0 = tile * kColsPerWG;                                                  \
  const int c_raw = tile_c0 + wave * kColsPerWave + j;                                    \
  const bool valid = c_raw < (N_COLS);                                                    \
  const int c = valid ? c_raw : (N_COLS) - 1;                                             \
  const int b = c / (N_EDGES);                                                            \
  const int k = c - b * (N_EDGES);

// anti-phase start of the second batch of workgroups (see chain_kernel)
__device__ __forceinline__ void stagger_start(int stagger) {
  if (stagger > 0 && (blockIdx.x >> 8) == 1) {
    for (int i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(127);
  }
}

// ---- constants in LDS: an MLP's b1 | b_mid | b_out | gamma | beta as one set of 5 x 256 floats behind the staging area and
// the destination ids.  Thread f carries feature f of each vector there; the kernels' prologues differ in how the five values
// are requested and waited for, so that part stays with them.
constexpr int kConstSetFloats = 5 * 256;
constexpr int kConstOff = kStageFloats + kColsPerWG;
static_assert((kConstOff * 4) % 16 == 0, "constants are read as 16-byte vectors");
constexpr int kB1 = 0, kBMid = 256, kBOut = 512, kGamma = 768, kBeta = 1024;  // float offsets inside a set
// one float per thread of a constant vector, requested like the indices (a load hipcc does not count)
__device__ __forceinline__ float hld1(const float* p) {
  float v;
  asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
// cv[0..4] -> set `set` (float offset behind kConstOff); visible to the workgroup after the next lds_barrier()
__device__ __forceinline__ void consts_to_lds(float* lds, int set, const float* cv) {
  float* cw = lds + kConstOff + threadIdx.x;
  cw[set + kB1] = cv[0];
  cw[set + kBMid] = cv[1];
  cw[set + kBOut] = cv[2];
  cw[set + kGamma] = cv[3];
  cw[set + kBeta] = cv[4];
}

// GW_LAYERNORM256(O, LD4, GAMMA, BETA, RES): LayerNorm over the 256 features of each column (eps 1e-5, biased variance) of the
// accumulator tiles O[16] (the caller has added the bias).  gamma / beta vectors of tile t are LD4(GAMMA + 16 * t + 4 * q) with
// LD4 = GW_LDS4 (constants in LDS) or ldg4 (global memory); RES is empty or a residual addend in the macro's indices t, r
// (`+ rres[t][r]`).  Expected in scope: q.  A macro, not a function: as an inlined function hipcc no longer contracts
// v += d * d (and others) into fused multiply-adds, which changes the rounding.
#define GW_LDS4(p) (*(const f32x4*)(p))
#define GW_LAYERNORM256(O, LD4, GAMMA, BETA, RES)                                                              \
  {                                                                                                            \
    constexpr float inv_n = 1.0f / 256.0f;                                                                     \
    float s = 0.f;                                                                                             \
    _Pragma("unroll") for (int t = 0; t < 16; ++t) s += (O[t].x + O[t].y) + (O[t].z + O[t].w);                 \
    s += __shfl_xor(s, 16);                                                                                    \
    s += __shfl_xor(s, 32);                                                                                    \
    const float mean = s * inv_n;                                                                              \
    float v = 0.f;                                                                                             \
    _Pragma("unroll") for (int t = 0; t < 16; ++t) _Pragma("unroll") for (int r = 0; r < 4; ++r) {             \
      const float d = O[t][r] - mean;                                                                          \
      v += d * d;                                                                                              \
    }                                                                                                          \
    v += __shfl_xor(v, 16);                                                                                    \
    v += __shfl_xor(v, 32);                                                                                    \
    const float rstd = 1.0f / sqrtf(v * inv_n + 1e-5f);                                                        \
    _Pragma("unroll") for (int t = 0; t < 16; ++t) {                                                           \
      const f32x4 gm = LD4(GAMMA + 16 * t + 4 * q);                                                            \
      const f32x4 bt = LD4(BETA + 16 * t + 4 * q);                                                             \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) O[t][r] = (O[t][r] - mean) * rstd * gm[r] + bt[r] RES;     \
    }                                                                                                          \
  }

// GW_STAGE_ROWS(O, GD_ID): stage the rows O[16] through LDS: [64 columns][kStageLd] floats over the weight buffers + the 64 global
// destination ids behind them (GD_ID: -1 for a column past the end); declares gdl, the ids.  Expected in scope: lds, wave, j, q.
// A macro: as a function edge_kernel recomputed 4 * q for the row address instead of reusing the prologue's register.
#define GW_STAGE_ROWS(O, GD_ID)                                                                                \
  __syncthreads(); /* every wave is done reading the weight buffers */                                         \
  {                                                                                                            \
    float* srow = lds + (wave * kColsPerWave + j) * kStageLd + 4 * q;                                          \
    _Pragma("unroll") for (int t = 0; t < 16; ++t) *(f32x4*)(srow + 16 * t) = O[t];                            \
    if (q == 0) ((int*)(lds + kStageFloats))[wave * kColsPerWave + j] = (GD_ID);                               \
  }                                                                                                            \
  __syncthreads();                                                                                             \
  const int* gdl = (const int*)(lds + kStageFloats);

// e_out rows from the staged tile: one 1 KiB coalesced store per row (wave w writes the rows of its own 16 columns)
__device__ __forceinline__ void store_e_rows(const float* lds, float* e_out, int tile_c0, int n_cols, int wave, int lane) {
#pragma unroll 4
  for (int i = 0; i < kColsPerWave; ++i) {
    const int col = wave * kColsPerWave + i;
    if (tile_c0 + col < n_cols) {
      const f32x4 vv = *(const f32x4*)(lds + col * kStageLd + 4 * lane);
      stg4(e_out + (size_t)(tile_c0 + col) * 256 + 4 * lane, vv);
    }
  }
}

// GW_SEGMENT_SUM_ATOMICS(AGG): segment sum of the staged tile in atomics mode.  Thread f owns feature f; columns are sorted by
// global destination id (gdl, from GW_STAGE_ROWS), so equal ids form runs.  Interior runs belong to this tile alone -> plain
// stores; the first and the last run may continue in the neighbouring tiles -> atomics (AGG is zero-filled by the caller).  See
// edge_kernel for the ballot walk; its own copy also has the deterministic mode.  Expected in scope: lds, gdl, lane.  A macro:
// as a function the walk compiled to other code (more s_waitcnt in estream_kernel<2>, another instruction order in <1>).
#define GW_SEGMENT_SUM_ATOMICS(AGG)                                                                            \
  {                                                                                                            \
    const int f = threadIdx.x;                                                                                 \
    float vv[kColsPerWG];                                                                                      \
    _Pragma("unroll") for (int i = 0; i < kColsPerWG; ++i) vv[i] = lds[i * kStageLd + f];                      \
    const int gdv = gdl[lane];                                                                                 \
    const int gdn = gdl[lane < kColsPerWG - 1 ? lane + 1 : lane];                                              \
    const unsigned long long ends = __ballot(lane == kColsPerWG - 1 || gdn != gdv); /* bit i: a run ends with column i */ \
    float run = 0.f;                                                                                           \
    bool first = true;                                                                                         \
    _Pragma("unroll") for (int i = 0; i < kColsPerWG; ++i) {                                                   \
      run += vv[i];                                                                                            \
      if (__builtin_expect((ends >> i) & 1ull, 0)) {                                                           \
        const int cur = __builtin_amdgcn_readlane(gdv, i);                                                     \
        if (cur >= 0) {                                                                                        \
          float* dstp = (AGG) + (size_t)cur * 256 + f;                                                         \
          if (first || i == kColsPerWG - 1) {                                                                  \
            __hip_atomic_fetch_add((GW_AS1 float*)dstp, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      \
          } else {                                                                                             \
            stg1(dstp, run);                                                                                   \
          }                                                                                                    \
        }                                                                                                      \
        first = false;                                                                                         \
        run = 0.f;                                                                                             \
      }                                                                                                        \
    }                                                                                                          \
  }

// ---- host side -----------------------------------------------------------------------------------------------
// One workgroup per 64-column tile.  (K is the same type for every instantiation of a kernel template, so the dynamic-LDS
// limit is raised once per args struct and device, for the instantiation launched first.)
template <typename K, typename A>
int launch_tile_kernel(K kernel, const A& a, int lds_bytes, const char* name, void* stream) {
  static DeviceOnce once;
  if (once.first()) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  const int grid = (a.n_cols + kColsPerWG - 1) / kColsPerWG;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), lds_bytes, (hipStream_t)stream, a);
  return check_launch(name);
}

// the tuning switches GW_CHUNK reads; args without them (EncfArgs: GW_FCHUNK has no switches) take the second overload
template <typename A>
auto fill_chunk_switches(A& a, int) -> decltype((void)a.skip) {
  static const int skip = GW_TUNE("GW_EDGE_SKIP", 0);
  static const int dma6 = GW_TUNE("GW_EDGE_DMA6", 0);
  a.skip = skip;
  a.dma6 = dma6;
}
template <typename A>
void fill_chunk_switches(A&, long) {}

// Start-up stagger, XCD-aware tile order (see EdgeArgs) and the chunk switches of a launch of `tiles` tiles whose kernel makes
// `passes` passes over 256 x 256 weights per tile.
template <typename A>
void fill_tile_schedule(A& a, int tiles, int passes) {
  fill_chunk_switches(a, 0);
  static const int stagger_override = GW_TUNE("GW_STAGGER", -1);
  static const int stagger_max_tiles = GW_TUNE("GW_STAGGER_MAX_TILES", 0);  // > 0: GW_STAGGER applies to launches of at most that many tiles
  const bool overridden = stagger_override >= 0 && (stagger_max_tiles <= 0 || tiles <= stagger_max_tiles);
  // No start-up delay at any launch size ("fp32 forward: no start-up stagger"): on today's kernels, with
  // two chains sharing the chip, workgroups 256..511 sleeping for 2 passes + 2 units of 8 k cycles cost the 1 degree batch-2
  // step 0.14 ms and the batch-8 shard 0.14 ms.  The mechanism stays for tuning builds (GW_STAGGER units per pass).
  a.stagger = overridden ? stagger_override * passes : 0;
  if (tiles <= 256) a.stagger = 0;
  static const int xcd_map = GW_TUNE("GW_XCD_MAP", 1);  // 0: workgroup i takes tile i (A/B measurements)
  a.xcd_base = (xcd_map != 0 && tiles >= 64) ? tiles / 8 : 0;
  a.xcd_rem = tiles % 8;
}

}  // namespace

#endif  // GW_EDGE_COMMON_HPP
