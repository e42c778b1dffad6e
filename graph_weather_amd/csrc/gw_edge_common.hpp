// gw_edge_common.hpp - device helpers shared by the hand-scheduled fp32 edge-update kernels (gw_edge.hip: edge_kernel,
// gw_edge_stream.hip: its persistent decoder form): loads hipcc must not count and their counted waits, the LDS weight ring
// (asm-issued LDS-DMA pieces, the LDS-only barrier) and the chunk macro with the hand-over in front of a chunk's last MFMAs.
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

}  // namespace

#endif  // GW_EDGE_COMMON_HPP
