// gw_encoder_fused.hip - the fp32 encoder stage in one launch: node encoder and encoder edge update on the same 64-column tile.
//
//     xg  = LN_n(Wn_out . relu(Wn_mid . relu(Wn_1 . features[src] + bn_1) + bn_mid) + bn_out)          (node encoder, per edge)
//     e'  = LN(W_out . relu(W_mid . relu(b1 + W_s . xg + sum_p P_p[row_p]) + b_mid) + b_out) [+ e_res]   (edge MLP)
//     agg[dst] += e'
//
// The encoder's bipartite graph has one edge per grid node, so the grid row a column of the edge update reads as its raw
// operand is the row that column can produce itself: after the node encoder's LayerNorm the accumulator layout IS the B-operand
// layout of the W_s pass (gw_kernels.hip, header), the rows stay in registers and the [B.G, 256] table between the two launches
// is neither written nor read.  What else the result does not need is gone as in gw_edge_lds.hip / gw_edge_stream.hip:
//   * the ten constant vectors (b1, b_mid, b_out, gamma, beta of each MLP) are copied to LDS at kernel start and read from there,
//   * without RES the per-edge residual row is not streamed (the caller adds its segment sums as a cached table).
// Arithmetic: the node-encoder part keeps chain_kernel<28, ...>'s summation order and LayerNorm expressions, the edge part
// elds_kernel<true, NPROJ>'s - with RES the aggregate is bit for bit the one of the two launches.
// Weight stream of a tile, through the 2 x 32 KiB ring of gw_edge_common.hpp: Wn_1 (28 K-steps: three chunks of 8 and one of 4
// with 4 DMA pieces per wave), Wn_mid, Wn_out, W_s, W_mid, W_out (8 chunks each): 44 chunks, 348 pieces and 5568 MFMAs per wave.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "gw_device.hpp"
#include "gw_edge_common.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

constexpr int kNodeSteps = 28;                                 // K-steps of the node encoder's first layer (17 .. 112 features)
constexpr int kNodeSet = 0, kEdgeSet = kConstSetFloats;        // two sets of constants: the node encoder's, then the edge MLP's
constexpr int kEncfLdsBytes = (kConstOff + 2 * kConstSetFloats) * 4;
static_assert(kEncfLdsBytes == 77056, "staging (66 560) + destination ids (256) + constants (10 240)");
static_assert(2 * kEncfLdsBytes <= 160 * 1024, "two workgroups per CU must fit the 160 KiB of LDS");

struct EncfArgs {
  int n_cols;  // batch * n_edges
  int n_edges;
  int n_dst;
  int stagger;
  int xcd_base;  // XCD-aware tile order, as in edge_kernel (0: identity)
  int xcd_rem;
  const int* src;
  const int* dst;
  // grid features: fp32 rows of k_valid floats, row = b * rows_pb + src[k]
  const float* feat;
  int feat_rows_pb;
  int feat_ld;
  int k_valid;
  // node encoder (packed: first layer in 28 K-steps)
  const float* n_w1;
  const float* n_w_mid;
  const float* n_w_out;
  const float* n_const[5];  // b1, b_mid, b_out, gamma, beta
  // edge MLP
  const float* w_raw;  // W_s
  const float* w_mid;
  const float* w_out;
  const float* e_const[5];
  // projected operands: rows already hold X . W1_slice^T, gathered and added
  const float* p_ptr[2];
  int p_rows_pb[2];
  int p_ld[2];
  int p_kind[2];  // 1: row = dst[k], 2: k
  // residual e rows (indexed by edge; RES kernels)
  const float* res_ptr;
  int res_rows_pb;
  int res_ld;
  float* agg;
};

constexpr int kChunksPerTile = 4 + 5 * kChunksPerLayer;

// Source of weight chunk i of a tile (i is a constant after unrolling)
__device__ __forceinline__ const float* chunk_src(const EncfArgs& a, int i) {
  if (i < 4) return a.n_w1 + (size_t)i * kChunkFloats;
  i -= 4;
  const float* m = i < 8 ? a.n_w_mid : (i < 16 ? a.n_w_out : (i < 24 ? a.w_raw : (i < 32 ? a.w_mid : a.w_out)));
  return m + (size_t)(i & 7) * kChunkFloats;
}

// loads hipcc must not count (gw_edge_common.hpp): one 8-byte pair per thread
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 hld2(const float* p) {
  f32x2 v;
  asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ void wait_const(float (&c)[10]) {
  asm volatile("s_waitcnt vmcnt(0)"
               : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]), "+v"(c[8]), "+v"(c[9])
               :
               : "memory");
}
__device__ __forceinline__ void wait_pairs(f32x2 (&r)[14]) {
  asm volatile("s_waitcnt vmcnt(0)"
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]), "+v"(r[8]), "+v"(r[9]),
                 "+v"(r[10]), "+v"(r[11]), "+v"(r[12]), "+v"(r[13])
               :
               : "memory");
}
__device__ __forceinline__ void wait_singles(float (&r)[kNodeSteps]) {
  asm volatile("s_waitcnt vmcnt(0)"
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]), "+v"(r[8]), "+v"(r[9]),
                 "+v"(r[10]), "+v"(r[11]), "+v"(r[12]), "+v"(r[13])
               :
               : "memory");
  asm volatile("s_waitcnt vmcnt(0)"
               : "+v"(r[14]), "+v"(r[15]), "+v"(r[16]), "+v"(r[17]), "+v"(r[18]), "+v"(r[19]), "+v"(r[20]), "+v"(r[21]), "+v"(r[22]),
                 "+v"(r[23]), "+v"(r[24]), "+v"(r[25]), "+v"(r[26]), "+v"(r[27])
               :
               : "memory");
}

// GW_FCHUNK(ACC, IN, OFF, NS, NP, DS, WAIT_STMT): GW_CHUNK of gw_edge_common.hpp for a ring whose chunks differ in size.
// This chunk has NS K-steps (B operand IN[OFF + s]); the next one (chunk ci + 1, source chunk_src(a, ci + 1)) has NP DMA pieces
// per wave (0: there is none), issued NP / DS per K-step during the first DS steps of this chunk.  Hand-over as in GW_CHUNK: in
// front of the last step's MFMAs the counted wait WAIT_STMT, the workgroup barrier and the first fragments of chunk ci + 1.
#define GW_FCHUNK(ACC, IN, OFF, NS, NP, DS, WAIT_STMT)                                                          \
  {                                                                                                            \
    const float* bl_ = lds + (ci & 1) * kLdsBufFloats + lane * 4;                                              \
    const float* nsrc_ = chunk_src(a, (NP) > 0 ? ci + 1 : ci);                                                 \
    _Pragma("unroll") for (int s_ = 0; s_ < (NS); ++s_) {                                                      \
      f32x4 a_nxt_[4];                                                                                         \
      if ((NP) > 0 && s_ < (DS))                                                                               \
        issue_pieces<((NP) > 0 ? (NP) / (DS) : 1)>(nsrc_, ((ci + 1) & 1) * kLdsBufFloats, s_ * ((NP) / (DS)), lane, wave); \
      if (s_ + 1 < (NS)) {                                                                                     \
        _Pragma("unroll") for (int b4 = 0; b4 < 4; ++b4) a_nxt_[b4] = *(const f32x4*)(bl_ + (s_ + 1) * 1024 + b4 * 256); \
      } else if ((NP) > 0) {                                                                                   \
        WAIT_STMT;                                                                                             \
        lds_barrier();                                                                                         \
        const float* bn_ = lds + ((ci + 1) & 1) * kLdsBufFloats + lane * 4;                                    \
        _Pragma("unroll") for (int b4 = 0; b4 < 4; ++b4) a_nxt_[b4] = *(const f32x4*)(bn_ + b4 * 256);          \
      }                                                                                                        \
      const float b_ = IN[(OFF) + s_];                                                                         \
      __builtin_amdgcn_sched_barrier(0);                                                                       \
      _Pragma("unroll") for (int t = 0; t < 16; ++t)                                                           \
          ACC[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[t >> 2][t & 3], b_, ACC[t], 0, 0, 0);             \
      __builtin_amdgcn_sched_barrier(0);                                                                       \
      if (s_ + 1 < (NS) || (NP) > 0) {                                                                         \
        _Pragma("unroll") for (int b4 = 0; b4 < 4; ++b4) a_cur[b4] = a_nxt_[b4];                                \
      }                                                                                                        \
    }                                                                                                          \
    ++ci;                                                                                                      \
  }

template <bool RES, int NPROJ>
__global__ __launch_bounds__(kThreads, 2) void encfused_kernel(const EncfArgs a) {
  float* const lds = lds_base();
  const float* const cst = lds + kConstOff;
  GW_TILE_COORDS(a.n_cols, a.n_edges, a.xcd_base, a.xcd_rem)
  stagger_start(a.stagger);

  // ---- prologue.  Issue order matters for the counted waits (vmcnt retires in order) ----
  int s_idx = hldi(a.src + k);
  int d_idx = hldi(a.dst + k);
  float cv[10];  // thread f carries feature f of the ten constant vectors to LDS; they travel with the indices
  {
    const int f = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 5; ++i) cv[i] = hld1(a.n_const[i] + f);
#pragma unroll
    for (int i = 0; i < 5; ++i) cv[5 + i] = hld1(a.e_const[i] + f);
  }
  issue_chunk32k(chunk_src(a, 0), lds, lane, wave);
  int ci = 0;  // chunk counter of this tile (wave uniform); chunk i lives in LDS buffer i & 1
  wait_regs<18>(s_idx, d_idx);  // the indices have landed; the ten constants and the 8 DMA pieces stay in flight
  const float* prow[NPROJ];
#pragma unroll
  for (int p = 0; p < NPROJ; ++p) {
    const int r = a.p_kind[p] == 1 ? d_idx : k;
    prow[p] = a.p_ptr[p] + ((size_t)b * (size_t)a.p_rows_pb[p] + (size_t)r) * (size_t)a.p_ld[p] + 4 * q;
  }
  int gd_id = valid ? b * a.n_dst + d_idx : -1;  // global destination row of this column (segment-sum key)
  asm volatile("" : "+v"(gd_id));                // (made here, where registers are free, not in the LayerNorm epilogue)

  // the feature row of this column, in the K order of the matrix product: x[s] = row[16 (s >> 2) + 4 q + (s & 3)], zero beyond
  // k_valid (chain_kernel's load_operand<28, false>: 8-byte pairs where the rows allow them)
  float x[kNodeSteps];
  {
    const float* row = a.feat + ((size_t)b * (size_t)a.feat_rows_pb + (size_t)s_idx) * (size_t)a.feat_ld;
    const bool pairs = (a.k_valid & 1) == 0 && ((size_t)row & 7) == 0;
    if (pairs) {
      f32x2 pv[14];
#pragma unroll
      for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int kk = 16 * i + 4 * q + 2 * r;
          pv[2 * i + r] = hld2(row + (kk < a.k_valid ? kk : 0));
        }
      wait_pairs(pv);
#pragma unroll
      for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const bool in = 16 * i + 4 * q + 2 * r < a.k_valid;
          x[4 * i + 2 * r] = in ? pv[2 * i + r].x : 0.f;
          x[4 * i + 2 * r + 1] = in ? pv[2 * i + r].y : 0.f;
        }
    } else {
#pragma unroll
      for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kk = 16 * i + 4 * q + r;
          x[4 * i + r] = hld1(row + (kk < a.k_valid ? kk : 0));
        }
      wait_singles(x);
#pragma unroll
      for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (!(16 * i + 4 * q + r < a.k_valid)) x[4 * i + r] = 0.f;
    }
  }
  wait_const(cv);  // (everything has landed: chunk 0, the constants, the row)
  consts_to_lds(lds, kNodeSet, cv);
  consts_to_lds(lds, kEdgeSet, cv + 5);
  lds_barrier();  // everybody's share of chunk 0 and of the constants

  f32x4 a_cur[4];  // A fragments of the next K-step to run
#pragma unroll
  for (int b4 = 0; b4 < 4; ++b4) a_cur[b4] = *(const f32x4*)(lds + lane * 4 + b4 * 256);

  // ================= node encoder (chain_kernel<28, false, 1, 16, 16, EPI_ROWS>'s arithmetic) =================
  f32x4 o[16];
  {
    f32x4 acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = *(const f32x4*)(cst + kNodeSet + kB1 + 16 * t + 4 * q);
    GW_FCHUNK(acc, x, 0, 8, 8, 4, wait_vm<0>())
    GW_FCHUNK(acc, x, 8, 8, 8, 4, wait_vm<0>())
    GW_FCHUNK(acc, x, 16, 8, 4, 4, wait_vm<0>())  // the next chunk is the short one: K-steps 24 .. 27, 4 pieces per wave
    GW_FCHUNK(acc, x, 24, 4, 8, 2, wait_vm<0>())  // 4 K-steps; the 8 pieces of the middle layer's first chunk under the first two
    f32x4 acc2[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc2[t] = *(const f32x4*)(cst + kNodeSet + kBMid + 16 * t + 4 * q);
#pragma unroll
    for (int cc = 0; cc < kChunksPerLayer; ++cc) {
      float in8[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        in8[r] = fmaxf(acc[2 * cc][r], 0.f);
        in8[4 + r] = fmaxf(acc[2 * cc + 1][r], 0.f);
      }
      GW_FCHUNK(acc2, in8, 0, 8, 8, 4, wait_vm<0>())
    }
    float hin[64];
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) hin[4 * t + r] = fmaxf(acc2[t][r], 0.f);
#pragma unroll
    for (int t = 0; t < 16; ++t) o[t] = *(const f32x4*)(cst + kNodeSet + kBOut + 16 * t + 4 * q);
#pragma unroll
    for (int cc = 0; cc < kChunksPerLayer; ++cc) GW_FCHUNK(o, hin, 8 * cc, 8, 8, 4, wait_vm<0>())
    GW_LAYERNORM256(o, GW_LDS4, cst + kNodeSet + kGamma, cst + kNodeSet + kBeta, )
  }

  // ================= edge update (elds_kernel<true, NPROJ>'s arithmetic); o = the grid row = its raw operand =================
  // ring[s & 1][p][h]: features 32s + 16h + 4q .. +3 of projected operand p = its part of the B operand of produce
  // chunk s.  Slice s is requested when slice s-2 has been consumed (end of chunk s-3) and consumed at the end of chunk s-1.
  f32x4 ring[2][NPROJ][2];
  // B operand of produce chunk `slice` from ring slot `slot`: the layer-1 accumulator tiles (they started from b1) plus the
  // gathered rows
#define GW_CONSUME_SLICE(slot, slice)                                          \
  {                                                                            \
    f32x4 v0_ = acc[2 * (slice)] + ring[slot][0][0];                           \
    f32x4 v1_ = acc[2 * (slice) + 1] + ring[slot][0][1];                       \
    _Pragma("unroll") for (int p = 1; p < NPROJ; ++p) {                        \
      v0_ += ring[slot][p][0];                                                 \
      v1_ += ring[slot][p][1];                                                 \
    }                                                                          \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                            \
      in8[r] = fmaxf(v0_[r], 0.f);                                             \
      in8[4 + r] = fmaxf(v1_[r], 0.f);                                         \
    }                                                                          \
  }

  f32x4 acc[16];   // layer-1 accumulator
  f32x4 acc2[16];  // first hidden layer accumulator
  float in8[8];    // B operand values of the next chunk
  {
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = *(const f32x4*)(cst + kEdgeSet + kB1 + 16 * t + 4 * q);
    float xr[64];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      xr[4 * i + 0] = o[i].x;
      xr[4 * i + 1] = o[i].y;
      xr[4 * i + 2] = o[i].z;
      xr[4 * i + 3] = o[i].w;
    }
#pragma unroll
    for (int cc = 0; cc < kChunksPerLayer; ++cc) {
      if (cc == kChunksPerLayer - 3) {  // the first two ring slices, once most of the row is dead
        GW_REQUEST_SLICE(0, 0)
        GW_REQUEST_SLICE(1, 1)
      }
      if (cc == kChunksPerLayer - 1) {  // next layer's bias, under the last chunk (the row is dead)
#pragma unroll
        for (int t = 0; t < 16; ++t) acc2[t] = *(const f32x4*)(cst + kEdgeSet + kBMid + 16 * t + 4 * q);
      }
      GW_FCHUNK(acc, xr, 8 * cc, 8, 8, 4, wait_vm<0>())
    }
    wait_regs<0>(ring[0]);  // (landed long ago: everything was drained by the vmcnt(0) boundaries above)
    wait_regs<0>(ring[1]);
    GW_CONSUME_SLICE(0, 0)
    GW_REQUEST_SLICE(0, 2)
  }

  // ---- first hidden layer: B operand produced slice by slice = relu(layer-1 accumulator + gathered rows) ----
  // boundary into produce chunk cc+1: the pieces of chunk cc+1 were issued during this chunk's first K-steps, i.e.
  // AFTER slice cc+2 was requested, so the wait is a full drain; the slice has had a whole chunk to land.
#define GW_PRODUCE_CHUNK(cc)                                                              \
  {                                                                                       \
    if ((cc) <= 6) {                                                                      \
      GW_FCHUNK(acc2, in8, 0, 8, 8, 4, wait_regs<0>(ring[((cc) + 1) & 1]))                 \
    } else {                                                                              \
      GW_FCHUNK(acc2, in8, 0, 8, 8, 4, wait_vm<0>())                                       \
    }                                                                                     \
    if ((cc) + 1 < kChunksPerLayer) GW_CONSUME_SLICE(((cc) + 1) & 1, (cc) + 1)             \
  }
  GW_PRODUCE_CHUNK(0)
  GW_REQUEST_SLICE(1, 3)
  GW_PRODUCE_CHUNK(1)
  GW_REQUEST_SLICE(0, 4)
  GW_PRODUCE_CHUNK(2)
  GW_REQUEST_SLICE(1, 5)
  GW_PRODUCE_CHUNK(3)
  GW_REQUEST_SLICE(0, 6)
  GW_PRODUCE_CHUNK(4)
  GW_REQUEST_SLICE(1, 7)
  GW_PRODUCE_CHUNK(5)
  GW_PRODUCE_CHUNK(6)
  GW_PRODUCE_CHUNK(7)

  // ---- output layer; with RES the residual rows are requested underneath it ----
  float hin[64];
#pragma unroll
  for (int t = 0; t < 16; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) hin[4 * t + r] = fmaxf(acc2[t][r], 0.f);
  f32x4 rres[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int cc = 0; cc < kChunksPerLayer; ++cc) {
    if (cc + 1 < kChunksPerLayer) {
      GW_FCHUNK(o, hin, 8 * cc, 8, 8, 4, wait_vm<0>())
    } else {
      GW_FCHUNK(o, hin, 8 * cc, 8, 0, 1, wait_vm<0>())
    }
    // residual rows, requested late and in halves: by now 32 / 48 of the 64 B-operand registers are dead
    if (RES && (cc == 3 || cc == 5)) {  // (pointer recomputed here rather than kept live since the prologue)
      const float* rrow = a.res_ptr + ((size_t)b * (size_t)a.res_rows_pb + (size_t)k) * (size_t)a.res_ld + 4 * q;
      if (cc == 3) hld_half_row<0>(rres, rrow); else hld_half_row<1>(rres, rrow);
    }
  }
  if (RES) wait_regs<0>(rres);

  // ---- bias, LayerNorm over the 256 features of each column (eps 1e-5, biased variance), residual ----
#pragma unroll
  for (int t = 0; t < 16; ++t) o[t] += *(const f32x4*)(cst + kEdgeSet + kBOut + 16 * t + 4 * q);
  if (RES) {
    GW_LAYERNORM256(o, GW_LDS4, cst + kEdgeSet + kGamma, cst + kEdgeSet + kBeta, + rres[t][r])
  } else {
    GW_LAYERNORM256(o, GW_LDS4, cst + kEdgeSet + kGamma, cst + kEdgeSet + kBeta, )
  }

  // ---- stage e' through LDS, segment sum ----
  GW_STAGE_ROWS(o, gd_id)
  GW_SEGMENT_SUM_ATOMICS(a.agg)
#undef GW_CONSUME_SLICE
#undef GW_PRODUCE_CHUNK
}

inline bool node_encoder_ok(const gw_mlp_weights* w) {
  return w->weight_dtype == GW_DTYPE_F32 && w->n_mid == 1 && w->hidden == 256 && w->n_out == 256 && w->w1[0] && w->b1 && w->w_mid &&
         w->b_mid && w->w_out && w->b_out && w->ln_gamma && w->ln_beta && (w->ln_width == 0 || w->ln_width == 256);
}

}  // namespace

int gw_encoder_fused_forward(int32_t batch, int32_t n_edges, const int32_t* src, const int32_t* dst, const gw_operand* features,
                             const gw_mlp_weights* w_node, const gw_operand* x_dst, const gw_operand* e_in, const gw_operand* e_res,
                             const gw_mlp_weights* w_edge, float* agg, int32_t n_dst, const gw_activation_save* save, int32_t flags,
                             void* stream) {
  if (batch <= 0 || n_edges < 0 || n_dst <= 0 || !features || !w_node || !x_dst || !e_in || !e_res || !w_edge)
    return set_error(GW_E_BADARG, "gw_encoder_fused_forward: bad arguments");
  if (n_edges == 0) return GW_OK;  // nothing to add: agg stays as the caller zeroed it
  if (!src || !dst || !agg || !features->ptr) return set_error(GW_E_BADARG, "gw_encoder_fused_forward: bad arguments");
  if ((int64_t)batch * n_edges >= (int64_t)1 << 31 || (int64_t)batch * n_dst >= (int64_t)1 << 31)
    return set_error(GW_E_UNSUPPORTED, "gw_encoder_fused_forward: batch*edges exceeds int32");
  if (save || flags != 0)
    return set_error(GW_E_UNSUPPORTED, "gw_encoder_fused_forward: inference in atomics mode on row tiles only (no activation saves, "
                                       "no deterministic sums, no segment tiles)");
  // node encoder: fp32, one middle layer, widths 256, LayerNorm over 256, first layer packed in 28 K-steps (17 .. 112 features)
  if (!node_encoder_ok(w_node) || features->layout != GW_LAYOUT_ROWS_F32 || features->projected || features->index ||
      features->k <= 16 || features->k > 112 || features->ld < features->k || features->rows_per_batch <= 0 ||
      (w_node->k_in > 0 && w_node->k_in != features->k))
    return set_error(GW_E_UNSUPPORTED, "gw_encoder_fused_forward: float32 node encoder with one middle layer, widths 256, LayerNorm "
                                       "over 256 and 17..112 input features as fp32 rows");
  // edge MLP: the raw operand is the node encoder's output; x_dst / e_in are projected fp32 rows (elds_kernel<true, 1 | 2>)
  gw_operand raw;
  memset(&raw, 0, sizeof(raw));
  raw.ptr = features->ptr;  // (stands for the rows that never exist: 256 wide fp32 rows, not projected)
  raw.rows_per_batch = features->rows_per_batch;
  raw.ld = 256;
  raw.k = 256;
  raw.layout = GW_LAYOUT_ROWS_F32;
  const gw_operand* pops[2] = {x_dst, e_in};
  EncfArgs a;
  memset(&a, 0, sizeof(a));
  int n_proj = 0;
  for (int i = 0; i < 2; ++i) {
    if (pops[i]->k == 0) continue;
    if (!pops[i]->projected || pops[i]->layout != GW_LAYOUT_ROWS_F32 || pops[i]->k != 256 || pops[i]->ld % 4 != 0 || !pops[i]->ptr)
      return set_error(GW_E_UNSUPPORTED, "gw_encoder_fused_forward: x_dst / e_in are projected 256-wide fp32 rows (or k = 0)");
    a.p_ptr[n_proj] = pops[i]->ptr;
    a.p_rows_pb[n_proj] = pops[i]->rows_per_batch;
    a.p_ld[n_proj] = pops[i]->ld;
    a.p_kind[n_proj] = i + 1;
    ++n_proj;
  }
  if (w_edge->hidden != 256 || w_edge->n_out != 256 || !w_edge->b1 || !w_edge->w_out || !w_edge->b_out || !w_edge->w1[0] || n_proj == 0 ||
      !gw::edge_lds_eligible(&raw, x_dst, e_in, w_edge))
    return set_error(GW_E_UNSUPPORTED, "gw_encoder_fused_forward: float32 edge MLP with one middle layer, widths 256, LayerNorm over "
                                       "256, its x_src slice packed and one or two projected operands");
  const bool res = e_res->k != 0;
  if (res && (e_res->k != 256 || e_res->ld % 4 != 0 || !e_res->ptr || e_res->layout != GW_LAYOUT_ROWS_F32))
    return set_error(GW_E_UNSUPPORTED, "gw_encoder_fused_forward: e_res (residual edge features) must be 256-wide fp32 rows (or k = 0)");
  a.n_cols = batch * n_edges;
  a.n_edges = n_edges;
  a.n_dst = n_dst;
  a.src = src;
  a.dst = dst;
  a.feat = features->ptr;
  a.feat_rows_pb = features->rows_per_batch;
  a.feat_ld = features->ld;
  a.k_valid = features->k;
  a.n_w1 = w_node->w1[0];
  a.n_w_mid = w_node->w_mid;
  a.n_w_out = w_node->w_out;
  a.n_const[0] = w_node->b1;
  a.n_const[1] = w_node->b_mid;
  a.n_const[2] = w_node->b_out;
  a.n_const[3] = w_node->ln_gamma;
  a.n_const[4] = w_node->ln_beta;
  a.w_raw = w_edge->w1[0];
  a.w_mid = w_edge->w_mid;
  a.w_out = w_edge->w_out;
  a.e_const[0] = w_edge->b1;
  a.e_const[1] = w_edge->b_mid;
  a.e_const[2] = w_edge->b_out;
  a.e_const[3] = w_edge->ln_gamma;
  a.e_const[4] = w_edge->ln_beta;
  if (res) {
    a.res_ptr = e_res->ptr;
    a.res_rows_pb = e_res->rows_per_batch;
    a.res_ld = e_res->ld;
  }
  a.agg = agg;
  fill_tile_schedule(a, (a.n_cols + kColsPerWG - 1) / kColsPerWG, 6);  // 28 of 64 K-steps + five full passes
  const char* what = "encfused_kernel launch";
  if (res)
    return n_proj == 1 ? launch_tile_kernel(encfused_kernel<true, 1>, a, kEncfLdsBytes, what, stream)
                       : launch_tile_kernel(encfused_kernel<true, 2>, a, kEncfLdsBytes, what, stream);
  return n_proj == 1 ? launch_tile_kernel(encfused_kernel<false, 1>, a, kEncfLdsBytes, what, stream)
                     : launch_tile_kernel(encfused_kernel<false, 2>, a, kEncfLdsBytes, what, stream);
}
