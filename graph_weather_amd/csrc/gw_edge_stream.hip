// gw_edge_stream.hip - the decoder form of the fp32 edge update: constants in LDS, no residual stream.
//
//     agg[dst] += LN(W_out . relu(W_mid . relu(b1 + sum_p P_p[row_p]) + b_mid) + b_out)
//
// for launches that have nothing raw, one or two projected operands, NO residual and no e' output (the decoder: e' is
// dropped and the segment sums of its batch-shared e enter the node update as a cached product).
// The weight ring, the chunk hand-over, the MFMA order and every arithmetic expression are edge_kernel's (gw_edge.hip,
// gw_edge_common.hpp); what differs is what surrounds the passes:
//   * b1, b_mid, b_out, gamma, beta are copied to LDS at kernel start (behind the staging area and the destination ids) and
//     read from there: no vector-memory instruction fetches a constant, and the layer-1 bias is no ring member,
//   * no residual rows are streamed (and none of the 64 registers that held them through the output layer is needed).
// One workgroup per 64-column tile, in edge_kernel's XCD-aware order.  (A persistent tile loop with next-tile prefetch was
// built and measured slower than this; DESIGN.md section 4 keeps the table.)

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "gw_device.hpp"
#include "gw_edge_common.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

constexpr int kStreamLdsBytes = (kConstOff + kConstSetFloats) * 4;  // staging + destination ids + one set of constants
static_assert(2 * kStreamLdsBytes <= 160 * 1024, "two workgroups per CU must fit the 160 KiB of LDS");

struct StreamArgs {
  int n_cols;  // batch * n_edges
  int n_edges;
  int n_dst;
  int stagger;
  int skip;  // (tuning builds: read by GW_CHUNK)
  int dma6;
  int xcd_base;  // XCD-aware tile order, as in edge_kernel (0: identity)
  int xcd_rem;
  const int* src;
  const int* dst;
  // projected operands: rows already hold X . W1_slice^T, gathered and added
  const float* p_ptr[2];
  int p_rows_pb[2];
  int p_ld[2];
  int p_kind[2];  // 0: row = src[k], 1: dst[k], 2: k
  const float* b1;
  const float* w_mid;
  const float* b_mid;
  const float* w_out;
  const float* b_out;
  const float* gamma;
  const float* beta;
  float* agg;
};

// Source of weight chunk i of a tile: w_mid (8 chunks) w_out (8).
__device__ __forceinline__ const float* chunk_src(const StreamArgs& a, int i) {
  if (i < kChunksPerLayer) return a.w_mid + (size_t)i * kChunkFloats;
  return a.w_out + (size_t)(i - kChunksPerLayer) * kChunkFloats;
}

template <int NPROJ>
__global__ __launch_bounds__(kThreads, 2) void estream_kernel(const StreamArgs a) {
  float* const lds = lds_base();
  const float* const cst = lds + kConstOff;
  GW_TILE_COORDS(a.n_cols, a.n_edges, a.xcd_base, a.xcd_rem)
  stagger_start(a.stagger);

  // ---- prologue.  Issue order matters for the counted waits (vmcnt retires in order) ----
  int s_idx = hldi(a.src + k);
  int d_idx = hldi(a.dst + k);
  issue_chunk32k(chunk_src(a, 0), lds, lane, wave);
  int ci = 0;  // chunk counter of this tile (wave uniform); chunk i lives in LDS buffer i & 1
  {  // constants to LDS while the indices travel (hipcc counts these loads: its wait in front of the LDS writes is a full drain)
    const int f = threadIdx.x;
    const float cv[5] = {ldg1(a.b1 + f), ldg1(a.b_mid + f), ldg1(a.b_out + f), ldg1(a.gamma + f), ldg1(a.beta + f)};
    consts_to_lds(lds, 0, cv);
  }
  wait_regs<0>(s_idx, d_idx);

  const float* prow[NPROJ];
#pragma unroll
  for (int p = 0; p < NPROJ; ++p) {
    const int r = a.p_kind[p] == 0 ? s_idx : (a.p_kind[p] == 1 ? d_idx : k);
    prow[p] = a.p_ptr[p] + ((size_t)b * (size_t)a.p_rows_pb[p] + (size_t)r) * (size_t)a.p_ld[p] + 4 * q;
  }
  const int gd_id = valid ? b * a.n_dst + d_idx : -1;  // global destination row of this column (segment-sum key)

  // ring[s & 1][p][h]: features 32s + 16h + 4q .. +3 of projected operand p = its part of the B operand of produce
  // chunk s.  Slice s is requested when slice s-2 has been consumed (end of chunk s-3) and consumed at the end of chunk s-1.
  f32x4 ring[2][NPROJ][2];
  // the layer-1 bias of slice `slice` from LDS (two registers, read one chunk before they are added)
#define GW_BIAS_SLICE(slice)                                                   \
  {                                                                            \
    bb0 = *(const f32x4*)(cst + kB1 + 32 * (slice) + 4 * q);                   \
    bb1 = *(const f32x4*)(cst + kB1 + 32 * (slice) + 16 + 4 * q);              \
  }
  // B operand of produce chunk `slice` from ring slot `slot`: the bias is added last, as in edge_kernel
#define GW_CONSUME_SLICE(slot, slice)                                          \
  {                                                                            \
    f32x4 v0_ = ring[slot][0][0], v1_ = ring[slot][0][1];                      \
    _Pragma("unroll") for (int p = 1; p < NPROJ; ++p) {                        \
      v0_ += ring[slot][p][0];                                                 \
      v1_ += ring[slot][p][1];                                                 \
    }                                                                          \
    v0_ += bb0;                                                                \
    v1_ += bb1;                                                                \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                            \
      in8[r] = fmaxf(v0_[r], 0.f);                                             \
      in8[4 + r] = fmaxf(v1_[r], 0.f);                                         \
    }                                                                          \
  }

  f32x4 a_cur[4];  // A fragments of the next K-step to run
  f32x4 acc2[16];  // first hidden layer accumulator
  float in8[8];    // B operand values of the next chunk
  f32x4 bb0, bb1;
  GW_REQUEST_SLICE(0, 0)
  GW_REQUEST_SLICE(1, 1)
  wait_regs<2 * NPROJ>(ring[0]);  // chunk 0 and slice 0 have landed; slice 1 stays in flight
  lds_barrier();                  // ... everybody's share of chunk 0 and of the constants
#pragma unroll
  for (int t = 0; t < 16; ++t) acc2[t] = *(const f32x4*)(cst + kBMid + 16 * t + 4 * q);
  GW_BIAS_SLICE(0)
#pragma unroll
  for (int b4 = 0; b4 < 4; ++b4) a_cur[b4] = *(const f32x4*)(lds + lane * 4 + b4 * 256);
  GW_CONSUME_SLICE(0, 0)
  GW_REQUEST_SLICE(0, 2)

  // ---- first hidden layer: B operand produced slice by slice = relu(gathered rows + bias) ----
  // boundary into produce chunk cc+1: the pieces of chunk cc+1 were issued during this chunk's first K-steps, i.e.
  // AFTER slice cc+2 was requested, so the wait is a full drain; the slice has had a whole chunk to land.
#define GW_PRODUCE_CHUNK(cc)                                                              \
  {                                                                                       \
    if ((cc) + 1 < kChunksPerLayer) GW_BIAS_SLICE((cc) + 1)                                \
    if ((cc) <= 6) {                                                                      \
      GW_CHUNK(acc2, in8, true, wait_regs<0>(ring[((cc) + 1) & 1]), chunk_src(a, ci + 1))                        \
    } else {                                                                              \
      GW_CHUNK(acc2, in8, true, wait_vm<0>(), chunk_src(a, ci + 1))                                              \
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

  // ---- output layer ----
  float hin[64];
#pragma unroll
  for (int t = 0; t < 16; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) hin[4 * t + r] = fmaxf(acc2[t][r], 0.f);
  f32x4 o[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int cc = 0; cc < kChunksPerLayer; ++cc) {
#pragma unroll
    for (int i = 0; i < 8; ++i) in8[i] = hin[8 * cc + i];
    if (cc + 1 < kChunksPerLayer) {
      GW_CHUNK(o, in8, true, wait_vm<0>(), chunk_src(a, ci + 1))
    } else {
      GW_CHUNK(o, in8, false, wait_vm<0>(), chunk_src(a, ci + 1))
    }
  }

  // ---- bias, LayerNorm, staging through LDS, segment sum ----
#pragma unroll
  for (int t = 0; t < 16; ++t) o[t] += *(const f32x4*)(cst + kBOut + 16 * t + 4 * q);
  GW_LAYERNORM256(o, GW_LDS4, cst + kGamma, cst + kBeta, )
  GW_STAGE_ROWS(o, gd_id)
  GW_SEGMENT_SUM_ATOMICS(a.agg)
#undef GW_BIAS_SLICE
#undef GW_CONSUME_SLICE
#undef GW_PRODUCE_CHUNK
}

inline bool is_proj_f32(const gw_operand* op) { return op->k > 0 && op->projected && op->layout == GW_LAYOUT_ROWS_F32; }

}  // namespace

namespace gw {

bool edge_stream_eligible(const gw_operand* x_src, const gw_operand* x_dst, const gw_operand* e_in, const gw_mlp_weights* w) {
  if (w->weight_dtype != GW_DTYPE_F32 || w->n_mid != 1 || !w->ln_gamma || !w->ln_beta || !w->w_mid || !w->b_mid) return false;
  if (w->ln_width > 0 && w->ln_width != 256) return false;
  const gw_operand* ops[3] = {x_src, x_dst, e_in};
  int n_proj = 0;
  for (int i = 0; i < 3; ++i) {
    if (ops[i]->k == 0) continue;
    if (!is_proj_f32(ops[i])) return false;  // a raw operand, or a 16-bit table format
    ++n_proj;
  }
  return n_proj == 1 || n_proj == 2;
}

int edge_stream_launch(int32_t batch, int32_t n_edges, const int32_t* src, const int32_t* dst, const gw_operand* x_src,
                       const gw_operand* x_dst, const gw_operand* e_in, const gw_mlp_weights* w, float* agg, int32_t n_dst,
                       void* stream) {
  StreamArgs a;
  memset(&a, 0, sizeof(a));
  a.n_cols = batch * n_edges;
  a.n_edges = n_edges;
  a.n_dst = n_dst;
  const int tiles = (a.n_cols + kColsPerWG - 1) / kColsPerWG;
  a.src = src;
  a.dst = dst;
  const gw_operand* ops[3] = {x_src, x_dst, e_in};
  int n_proj = 0;
  for (int i = 0; i < 3; ++i) {
    if (ops[i]->k == 0) continue;
    if (n_proj == 2) return set_error(GW_E_UNSUPPORTED, "edge_stream_launch: at most two projected operands");
    a.p_ptr[n_proj] = ops[i]->ptr;
    a.p_rows_pb[n_proj] = ops[i]->rows_per_batch;
    a.p_ld[n_proj] = ops[i]->ld;
    a.p_kind[n_proj] = i;
    ++n_proj;
  }
  if (n_proj == 0) return set_error(GW_E_UNSUPPORTED, "edge_stream_launch: no projected operand");
  a.b1 = w->b1;
  a.w_mid = w->w_mid;
  a.b_mid = w->b_mid;
  a.w_out = w->w_out;
  a.b_out = w->b_out;
  a.gamma = w->ln_gamma;
  a.beta = w->ln_beta;
  a.agg = agg;
  fill_tile_schedule(a, tiles, 2);            // middle layer + output layer
  if (a.skip != 4 && a.skip != 5) a.skip = 0;  // (only the chunk macro's switches apply here)
  const char* what = "estream_kernel launch";
  return n_proj == 1 ? launch_tile_kernel(estream_kernel<1>, a, kStreamLdsBytes, what, stream)
                     : launch_tile_kernel(estream_kernel<2>, a, kStreamLdsBytes, what, stream);
}

}  // namespace gw
