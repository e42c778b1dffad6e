// gw_edge_lds.hip - the inference form of the fp32 edge update with residual: constants in LDS.
//
//     e' = LN(W_out . relu(W_mid . relu(b1 + [W_raw . raw] + sum_p P_p[row_p]) + b_mid) + b_out) + e_res
//     agg[dst] += e'
//
// for the launches of the processor (blocks 1..8: one raw operand, two projected), the encoder (one raw, one or two projected)
// and processor block 0 (nothing raw, three projected) in inference: one middle layer, no activation saving, atomics mode.
// The tile map, the weight ring, the chunk hand-over, the MFMA order and every arithmetic expression are edge_kernel's
// (gw_edge.hip, gw_edge_common.hpp), so results are bit for bit the same; what differs is where the constants come from:
//   * b1, b_mid, b_out, gamma, beta are copied to LDS at kernel start (behind the staging area and the destination ids, as in
//     gw_edge_stream.hip) and read from there.  Of the 146 vector-memory instructions a wave issued per tile, the 80 that
//     fetched these same 5 KiB are gone: the layer-1 accumulator (raw forms) and the middle layer's start from ds_read_b128,
//     the layer-1 bias of the non-raw form is no ring member, and the LayerNorm epilogue waits for no global load,
//   * the last raw chunk's hand-over waits for nothing but its DMA (no bias row arrives underneath it).
// Kept: the raw row load, the two-slot ring of projected slices, the residual rows requested in halves under the output layer,
// the staging through LDS with the row-coalesced e' store, the ballot walk of the segment sum.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "gw_device.hpp"
#include "gw_edge_common.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

constexpr int kEldsLdsBytes = (kConstOff + kConstSetFloats) * 4;
static_assert(kEldsLdsBytes == 71936, "staging + destination ids + one set of constants");
static_assert(2 * kEldsLdsBytes <= 160 * 1024, "two workgroups per CU must fit the 160 KiB of LDS");

struct EldsArgs {
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
  // raw operand (RAW kernels): full 256-float rows, multiplied by w_raw on the matrix cores
  const float* raw_ptr;
  int raw_rows_pb;
  int raw_ld;
  int raw_kind;  // 0: row = src[k], 1: dst[k], 2: k
  const float* w_raw;
  // projected operands: rows already hold X . W1_slice^T, gathered and added
  const float* p_ptr[3];
  int p_rows_pb[3];
  int p_ld[3];
  int p_kind[3];
  const float* b1;
  const float* w_mid;
  const float* b_mid;
  const float* w_out;
  const float* b_out;
  const float* gamma;
  const float* beta;
  // residual e rows (indexed by edge), outputs
  const float* res_ptr;
  int res_rows_pb;
  int res_ld;
  float* e_out;
  float* agg;
};

// Source of weight chunk i of a tile: [w_raw (8 chunks)] w_mid (8) w_out (8).
template <bool RAW>
__device__ __forceinline__ const float* chunk_src(const EldsArgs& a, int i) {
  if (RAW) {
    if (i < kChunksPerLayer) return a.w_raw + (size_t)i * kChunkFloats;
    i -= kChunksPerLayer;
  }
  if (i < kChunksPerLayer) return a.w_mid + (size_t)i * kChunkFloats;
  return a.w_out + (size_t)(i - kChunksPerLayer) * kChunkFloats;
}

// the counted wait of the prologue: the two indices and the five constants have landed, N younger requests stay in flight
template <int N>
__device__ __forceinline__ void wait_prologue(int& s, int& d, float (&c)[5]) {
  asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(s), "+v"(d), "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]) : [n] "n"(N) : "memory");
}

template <bool RAW, int NPROJ>
__global__ __launch_bounds__(kThreads, 2) void elds_kernel(const EldsArgs a) {
  float* const lds = lds_base();
  const float* const cst = lds + kConstOff;
  GW_TILE_COORDS(a.n_cols, a.n_edges, a.xcd_base, a.xcd_rem)
  stagger_start(a.stagger);

  // ---- prologue.  Issue order matters for the counted waits (vmcnt retires in order) ----
  int s_idx = hldi(a.src + k);
  int d_idx = hldi(a.dst + k);
  float cv[5];  // thread f carries feature f of the five constant vectors to LDS; they travel with the indices
  {
    const int f = threadIdx.x;
    cv[0] = hld1(a.b1 + f);
    cv[1] = hld1(a.b_mid + f);
    cv[2] = hld1(a.b_out + f);
    cv[3] = hld1(a.gamma + f);
    cv[4] = hld1(a.beta + f);
  }
  issue_chunk32k(chunk_src<RAW>(a, 0), lds, lane, wave);
  int ci = 0;  // chunk counter of this tile (wave uniform); chunk i lives in LDS buffer i & 1
  wait_prologue<8>(s_idx, d_idx, cv);  // the 8 DMA pieces stay in flight
  consts_to_lds(lds, 0, cv);

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
  // non-raw form: the layer-1 bias of slice `slice` from LDS (two registers, read one chunk before they are added)
#define GW_BIAS_SLICE(slice)                                                   \
  if (!RAW) {                                                                  \
    bb0 = *(const f32x4*)(cst + kB1 + 32 * (slice) + 4 * q);                   \
    bb1 = *(const f32x4*)(cst + kB1 + 32 * (slice) + 16 + 4 * q);              \
  }
  // B operand of produce chunk `slice` from ring slot `slot`: the layer-1 accumulator tiles (raw forms; they started from b1)
  // plus the gathered rows, or the gathered rows plus the bias, which is added last - the place edge_kernel's ring member had
#define GW_CONSUME_SLICE(slot, slice)                                          \
  {                                                                            \
    f32x4 v0_, v1_;                                                            \
    if (RAW) {                                                                 \
      v0_ = acc[2 * (slice)] + ring[slot][0][0];                               \
      v1_ = acc[2 * (slice) + 1] + ring[slot][0][1];                           \
    } else {                                                                   \
      v0_ = ring[slot][0][0];                                                  \
      v1_ = ring[slot][0][1];                                                  \
    }                                                                          \
    _Pragma("unroll") for (int p = 1; p < NPROJ; ++p) {                        \
      v0_ += ring[slot][p][0];                                                 \
      v1_ += ring[slot][p][1];                                                 \
    }                                                                          \
    if (!RAW) {                                                                \
      v0_ += bb0;                                                              \
      v1_ += bb1;                                                              \
    }                                                                          \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                            \
      in8[r] = fmaxf(v0_[r], 0.f);                                             \
      in8[4 + r] = fmaxf(v1_[r], 0.f);                                         \
    }                                                                          \
  }

  f32x4 a_cur[4];  // A fragments of the next K-step to run
  f32x4 acc[16];   // layer-1 accumulator (RAW only)
  f32x4 acc2[16];  // first hidden layer accumulator
  float in8[8];    // B operand values of the next chunk
  f32x4 bb0, bb1;  // (non-raw form)
  if (RAW) {
    const int r = a.raw_kind == 0 ? s_idx : (a.raw_kind == 1 ? d_idx : k);
    const float* xrow = a.raw_ptr + ((size_t)b * (size_t)a.raw_rows_pb + (size_t)r) * (size_t)a.raw_ld + 4 * q;
    f32x4 xv[16];
    hld_row(xv, xrow);
    wait_regs<0>(xv);  // chunk 0 and x have landed
    lds_barrier();     // ... everybody's share of chunk 0 and of the constants
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = *(const f32x4*)(cst + kB1 + 16 * t + 4 * q);
#pragma unroll
    for (int b4 = 0; b4 < 4; ++b4) a_cur[b4] = *(const f32x4*)(lds + lane * 4 + b4 * 256);
    float x[64];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      x[4 * i + 0] = xv[i].x;
      x[4 * i + 1] = xv[i].y;
      x[4 * i + 2] = xv[i].z;
      x[4 * i + 3] = xv[i].w;
    }
#pragma unroll
    for (int cc = 0; cc < kChunksPerLayer; ++cc) {
#pragma unroll
      for (int i = 0; i < 8; ++i) in8[i] = x[8 * cc + i];
      if (cc == kChunksPerLayer - 3) {  // the first two ring slices, once most of x is dead
        GW_REQUEST_SLICE(0, 0)
        GW_REQUEST_SLICE(1, 1)
      }
      if (cc == kChunksPerLayer - 1) {  // next layer's bias, under the last chunk (x is dead)
#pragma unroll
        for (int t = 0; t < 16; ++t) acc2[t] = *(const f32x4*)(cst + kBMid + 16 * t + 4 * q);
      }
      GW_CHUNK(acc, in8, true, wait_vm<0>(), chunk_src<RAW>(a, ci + 1))
    }
    wait_regs<0>(ring[0]);  // (landed long ago: everything was drained by the vmcnt(0) boundaries above)
    wait_regs<0>(ring[1]);
    GW_CONSUME_SLICE(0, 0)
    GW_REQUEST_SLICE(0, 2)
  } else {
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
  }

  // ---- first hidden layer: B operand produced slice by slice = relu(layer-1 accumulator + gathered rows) ----
  // boundary into produce chunk cc+1: the pieces of chunk cc+1 were issued during this chunk's first K-steps, i.e.
  // AFTER slice cc+2 was requested, so the wait is a full drain; the slice has had a whole chunk to land.
#define GW_PRODUCE_CHUNK(cc)                                                              \
  {                                                                                       \
    if ((cc) + 1 < kChunksPerLayer) GW_BIAS_SLICE((cc) + 1)                                \
    if ((cc) <= 6) {                                                                      \
      GW_CHUNK(acc2, in8, true, wait_regs<0>(ring[((cc) + 1) & 1]), chunk_src<RAW>(a, ci + 1))                        \
    } else {                                                                              \
      GW_CHUNK(acc2, in8, true, wait_vm<0>(), chunk_src<RAW>(a, ci + 1))                                              \
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

  // ---- output layer; the residual rows are requested underneath it ----
  float hin[64];
#pragma unroll
  for (int t = 0; t < 16; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) hin[4 * t + r] = fmaxf(acc2[t][r], 0.f);
  f32x4 o[16];
  f32x4 rres[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int cc = 0; cc < kChunksPerLayer; ++cc) {
#pragma unroll
    for (int i = 0; i < 8; ++i) in8[i] = hin[8 * cc + i];
    if (cc + 1 < kChunksPerLayer) {
      GW_CHUNK(o, in8, true, wait_vm<0>(), chunk_src<RAW>(a, ci + 1))
    } else {
      GW_CHUNK(o, in8, false, wait_vm<0>(), chunk_src<RAW>(a, ci + 1))
    }
    // residual rows, requested late and in halves: by now 32 / 48 of the 64 B-operand registers are dead
    if (cc == 3 || cc == 5) {  // (pointer recomputed here rather than kept live since the prologue)
      const float* rrow = a.res_ptr + ((size_t)b * (size_t)a.res_rows_pb + (size_t)k) * (size_t)a.res_ld + 4 * q;
      if (cc == 3) hld_half_row<0>(rres, rrow); else hld_half_row<1>(rres, rrow);
    }
  }
  wait_regs<0>(rres);

  // ---- bias, LayerNorm over the 256 features of each column (eps 1e-5, biased variance), residual ----
#pragma unroll
  for (int t = 0; t < 16; ++t) o[t] += *(const f32x4*)(cst + kBOut + 16 * t + 4 * q);
  GW_LAYERNORM256(o, GW_LDS4, cst + kGamma, cst + kBeta, + rres[t][r])

  // ---- stage e' through LDS, e_out rows, segment sum ----
  GW_STAGE_ROWS(o, gd_id)
  if (a.e_out != nullptr) store_e_rows(lds, a.e_out, tile_c0, a.n_cols, wave, lane);
  GW_SEGMENT_SUM_ATOMICS(a.agg)
#undef GW_BIAS_SLICE
#undef GW_CONSUME_SLICE
#undef GW_PRODUCE_CHUNK
}

inline bool f32_rows(const gw_operand* op) { return op->layout == GW_LAYOUT_ROWS_F32; }

// raw / projected operand counts of a launch; false if an operand is no fp32 row table
inline bool count_operands(const gw_operand* x_src, const gw_operand* x_dst, const gw_operand* e_in, int& n_raw, int& n_proj) {
  const gw_operand* ops[3] = {x_src, x_dst, e_in};
  n_raw = n_proj = 0;
  for (int i = 0; i < 3; ++i) {
    if (ops[i]->k == 0) continue;
    if (!f32_rows(ops[i])) return false;
    if (ops[i]->projected) ++n_proj; else ++n_raw;
  }
  return true;
}

}  // namespace

namespace gw {

bool edge_lds_eligible(const gw_operand* x_src, const gw_operand* x_dst, const gw_operand* e_in, const gw_mlp_weights* w) {
  if (w->weight_dtype != GW_DTYPE_F32 || w->n_mid != 1 || !w->ln_gamma || !w->ln_beta || !w->w_mid || !w->b_mid) return false;
  if (w->ln_width > 0 && w->ln_width != 256) return false;
  int n_raw, n_proj;
  if (!count_operands(x_src, x_dst, e_in, n_raw, n_proj)) return false;
  if (!(n_raw == 1 ? (n_proj == 1 || n_proj == 2) : (n_raw == 0 && n_proj == 3))) return false;
  static const int impl = GW_TUNE("GW_EDGE_LDS", 1);  // 0: these launches keep edge_kernel (A/B measurements)
  return impl != 0 && edge_fast_eligible(x_src, x_dst, e_in, w);
}

int edge_lds_launch(int32_t batch, int32_t n_edges, const int32_t* src, const int32_t* dst, const gw_operand* x_src,
                    const gw_operand* x_dst, const gw_operand* e_in, const gw_operand* e_res, const gw_mlp_weights* w, float* e_out,
                    float* agg, int32_t n_dst, void* stream) {
  EldsArgs a;
  memset(&a, 0, sizeof(a));
  a.n_cols = batch * n_edges;
  a.n_edges = n_edges;
  a.n_dst = n_dst;
  const int tiles = (a.n_cols + kColsPerWG - 1) / kColsPerWG;
  a.src = src;
  a.dst = dst;
  const gw_operand* ops[3] = {x_src, x_dst, e_in};
  int n_proj = 0, n_raw = 0;
  for (int i = 0; i < 3; ++i) {
    if (ops[i]->k == 0) continue;
    if (!ops[i]->projected) {
      if (n_raw == 1) return set_error(GW_E_UNSUPPORTED, "edge_lds_launch: at most one raw operand");
      ++n_raw;
      a.raw_ptr = ops[i]->ptr;
      a.raw_rows_pb = ops[i]->rows_per_batch;
      a.raw_ld = ops[i]->ld;
      a.raw_kind = i;
      a.w_raw = w->w1[i];
    } else {
      if (n_proj == 3) return set_error(GW_E_UNSUPPORTED, "edge_lds_launch: at most three projected operands");
      a.p_ptr[n_proj] = ops[i]->ptr;
      a.p_rows_pb[n_proj] = ops[i]->rows_per_batch;
      a.p_ld[n_proj] = ops[i]->ld;
      a.p_kind[n_proj] = i;
      ++n_proj;
    }
  }
  if (!(n_raw == 1 ? (n_proj == 1 || n_proj == 2) : n_proj == 3) || (n_raw == 1 && !a.w_raw))
    return set_error(GW_E_UNSUPPORTED, "edge_lds_launch: one raw operand with one or two projected, or three projected operands");
  a.b1 = w->b1;
  a.w_mid = w->w_mid;
  a.b_mid = w->b_mid;
  a.w_out = w->w_out;
  a.b_out = w->b_out;
  a.gamma = w->ln_gamma;
  a.beta = w->ln_beta;
  a.res_ptr = e_res->ptr;
  a.res_rows_pb = e_res->rows_per_batch;
  a.res_ld = e_res->ld;
  a.e_out = e_out;
  a.agg = agg;
  fill_tile_schedule(a, tiles, 2 + n_raw);     // [raw layer-1 pass +] middle layer + output layer
  if (a.skip != 4 && a.skip != 5) a.skip = 0;  // (only the chunk macro's switches apply here)
  const char* what = "elds_kernel launch";
  if (n_raw == 1)
    return n_proj == 1 ? launch_tile_kernel(elds_kernel<true, 1>, a, kEldsLdsBytes, what, stream)
                       : launch_tile_kernel(elds_kernel<true, 2>, a, kEldsLdsBytes, what, stream);
  return launch_tile_kernel(elds_kernel<false, 3>, a, kEldsLdsBytes, what, stream);
}

}  // namespace gw
