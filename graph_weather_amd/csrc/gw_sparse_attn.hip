// gw_sparse_attn.hip - masked multi-head attention over a sparse [n_rows, n_cols] mask (the SparseAttention of GenCast's
// experimental sparse processor, graph_weather/models/gencast/layers/experimental/sparse_transformer.py).
//
//   Entry t of the row-sorted mask attends from row i to column col[t]; per head h, with q scaled by `scale` on load,
//     s_t = scale q[i, h] . k[col[t], h],  p = softmax of s over the entries of row i,  out[i, h] = sum_t p_t v[col[t], h].
//   Rows are in the head-major working layout: head h is the contiguous segment [h dh, (h + 1) dh) of a row of heads * dh floats.
//
//   sp_fwd_kernel      one wave per (copy, row) covers ALL heads: lane group g = lane / (64 / heads) owns head g, its lanes hold
//                      16-byte pieces of the head's segment, a score is a sum inside the group (log2(64 / heads) shuffles) and
//                      every group runs its own online softmax.  The q row stays in registers, the whole k and v rows of U entries
//                      are gathered with 16-byte loads (U x 2 rows in flight per wave).  Nothing of size E x D or E x heads is
//                      written; the score maximum and log sum exp per (row, head) go to two planes.
//   sp_bwd_row_kernel  backward by recomputation from q, k and the planes: delta = rowsum(dout o out) per head, then the same walk
//                      forms dq (with respect to the unscaled q).
//   sp_bwd_col_kernel  one wave per (copy, column) walks the column-sorted positions and writes dk and dv.
//   sp_*_gen_kernel    any heads and dim_head (heads that do not divide 64, a dim_head that is no multiple of 4, rows above 2048
//                      floats, unaligned tables): one wave per workgroup and (copy, row), the heads in order, running rows in LDS,
//                      everything else streamed.  Coverage, not speed.
//   `batch` copies of one mask share the plan; copy b's rows start at b n_rows (q, out, dq, dout) and b n_cols (k, v, dk, dv).
//
// fp32, plain stores, no atomics, every sum in one fixed order: equal inputs give bitwise equal results; every row of out, dq, dk
// and dv is written once.  A row of any length is one wave's serial walk.  No host synchronisation.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gw_amd.h"
#include "gw_device.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

constexpr int kSpMaxRow = 4096;   // heads * dim_head
constexpr int kSpFastRow = 2048;  // widest row of the register path (8 x 16 bytes per lane)

struct SpArgs {
  int n_rows, n_cols, heads, dh, batch;
  int G;                   // lanes per head group of the register path: 64 / heads
  float scale;
  const int* row_ptr;      // [n_rows + 1]
  const int* col;          // [E] column of row-sorted entry t
  const int* row;          // [E] row of row-sorted entry t (column pass)
  const int* col_pos;      // [E] row-sorted positions grouped by column (column pass)
  const int* col_ptr;      // [n_cols + 1]
  const float *q, *k, *v;
  long long ld_q, ld_k, ld_v;
  float* out;              // forward: written; backward: the forward's rows
  long long ld_out;
  float* lse;              // [2][batch n_rows heads]
  long long planes;        // batch * n_rows * heads
  const float* dout;
  long long ld_dout;
  float* delta;            // [batch n_rows heads]
  float *dq, *dk, *dv;
  long long ld_dq, ld_dk, ld_dv;
};

__device__ __forceinline__ SpArgs sp_copy(SpArgs a, long long b) {
  const long long rr = b * a.n_rows, rc = b * a.n_cols;
  a.q += rr * a.ld_q, a.k += rc * a.ld_k, a.v += rc * a.ld_v;
  if (a.out != nullptr) a.out += rr * a.ld_out;
  a.lse += rr * a.heads;
  if (a.dout != nullptr) a.dout += rr * a.ld_dout;
  if (a.delta != nullptr) a.delta += rr * a.heads;
  if (a.dq != nullptr) a.dq += rr * a.ld_dq;
  if (a.dk != nullptr) a.dk += rc * a.ld_dk;
  if (a.dv != nullptr) a.dv += rc * a.ld_dv;
  return a;
}

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sums over the G lanes (a power of two) of a head group; every lane of the group gets the total
template <int N>
__device__ __forceinline__ void group_sum(float (&s)[N], int G) {
  for (int o = G >> 1; o > 0; o >>= 1) {
#pragma unroll
    for (int u = 0; u < N; ++u) s[u] += __shfl_xor(s[u], o);
  }
}

// A lane's part of a row: NJ pieces of 4 floats at segment offsets 4 gl + 4 G j of head h (columns h dh + that); pieces past the
// head's end hold zeros, so dot products need no guard.
template <int NJ>
struct HFrag {
  f32x4 r[NJ];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int j = 0; j < NJ; ++j) r[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __device__ __forceinline__ void load(const float* __restrict__ p, int off, int step, int dh) {  // p: start of the head's segment
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = off + step * j;
      r[j] = c < dh ? ldg4(p + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ p, int off, int step, int dh) const {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = off + step * j;
      if (c < dh) stg4(p + c, r[j]);
    }
  }
  __device__ __forceinline__ void scale(float s) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) r[j] *= s;
  }
  __device__ __forceinline__ void divide(float s) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) r[j] /= s;
  }
  __device__ __forceinline__ void axpy(float s, const HFrag& o) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      r[j].x = fmaf(s, o.r[j].x, r[j].x), r[j].y = fmaf(s, o.r[j].y, r[j].y);
      r[j].z = fmaf(s, o.r[j].z, r[j].z), r[j].w = fmaf(s, o.r[j].w, r[j].w);
    }
  }
  __device__ __forceinline__ float dot(const HFrag& o) const {  // this lane's part; group_sum makes the head's
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      s = fmaf(r[j].x, o.r[j].x, s), s = fmaf(r[j].y, o.r[j].y, s);
      s = fmaf(r[j].z, o.r[j].z, s), s = fmaf(r[j].w, o.r[j].w, s);
    }
    return s;
  }
};

// what a wave needs to know about its place: the item (copy, row or column) and the lane's head and offsets
struct SpLane {
  int h, off, step;
  long long hc;  // h * dh
  bool lead;     // first lane of its head group
};
__device__ __forceinline__ SpLane sp_lane(const SpArgs& a, int lane) {
  SpLane l;
  l.h = lane / a.G;
  const int gl = lane - l.h * a.G;
  l.off = 4 * gl, l.step = 4 * a.G, l.hc = (long long)l.h * a.dh, l.lead = gl == 0;
  return l;
}

// grid ceil(batch n_rows / 4), block 256: wave = one (copy, row), all heads
template <int NJ, int U>
__global__ __launch_bounds__(256) void sp_fwd_kernel(SpArgs a0) {
  typedef HFrag<NJ> F;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long gitem = (long long)blockIdx.x * 4 + wave;
  if (gitem >= (long long)a0.n_rows * a0.batch) return;
  const long long copy = (long long)__builtin_amdgcn_readfirstlane((int)(gitem / a0.n_rows));
  const int i = (int)(gitem - copy * a0.n_rows);
  const SpArgs a = sp_copy(a0, copy);
  const SpLane ln = sp_lane(a, lane);
  const int dh = a.dh;
  const int e0 = ldgi(a.row_ptr + i), e1 = ldgi(a.row_ptr + i + 1);
  F qf, acc;
  qf.load(a.q + (long long)i * a.ld_q + ln.hc, ln.off, ln.step, dh);
  qf.scale(a.scale);
  acc.zero();
  float m = -INFINITY, l = 0.f;
  for (int t = e0; t < e1; t += U) {
    float s[U];
    F vf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int tt = t + u < e1 ? t + u : e1 - 1;  // past the run: the last entry again, with a score of -inf
      const int j = ldgi(a.col + tt);
      F kf;
      kf.load(a.k + (long long)j * a.ld_k + ln.hc, ln.off, ln.step, dh);
      vf[u].load(a.v + (long long)j * a.ld_v + ln.hc, ln.off, ln.step, dh);
      s[u] = qf.dot(kf);
    }
    group_sum<U>(s, a.G);
    float mn = m;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      s[u] = t + u < e1 ? s[u] : -INFINITY;
      mn = fmaxf(mn, s[u]);
    }
    const float sc = expf(m - mn);  // 0 at the first step (m = -inf, mn finite: s[0] is a real entry)
    l *= sc;
    acc.scale(sc);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float p = expf(s[u] - mn);
      l += p;
      acc.axpy(p, vf[u]);
    }
    m = mn;
  }
  const bool any = e1 > e0;  // a row without entries: output 0 (and 0 in both planes, which nothing reads)
  if (any) acc.divide(l);
  if (ln.lead) {
    a.lse[(long long)i * a.heads + ln.h] = any ? m : 0.f;
    a.lse[a.planes + (long long)i * a.heads + ln.h] = any ? logf(l) : 0.f;
  }
  acc.store(a.out + (long long)i * a.ld_out + ln.hc, ln.off, ln.step, dh);
}

// grid ceil(batch n_rows / 4), block 256: wave = one (copy, row); writes delta and dq
template <int NJ, int U>
__global__ __launch_bounds__(256) void sp_bwd_row_kernel(SpArgs a0) {
  typedef HFrag<NJ> F;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long gitem = (long long)blockIdx.x * 4 + wave;
  if (gitem >= (long long)a0.n_rows * a0.batch) return;
  const long long copy = (long long)__builtin_amdgcn_readfirstlane((int)(gitem / a0.n_rows));
  const int i = (int)(gitem - copy * a0.n_rows);
  const SpArgs a = sp_copy(a0, copy);
  const SpLane ln = sp_lane(a, lane);
  const int dh = a.dh;
  const int e0 = ldgi(a.row_ptr + i), e1 = ldgi(a.row_ptr + i + 1);
  F qf, dof, dqf;
  qf.load(a.q + (long long)i * a.ld_q + ln.hc, ln.off, ln.step, dh);
  qf.scale(a.scale);
  dof.load(a.dout + (long long)i * a.ld_dout + ln.hc, ln.off, ln.step, dh);
  float dl[1];
  {
    F of;
    of.load(a.out + (long long)i * a.ld_out + ln.hc, ln.off, ln.step, dh);
    dl[0] = dof.dot(of);
  }
  group_sum<1>(dl, a.G);
  const float delta = dl[0];
  const long long ih = (long long)i * a.heads + ln.h;
  if (ln.lead) a.delta[ih] = delta;
  const float m = a.lse[ih], ll = a.lse[a.planes + ih];
  dqf.zero();
  for (int t = e0; t < e1; t += U) {
    float s[2 * U];
    F kf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int tt = t + u < e1 ? t + u : e1 - 1;
      const int j = ldgi(a.col + tt);
      F vf;
      kf[u].load(a.k + (long long)j * a.ld_k + ln.hc, ln.off, ln.step, dh);
      vf.load(a.v + (long long)j * a.ld_v + ln.hc, ln.off, ln.step, dh);
      s[u] = qf.dot(kf[u]);
      s[U + u] = dof.dot(vf);
    }
    group_sum<2 * U>(s, a.G);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float p = expf((s[u] - m) - ll);
      const float g = t + u < e1 ? p * (s[U + u] - delta) : 0.f;
      dqf.axpy(g, kf[u]);
    }
  }
  dqf.scale(a.scale);
  dqf.store(a.dq + (long long)i * a.ld_dq + ln.hc, ln.off, ln.step, dh);
}

// grid ceil(batch n_cols / 4), block 256: wave = one (copy, column); reads delta of sp_bwd_row_kernel, writes dk and dv
template <int NJ>
__global__ __launch_bounds__(256) void sp_bwd_col_kernel(SpArgs a0) {
  typedef HFrag<NJ> F;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long gitem = (long long)blockIdx.x * 4 + wave;
  if (gitem >= (long long)a0.n_cols * a0.batch) return;
  const long long copy = (long long)__builtin_amdgcn_readfirstlane((int)(gitem / a0.n_cols));
  const int j = (int)(gitem - copy * a0.n_cols);
  const SpArgs a = sp_copy(a0, copy);
  const SpLane ln = sp_lane(a, lane);
  const int dh = a.dh;
  const int s0 = ldgi(a.col_ptr + j), s1 = ldgi(a.col_ptr + j + 1);
  F kf, vf, dkf, dvf;
  kf.load(a.k + (long long)j * a.ld_k + ln.hc, ln.off, ln.step, dh);
  vf.load(a.v + (long long)j * a.ld_v + ln.hc, ln.off, ln.step, dh);
  dkf.zero();
  dvf.zero();
  for (int t = s0; t < s1; ++t) {
    const int pos = ldgi(a.col_pos + t);
    const int i = ldgi(a.row + pos);
    F qf, dof;
    qf.load(a.q + (long long)i * a.ld_q + ln.hc, ln.off, ln.step, dh);
    qf.scale(a.scale);
    dof.load(a.dout + (long long)i * a.ld_dout + ln.hc, ln.off, ln.step, dh);
    const long long ih = (long long)i * a.heads + ln.h;
    const float m = a.lse[ih], ll = a.lse[a.planes + ih], delta = a.delta[ih];
    float s[2] = {qf.dot(kf), dof.dot(vf)};
    group_sum<2>(s, a.G);
    const float p = expf((s[0] - m) - ll);
    dkf.axpy(p * (s[1] - delta), qf);
    dvf.axpy(p, dof);
  }
  dkf.store(a.dk + (long long)j * a.ld_dk + ln.hc, ln.off, ln.step, dh);
  dvf.store(a.dv + (long long)j * a.ld_dv + ln.hc, ln.off, ln.step, dh);
}

// ---- the general path: any heads and dim_head ---------------------------------------------------------------------------------
// One wave per workgroup and item, the heads in order; lane l owns columns l, l + 64, ... of a head's segment, the running rows
// live in LDS (each lane reads and writes its own columns only: no barrier).
__device__ __forceinline__ float sp_row_dot(const float* __restrict__ x, const float* __restrict__ y, int n, int lane) {
  float d = 0.f;
  for (int c = lane; c < n; c += 64) d = fmaf(ldg1(x + c), ldg1(y + c), d);
  return d;
}

__global__ __launch_bounds__(64) void sp_fwd_gen_kernel(SpArgs a0) {
  __shared__ float acc[kSpMaxRow];
  const int lane = threadIdx.x, dh = a0.dh;
  const long long copy = blockIdx.x / a0.n_rows;
  const int i = (int)(blockIdx.x - copy * a0.n_rows);
  const SpArgs a = sp_copy(a0, copy);
  const int e0 = ldgi(a.row_ptr + i), e1 = ldgi(a.row_ptr + i + 1);
  const bool any = e1 > e0;
  for (int h = 0; h < a.heads; ++h) {
    const long long hc = (long long)h * dh;
    const float* qr = a.q + (long long)i * a.ld_q + hc;
    for (int c = lane; c < dh; c += 64) acc[c] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int t = e0; t < e1; ++t) {
      const int j = ldgi(a.col + t);
      const float* kr = a.k + (long long)j * a.ld_k + hc;
      const float* vr = a.v + (long long)j * a.ld_v + hc;
      float d = 0.f;
      for (int c = lane; c < dh; c += 64) d = fmaf(ldg1(qr + c) * a.scale, ldg1(kr + c), d);
      const float s = wave_sum64(d);
      const float mn = fmaxf(m, s), sc = expf(m - mn), p = expf(s - mn);
      l = l * sc + p;
      for (int c = lane; c < dh; c += 64) acc[c] = fmaf(p, ldg1(vr + c), acc[c] * sc);
      m = mn;
    }
    if (lane == 0) {
      a.lse[(long long)i * a.heads + h] = any ? m : 0.f;
      a.lse[a.planes + (long long)i * a.heads + h] = any ? logf(l) : 0.f;
    }
    for (int c = lane; c < dh; c += 64) stg1(a.out + (long long)i * a.ld_out + hc + c, any ? acc[c] / l : 0.f);
  }
}

__global__ __launch_bounds__(64) void sp_bwd_row_gen_kernel(SpArgs a0) {
  __shared__ float acc[kSpMaxRow];
  const int lane = threadIdx.x, dh = a0.dh;
  const long long copy = blockIdx.x / a0.n_rows;
  const int i = (int)(blockIdx.x - copy * a0.n_rows);
  const SpArgs a = sp_copy(a0, copy);
  const int e0 = ldgi(a.row_ptr + i), e1 = ldgi(a.row_ptr + i + 1);
  for (int h = 0; h < a.heads; ++h) {
    const long long hc = (long long)h * dh;
    const float* qr = a.q + (long long)i * a.ld_q + hc;
    const float* gr = a.dout + (long long)i * a.ld_dout + hc;
    const float delta = wave_sum64(sp_row_dot(gr, a.out + (long long)i * a.ld_out + hc, dh, lane));
    const long long ih = (long long)i * a.heads + h;
    if (lane == 0) a.delta[ih] = delta;
    const float m = a.lse[ih], ll = a.lse[a.planes + ih];
    for (int c = lane; c < dh; c += 64) acc[c] = 0.f;
    for (int t = e0; t < e1; ++t) {
      const int j = ldgi(a.col + t);
      const float* kr = a.k + (long long)j * a.ld_k + hc;
      float d = 0.f;
      for (int c = lane; c < dh; c += 64) d = fmaf(ldg1(qr + c) * a.scale, ldg1(kr + c), d);
      const float s = wave_sum64(d);
      const float dp = wave_sum64(sp_row_dot(gr, a.v + (long long)j * a.ld_v + hc, dh, lane));
      const float g = expf((s - m) - ll) * (dp - delta);
      for (int c = lane; c < dh; c += 64) acc[c] = fmaf(g, ldg1(kr + c), acc[c]);
    }
    for (int c = lane; c < dh; c += 64) stg1(a.dq + (long long)i * a.ld_dq + hc + c, acc[c] * a.scale);
  }
}

__global__ __launch_bounds__(64) void sp_bwd_col_gen_kernel(SpArgs a0) {
  __shared__ float acck[kSpMaxRow], accv[kSpMaxRow];
  const int lane = threadIdx.x, dh = a0.dh;
  const long long copy = blockIdx.x / a0.n_cols;
  const int j = (int)(blockIdx.x - copy * a0.n_cols);
  const SpArgs a = sp_copy(a0, copy);
  const int s0 = ldgi(a.col_ptr + j), s1 = ldgi(a.col_ptr + j + 1);
  for (int h = 0; h < a.heads; ++h) {
    const long long hc = (long long)h * dh;
    const float* kr = a.k + (long long)j * a.ld_k + hc;
    const float* vr = a.v + (long long)j * a.ld_v + hc;
    for (int c = lane; c < dh; c += 64) acck[c] = 0.f, accv[c] = 0.f;
    for (int t = s0; t < s1; ++t) {
      const int pos = ldgi(a.col_pos + t);
      const int i = ldgi(a.row + pos);
      const float* qr = a.q + (long long)i * a.ld_q + hc;
      const float* gr = a.dout + (long long)i * a.ld_dout + hc;
      const long long ih = (long long)i * a.heads + h;
      const float m = a.lse[ih], ll = a.lse[a.planes + ih], delta = a.delta[ih];
      float d = 0.f;
      for (int c = lane; c < dh; c += 64) d = fmaf(ldg1(qr + c) * a.scale, ldg1(kr + c), d);
      const float s = wave_sum64(d);
      const float dp = wave_sum64(sp_row_dot(gr, vr, dh, lane));
      const float p = expf((s - m) - ll);
      const float g = p * (dp - delta);
      for (int c = lane; c < dh; c += 64) {
        acck[c] = fmaf(g, ldg1(qr + c) * a.scale, acck[c]);
        accv[c] = fmaf(p, ldg1(gr + c), accv[c]);
      }
    }
    for (int c = lane; c < dh; c += 64) {
      stg1(a.dk + (long long)j * a.ld_dk + hc + c, acck[c]);
      stg1(a.dv + (long long)j * a.ld_dv + hc + c, accv[c]);
    }
  }
}

bool sp_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// register-path variants by row width: 0..3 = rows up to 256 / 512 / 1024 / 2048 floats; -1 = the general path
int sp_variant(int heads, int dh, bool vec) {
  const int D = heads * dh;
  if (!vec || 64 % heads != 0 || dh % 4 != 0 || D > kSpFastRow) return -1;
  return D <= 256 ? 0 : D <= 512 ? 1 : D <= 1024 ? 2 : 3;
}

#define GW_SP_VARIANTS(X, GEN) \
  switch (variant) {           \
    case 0: X(1, 4); break;    \
    case 1: X(2, 4); break;    \
    case 2: X(4, 2); break;    \
    case 3: X(8, 1); break;    \
    default: GEN; break;       \
  }

int sp_check(const char* bad, int32_t batch, int32_t n_rows, int32_t n_cols, int32_t n_edges, int32_t heads, int32_t dim_head,
             float scale) {
  if (n_rows < 0 || n_cols < 0 || n_edges < 0 || heads < 1 || dim_head < 1 || batch < 1 || !(scale == scale) || isinf(scale))
    return set_error(GW_E_BADARG, bad);
  if ((int64_t)heads * dim_head > kSpMaxRow) return set_error(GW_E_UNSUPPORTED, "sparse attention: heads * dim_head must be at most 4096");
  if ((int64_t)batch * n_rows * heads >= ((int64_t)1 << 31) || (int64_t)batch * n_cols * heads >= ((int64_t)1 << 31))
    return set_error(GW_E_BADARG, bad);
  return GW_OK;
}

}  // namespace

extern "C" {

int gw_sparse_attention_forward(int32_t batch, int32_t n_rows, int32_t n_cols, int32_t n_edges, int32_t heads, int32_t dim_head,
                                float scale, const int32_t* row_ptr, const int32_t* col, const float* q, int32_t ld_q, const float* k,
                                int32_t ld_k, const float* v, int32_t ld_v, float* out, int32_t ld_out, float* lse, void* stream) {
  const char* bad = "gw_sparse_attention_forward: bad arguments";
  if (int rc = sp_check(bad, batch, n_rows, n_cols, n_edges, heads, dim_head, scale)) return rc;
  if (n_rows == 0 || n_edges == 0) return GW_OK;
  const int D = heads * dim_head;
  if (!row_ptr || !col || !q || !k || !v || !out || !lse || n_cols < 1 || ld_q < D || ld_k < D || ld_v < D || ld_out < D)
    return set_error(GW_E_BADARG, bad);
  const bool vec = ld_q % 4 == 0 && ld_k % 4 == 0 && ld_v % 4 == 0 && ld_out % 4 == 0 && sp_aligned16(q) && sp_aligned16(k) &&
                   sp_aligned16(v) && sp_aligned16(out);
  SpArgs a = {};
  a.n_rows = n_rows, a.n_cols = n_cols, a.heads = heads, a.dh = dim_head, a.batch = batch, a.scale = scale;
  a.row_ptr = row_ptr, a.col = col;
  a.q = q, a.k = k, a.v = v, a.ld_q = ld_q, a.ld_k = ld_k, a.ld_v = ld_v;
  a.out = out, a.ld_out = ld_out, a.lse = lse, a.planes = (long long)batch * n_rows * heads;
  const int variant = sp_variant(heads, dim_head, vec);
  a.G = variant >= 0 ? 64 / heads : 0;
  const int64_t items = (int64_t)n_rows * batch;
  const unsigned grid = (unsigned)((items + 3) / 4);
#define GW_SP_FWD(NJ, U) hipLaunchKernelGGL((sp_fwd_kernel<NJ, U>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a)
  GW_SP_VARIANTS(GW_SP_FWD, hipLaunchKernelGGL(sp_fwd_gen_kernel, dim3((unsigned)items), dim3(64), 0, (hipStream_t)stream, a))
#undef GW_SP_FWD
  return check_launch("sp_fwd_kernel launch");
}

int gw_sparse_attention_backward(int32_t batch, int32_t n_rows, int32_t n_cols, int32_t n_edges, int32_t heads, int32_t dim_head,
                                 float scale, const int32_t* row_ptr, const int32_t* col, const int32_t* row, const int32_t* col_pos,
                                 const int32_t* col_ptr, const float* q, int32_t ld_q, const float* k, int32_t ld_k, const float* v,
                                 int32_t ld_v, const float* out, int32_t ld_out, const float* dout, int32_t ld_dout, const float* lse,
                                 float* delta, float* dq, int32_t ld_dq, float* dk, int32_t ld_dk, float* dv, int32_t ld_dv,
                                 void* stream) {
  const char* bad = "gw_sparse_attention_backward: bad arguments";
  if (int rc = sp_check(bad, batch, n_rows, n_cols, n_edges, heads, dim_head, scale)) return rc;
  if (n_edges == 0 || n_rows == 0 || n_cols == 0) return GW_OK;
  const int D = heads * dim_head;
  if (!row_ptr || !col || !row || !col_pos || !col_ptr || !q || !k || !v || !out || !dout || !lse || !delta || !dq || !dk || !dv ||
      ld_q < D || ld_k < D || ld_v < D || ld_out < D || ld_dout < D || ld_dq < D || ld_dk < D || ld_dv < D)
    return set_error(GW_E_BADARG, bad);
  const bool vec = ld_q % 4 == 0 && ld_k % 4 == 0 && ld_v % 4 == 0 && ld_out % 4 == 0 && ld_dout % 4 == 0 && ld_dq % 4 == 0 &&
                   ld_dk % 4 == 0 && ld_dv % 4 == 0 && sp_aligned16(q) && sp_aligned16(k) && sp_aligned16(v) && sp_aligned16(out) &&
                   sp_aligned16(dout) && sp_aligned16(dq) && sp_aligned16(dk) && sp_aligned16(dv);
  SpArgs a = {};
  a.n_rows = n_rows, a.n_cols = n_cols, a.heads = heads, a.dh = dim_head, a.batch = batch, a.scale = scale;
  a.row_ptr = row_ptr, a.col = col, a.row = row, a.col_pos = col_pos, a.col_ptr = col_ptr;
  a.q = q, a.k = k, a.v = v, a.ld_q = ld_q, a.ld_k = ld_k, a.ld_v = ld_v;
  a.out = const_cast<float*>(out), a.ld_out = ld_out, a.lse = const_cast<float*>(lse), a.planes = (long long)batch * n_rows * heads;
  a.dout = dout, a.ld_dout = ld_dout, a.delta = delta;
  a.dq = dq, a.dk = dk, a.dv = dv, a.ld_dq = ld_dq, a.ld_dk = ld_dk, a.ld_dv = ld_dv;
  const int variant = sp_variant(heads, dim_head, vec);
  a.G = variant >= 0 ? 64 / heads : 0;
  const int64_t items_r = (int64_t)n_rows * batch, items_c = (int64_t)n_cols * batch;
  const unsigned grid_r = (unsigned)((items_r + 3) / 4), grid_c = (unsigned)((items_c + 3) / 4);
#define GW_SP_BWD_ROW(NJ, U) \
  hipLaunchKernelGGL((sp_bwd_row_kernel<NJ, (U > 2 ? 2 : U)>), dim3(grid_r), dim3(256), 0, (hipStream_t)stream, a)
  GW_SP_VARIANTS(GW_SP_BWD_ROW, hipLaunchKernelGGL(sp_bwd_row_gen_kernel, dim3((unsigned)items_r), dim3(64), 0, (hipStream_t)stream, a))
#undef GW_SP_BWD_ROW
  if (int rc = check_launch("sp_bwd_row_kernel launch")) return rc;
#define GW_SP_BWD_COL(NJ, U) hipLaunchKernelGGL((sp_bwd_col_kernel<NJ>), dim3(grid_c), dim3(256), 0, (hipStream_t)stream, a)
  GW_SP_VARIANTS(GW_SP_BWD_COL, hipLaunchKernelGGL(sp_bwd_col_gen_kernel, dim3((unsigned)items_c), dim3(64), 0, (hipStream_t)stream, a))
#undef GW_SP_BWD_COL
  return check_launch("sp_bwd_col_kernel launch");
}

}  // extern "C"
