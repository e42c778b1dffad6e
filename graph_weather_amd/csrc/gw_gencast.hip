// gw_gencast.hip - the GenCast layers (graph_weather/models/gencast/layers): graph-transformer attention over the incoming edges
// of every node (the TransformerConv of the mesh processor) and the row operations around it.
//
//   attn_fwd_kernel      one wave per (destination, head) - per destination with the head-mean, the heads then in order - walks the
//                        destination's run of the destination-sorted edge list once: the q row stays in registers, the k, v (and e)
//                        rows of U edges are gathered into registers with 16-byte loads, the scores are wave sums, the softmax is
//                        online (running maximum, sum and output row in registers).  Nothing of size E x H x C or E x H is written;
//                        per (destination, head) the score maximum and log sum exp(s - max) go to two planes for the backward.
//   attn_bwd_dst_kernel  backward by recomputation, one wave per (destination, head): delta = rowsum(dout o out), then the same walk
//                        writes dq and - every edge belongs to one destination - de in the caller's edge order with plain stores.
//   attn_bwd_src_kernel  one wave per (source, head) walks the source-sorted list (GraphPlan.src_sorted) and writes dk and dv.
//   A row fragment is NE floats per lane: columns 4 lane + 256 j .. + 3 (VEC: dim_head and every stride a multiple of 4, 16-byte
//   loads) or lane + 64 j (scalar path, any dim_head and stride); columns past dim_head hold zeros, so dot products need no guard.
//   attn_*_long_kernel   rows too long for register fragments (a scalar dim_head above 512, any above 2048): one wave per workgroup,
//                        running rows in LDS, everything else streamed - coverage up to heads * dim_head = 4096.
//   A destination with many edges is one wave's serial walk: correct at any degree, fast only for near-uniform degrees.
//   Batch-shared form (gw_graph_attention_batched_*): `batch` disconnected copies of one graph share the plan; copy b's node rows
//   start at b n, the work item is (copy, destination, head) with the walk above, and the edge table moves by e_bstride rows per
//   copy (0: one table for all).  The gradient of a shared table is summed over the copies in copy order by the wave that owns
//   the destination (it owns the same edges in every copy): plain read-modify-write, no atomics.
//
//   cln_*_kernel         ConditionalLayerNorm: act(scale[g] o LN(x[r]) + bias[g]) (LN without affine, eps 1e-5), one wave per row;
//                        g = r / rows_per_group (1: a scale and bias row per row).  Grouped gradient of scale and bias: per-slab
//                        partials (256 rows of one group, one thread per column, rows in order) added in slab order
//   cln_fan_*_kernel     the fan-out form for an ensemble (B samples x N members): one wave per row of x [B M, W] forms the statistics
//                        once and writes the row's N conditioned outputs [B N M, W]; backward: dx summed over the members in member
//                        order by the owning wave, the gradients of scale and bias [B N, W] through the slab partials above
//   precond_*_kernel     the Denoiser's preconditioning (Karras et al. 2022) as row kernels: the encoder's grid input rows
//                        (c_in(sigma_b) Z | X | static grid features) with c_noise, and c_skip(sigma_b) Z + c_out(sigma_b) preds
//   gate_*_kernel        TransformerConv's beta gate: g = sigmoid(w_a.out + w_b.x_r + w_c.(out - x_r)), y = g x_r + (1 - g) out; the
//                        weight gradient is per-slab partials (256 rows, one thread per column, rows in order) added in slab order
//   silu_*, fourier_*    SiLU; cos / sin features of the noise level (accurate cosf / sinf) and their gradient
//
// fp32 data, no atomics, every sum in one fixed order: equal inputs give bitwise equal results.  No host synchronisation.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gw_amd.h"
#include "gw_device.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

int failf(int code, const char* msg) { return set_error(code, msg); }

constexpr int kMaxRow = 4096;   // heads * dim_head
constexpr int kGateSlab = 256;  // rows per partial of the gate's weight gradient

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

unsigned grid_for(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b < 16384 ? (b > 0 ? b : 1) : 16384);
}

// ---- row fragments -----------------------------------------------------------------------------------------------------------
template <int NE, bool VEC>
struct Frag {
  float r[NE];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int j = 0; j < NE; ++j) r[j] = 0.f;
  }
  __device__ __forceinline__ void load(const float* __restrict__ p, int C, int lane) {
    if constexpr (VEC) {
#pragma unroll
      for (int j = 0; j < NE / 4; ++j) {
        const int c = 4 * lane + 256 * j;
        const f32x4 v = c < C ? ldg4(p + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        r[4 * j] = v.x, r[4 * j + 1] = v.y, r[4 * j + 2] = v.z, r[4 * j + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        const int c = lane + 64 * j;
        r[j] = c < C ? ldg1(p + c) : 0.f;
      }
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ p, int C, int lane) const {
    if constexpr (VEC) {
#pragma unroll
      for (int j = 0; j < NE / 4; ++j) {
        const int c = 4 * lane + 256 * j;
        if (c < C) stg4(p + c, f32x4{r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]});
      }
    } else {
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        const int c = lane + 64 * j;
        if (c < C) stg1(p + c, r[j]);
      }
    }
  }
  __device__ __forceinline__ void add(const Frag& o) {
#pragma unroll
    for (int j = 0; j < NE; ++j) r[j] += o.r[j];
  }
  __device__ __forceinline__ void scale(float s) {
#pragma unroll
    for (int j = 0; j < NE; ++j) r[j] *= s;
  }
  __device__ __forceinline__ void divide(float s) {
#pragma unroll
    for (int j = 0; j < NE; ++j) r[j] /= s;
  }
  __device__ __forceinline__ void axpy(float s, const Frag& o) {
#pragma unroll
    for (int j = 0; j < NE; ++j) r[j] = fmaf(s, o.r[j], r[j]);
  }
  __device__ __forceinline__ float dot(const Frag& o) const {  // this lane's part; wave_sum makes the row's
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NE; ++j) s = fmaf(r[j], o.r[j], s);
    return s;
  }
};

struct AttnArgs {
  int n_dst, n_src, heads, C, mean;
  const int* dst_ptr;        // [n_dst + 1]
  const int* src;            // [E] source row of destination-sorted edge t
  const int* dst;            // [E] destination row of destination-sorted edge t (source pass)
  const long long* perm;     // [E] caller's edge id of destination-sorted edge t (NULL: t itself)
  const int* src_pos;        // [E] destination-sorted positions grouped by source row (source pass)
  const int* src_ptr;        // [n_src + 1]
  const float *q, *k, *v, *e;
  long long ld_q, ld_k, ld_v, ld_e;
  float* out;
  long long ld_out;
  float* out_heads;          // forward: per-head rows beside the head-mean (may be NULL); backward: the per-head output rows
  long long ld_oh;
  float* lse;                // [2][n_dst * heads]
  const float* dout;
  long long ld_dout;
  float* delta;              // [n_dst * heads]
  float *dq, *dk, *dv, *de;
  long long ld_dq, ld_dk, ld_dv, ld_de;
  float sqrt_c;
  int batch;                 // copies of the graph that share the plan
  int de_loop;               // destination pass: one wave walks its (destination, head) in every copy and sums de in copy order
  long long e_bstride;       // rows between the edge tables (e, de) of two copies; 0: one table
  long long planes;          // batch * n_dst * heads: the distance between the two planes of lse
};

// the arguments of copy b: node tables, planes and scratch move by whole copies, the edge tables by e_bstride rows
__device__ __forceinline__ AttnArgs attn_copy(AttnArgs a, long long b) {
  const long long rd = b * a.n_dst, rs = b * a.n_src, eb = b * a.e_bstride;
  a.q += rd * a.ld_q, a.k += rs * a.ld_k, a.v += rs * a.ld_v;
  if (a.e != nullptr) a.e += eb * a.ld_e;
  if (a.out != nullptr) a.out += rd * a.ld_out;
  if (a.out_heads != nullptr) a.out_heads += rd * a.ld_oh;
  a.lse += rd * a.heads;
  if (a.dout != nullptr) a.dout += rd * a.ld_dout;
  if (a.delta != nullptr) a.delta += rd * a.heads;
  if (a.dq != nullptr) a.dq += rd * a.ld_dq;
  if (a.dk != nullptr) a.dk += rs * a.ld_dk;
  if (a.dv != nullptr) a.dv += rs * a.ld_dv;
  if (a.de != nullptr) a.de += eb * a.ld_de;
  return a;
}

// the copy of a wave's item.  Every lane of a wave holds the same item, but it comes from threadIdx, so the compiler takes it for
// a per-lane value; read through the first lane the copy is a scalar and the table pointers attn_copy moves stay in SGPRs
__device__ __forceinline__ long long wave_uniform_copy(long long gitem, long long n_items) {
  return (long long)__builtin_amdgcn_readfirstlane((int)(gitem / n_items));
}

// grid ceil(batch items / 4), block 256: wave = one (copy, destination, head), or one (copy, destination) with its heads in order
// (head-mean)
template <int NE, bool VEC, int U>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs a0) {
  typedef Frag<NE, VEC> F;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long gitem = (long long)blockIdx.x * 4 + wave;
  const long long n_items = a0.mean ? (long long)a0.n_dst : (long long)a0.n_dst * a0.heads;
  if (gitem >= n_items * a0.batch) return;
  const long long copy = wave_uniform_copy(gitem, n_items), item = gitem - copy * n_items;
  const AttnArgs a = attn_copy(a0, copy);
  const int i = a.mean ? (int)item : (int)(item / a.heads);
  const int h0 = a.mean ? 0 : (int)(item % a.heads), hn = a.mean ? a.heads : 1;
  const int C = a.C;
  const int e0 = ldgi(a.dst_ptr + i), e1 = ldgi(a.dst_ptr + i + 1);
  const long long planes = a.planes;
  F macc;
  macc.zero();
  for (int hh = 0; hh < hn; ++hh) {
    const int h = h0 + hh;
    const long long hc = (long long)h * C;
    F qf, acc;
    qf.load(a.q + (long long)i * a.ld_q + hc, C, lane);
    acc.zero();
    float m = -INFINITY, l = 0.f;
    for (int t = e0; t < e1; t += U) {
      float s[U];
      F vf[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int tt = t + u < e1 ? t + u : e1 - 1;  // past the run: the last edge again, with a score of -inf
        const int j = ldgi(a.src + tt);
        F kf;
        kf.load(a.k + (long long)j * a.ld_k + hc, C, lane);
        vf[u].load(a.v + (long long)j * a.ld_v + hc, C, lane);
        if (a.e != nullptr) {
          const long long eid = a.perm != nullptr ? a.perm[tt] : (long long)tt;
          F ef;
          ef.load(a.e + eid * a.ld_e + hc, C, lane);
          kf.add(ef);
          vf[u].add(ef);
        }
        const float d = wave_sum(qf.dot(kf)) / a.sqrt_c;
        s[u] = t + u < e1 ? d : -INFINITY;
      }
      float mn = m;
#pragma unroll
      for (int u = 0; u < U; ++u) mn = fmaxf(mn, s[u]);
      const float sc = expf(m - mn);  // 0 at the first step (m = -inf, mn finite: s[0] is a real edge)
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
    const bool any = e1 > e0;  // a destination without edges: output 0 (and 0 in both planes, which nothing reads)
    if (any) acc.divide(l);
    if (lane == 0) {
      a.lse[(long long)i * a.heads + h] = any ? m : 0.f;
      a.lse[planes + (long long)i * a.heads + h] = any ? logf(l) : 0.f;
    }
    if (a.mean) {
      macc.add(acc);
      if (a.out_heads != nullptr) acc.store(a.out_heads + (long long)i * a.ld_oh + hc, C, lane);
    } else {
      acc.store(a.out + (long long)i * a.ld_out + hc, C, lane);
    }
  }
  if (a.mean) {
    macc.divide((float)a.heads);
    macc.store(a.out + (long long)i * a.ld_out, C, lane);
  }
}

// one (destination, head) of one copy; de_add: de already holds the sum over the earlier copies
template <int NE, bool VEC>
__device__ __forceinline__ void attn_bwd_dst_item(const AttnArgs& a, long long item, int lane, bool de_add) {
  typedef Frag<NE, VEC> F;
  const int i = (int)(item / a.heads), h = (int)(item % a.heads), C = a.C;
  const long long hc = (long long)h * C;
  const int e0 = ldgi(a.dst_ptr + i), e1 = ldgi(a.dst_ptr + i + 1);
  F qf, dof, dqf;
  qf.load(a.q + (long long)i * a.ld_q + hc, C, lane);
  dof.load(a.dout + (long long)i * a.ld_dout + (a.mean ? 0 : hc), C, lane);
  if (a.mean) dof.divide((float)a.heads);
  float delta;
  {
    F of;
    of.load(a.out_heads + (long long)i * a.ld_oh + hc, C, lane);
    delta = wave_sum(dof.dot(of));
  }
  if (lane == 0) a.delta[item] = delta;
  const float m = a.lse[item], ll = a.lse[a.planes + item];
  dqf.zero();
  for (int t = e0; t < e1; ++t) {
    const int j = ldgi(a.src + t);
    const long long eid = a.perm != nullptr ? a.perm[t] : (long long)t;
    const float* er = a.e != nullptr ? a.e + eid * a.ld_e + hc : nullptr;
    F kf;
    kf.load(a.k + (long long)j * a.ld_k + hc, C, lane);
    if (er != nullptr) {
      F ef;
      ef.load(er, C, lane);
      kf.add(ef);
    }
    const float s = wave_sum(qf.dot(kf)) / a.sqrt_c;
    float dp;
    {  // (the widest fragments read e a second time instead of keeping it: registers)
      F vf;
      vf.load(a.v + (long long)j * a.ld_v + hc, C, lane);
      if (er != nullptr) {
        F ef;
        ef.load(er, C, lane);
        vf.add(ef);
      }
      dp = wave_sum(dof.dot(vf));
    }
    const float p = expf((s - m) - ll);
    const float g = p * (dp - delta) / a.sqrt_c;
    dqf.axpy(g, kf);
    if (a.de != nullptr) {  // d(k + e) + d(v + e) of this edge and head
      F def;
      def.zero();
      def.axpy(g, qf);
      def.axpy(p, dof);
      if (de_add) {
        F old;
        old.load(a.de + eid * a.ld_de + hc, C, lane);
        def.add(old);
      }
      def.store(a.de + eid * a.ld_de + hc, C, lane);
    }
  }
  dqf.store(a.dq + (long long)i * a.ld_dq + hc, C, lane);
}

// grid ceil(batch n_dst heads / 4), block 256: wave = one (copy, destination, head).  LOOP (a de table shared by the copies): grid
// ceil(n_dst heads / 4), the wave takes its (destination, head) through the copies in order and sums de by read-modify-write
template <int NE, bool VEC, bool LOOP>
__global__ __launch_bounds__(256) void attn_bwd_dst_kernel(AttnArgs a0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long gitem = (long long)blockIdx.x * 4 + wave;
  const long long n_items = (long long)a0.n_dst * a0.heads;
  if constexpr (LOOP) {
    if (gitem >= n_items) return;
    for (int b = 0; b < a0.batch; ++b) {
      const AttnArgs a = attn_copy(a0, b);
      attn_bwd_dst_item<NE, VEC>(a, gitem, lane, b > 0);
    }
  } else {
    if (gitem >= n_items * a0.batch) return;
    const long long copy = wave_uniform_copy(gitem, n_items);
    const AttnArgs a = attn_copy(a0, copy);
    attn_bwd_dst_item<NE, VEC>(a, gitem - copy * n_items, lane, false);
  }
}

// grid ceil(batch n_src heads / 4), block 256; reads delta of attn_bwd_dst_kernel
template <int NE, bool VEC>
__global__ __launch_bounds__(256) void attn_bwd_src_kernel(AttnArgs a0) {
  typedef Frag<NE, VEC> F;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long gitem = (long long)blockIdx.x * 4 + wave;
  const long long n_items = (long long)a0.n_src * a0.heads;
  if (gitem >= n_items * a0.batch) return;
  const long long copy = wave_uniform_copy(gitem, n_items), item = gitem - copy * n_items;
  const AttnArgs a = attn_copy(a0, copy);
  const int j = (int)(item / a.heads), h = (int)(item % a.heads), C = a.C;
  const long long hc = (long long)h * C, planes = a.planes;
  const int s0 = ldgi(a.src_ptr + j), s1 = ldgi(a.src_ptr + j + 1);
  F kf, vf, dkf, dvf;
  kf.load(a.k + (long long)j * a.ld_k + hc, C, lane);
  vf.load(a.v + (long long)j * a.ld_v + hc, C, lane);
  dkf.zero();
  dvf.zero();
  for (int t = s0; t < s1; ++t) {
    const int pos = ldgi(a.src_pos + t);
    const int i = ldgi(a.dst + pos);
    F ke = kf, ve = vf, qf, dof;
    if (a.e != nullptr) {
      const long long eid = a.perm != nullptr ? a.perm[pos] : (long long)pos;
      F ef;
      ef.load(a.e + eid * a.ld_e + hc, C, lane);
      ke.add(ef);
      ve.add(ef);
    }
    qf.load(a.q + (long long)i * a.ld_q + hc, C, lane);
    dof.load(a.dout + (long long)i * a.ld_dout + (a.mean ? 0 : hc), C, lane);
    if (a.mean) dof.divide((float)a.heads);
    const long long ih = (long long)i * a.heads + h;
    const float m = a.lse[ih], ll = a.lse[planes + ih], delta = a.delta[ih];
    const float s = wave_sum(qf.dot(ke)) / a.sqrt_c;
    const float dp = wave_sum(dof.dot(ve));
    const float p = expf((s - m) - ll);
    dkf.axpy(p * (dp - delta) / a.sqrt_c, qf);
    dvf.axpy(p, dof);
  }
  dkf.store(a.dk + (long long)j * a.ld_dk + hc, C, lane);
  dvf.store(a.dv + (long long)j * a.ld_dv + hc, C, lane);
}

// ---- rows too long for register fragments (a scalar dim_head above 512, any dim_head above 2048) ------------------------------
// The same three walks with one wave per workgroup: the rows are streamed (lane l owns columns l, l + 64, ...), the running rows
// live in LDS (each lane reads and writes its own columns only: no barrier).  Coverage, not speed.
__device__ __forceinline__ float row_dot(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ e, int C,
                                         int lane) {  // sum_c x[c] (y[c] + e[c]) over this lane's columns
  float d = 0.f;
  for (int c = lane; c < C; c += 64) d = fmaf(ldg1(x + c), ldg1(y + c) + (e != nullptr ? ldg1(e + c) : 0.f), d);
  return d;
}

__global__ __launch_bounds__(64) void attn_fwd_long_kernel(AttnArgs a0) {
  __shared__ float acc[kMaxRow], macc[kMaxRow];
  const int lane = threadIdx.x, C = a0.C;
  const long long n_items = a0.mean ? (long long)a0.n_dst : (long long)a0.n_dst * a0.heads;
  const long long copy = blockIdx.x / n_items, item = blockIdx.x - copy * n_items;
  const AttnArgs a = attn_copy(a0, copy);
  const int i = a.mean ? (int)item : (int)(item / a.heads);
  const int h0 = a.mean ? 0 : (int)(item % a.heads), hn = a.mean ? a.heads : 1;
  const int e0 = ldgi(a.dst_ptr + i), e1 = ldgi(a.dst_ptr + i + 1);
  const long long planes = a.planes;
  for (int c = lane; c < C; c += 64) macc[c] = 0.f;
  for (int hh = 0; hh < hn; ++hh) {
    const int h = h0 + hh;
    const long long hc = (long long)h * C;
    const float* qr = a.q + (long long)i * a.ld_q + hc;
    for (int c = lane; c < C; c += 64) acc[c] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int t = e0; t < e1; ++t) {
      const int j = ldgi(a.src + t);
      const float* er = a.e != nullptr ? a.e + (a.perm != nullptr ? a.perm[t] : (long long)t) * a.ld_e + hc : nullptr;
      const float* vr = a.v + (long long)j * a.ld_v + hc;
      const float s = wave_sum(row_dot(qr, a.k + (long long)j * a.ld_k + hc, er, C, lane)) / a.sqrt_c;
      const float mn = fmaxf(m, s), sc = expf(m - mn), p = expf(s - mn);
      l = l * sc + p;
      for (int c = lane; c < C; c += 64) acc[c] = fmaf(p, ldg1(vr + c) + (er != nullptr ? ldg1(er + c) : 0.f), acc[c] * sc);
      m = mn;
    }
    const bool any = e1 > e0;
    if (lane == 0) {
      a.lse[(long long)i * a.heads + h] = any ? m : 0.f;
      a.lse[planes + (long long)i * a.heads + h] = any ? logf(l) : 0.f;
    }
    for (int c = lane; c < C; c += 64) {
      const float o = any ? acc[c] / l : 0.f;
      if (a.mean) {
        macc[c] += o;
        if (a.out_heads != nullptr) stg1(a.out_heads + (long long)i * a.ld_oh + hc + c, o);
      } else {
        stg1(a.out + (long long)i * a.ld_out + hc + c, o);
      }
    }
  }
  if (a.mean)
    for (int c = lane; c < C; c += 64) stg1(a.out + (long long)i * a.ld_out + c, macc[c] / (float)a.heads);
}

__device__ __forceinline__ void attn_bwd_dst_long_item(const AttnArgs& a, long long item, int lane, bool de_add, float* acc) {
  const int C = a.C;
  const int i = (int)(item / a.heads), h = (int)(item % a.heads);
  const long long hc = (long long)h * C;
  const int e0 = ldgi(a.dst_ptr + i), e1 = ldgi(a.dst_ptr + i + 1);
  const float* qr = a.q + (long long)i * a.ld_q + hc;
  const float* gr = a.dout + (long long)i * a.ld_dout + (a.mean ? 0 : hc);
  const float hdiv = a.mean ? (float)a.heads : 1.f;  // (x / 1 is x)
  float d = 0.f;
  for (int c = lane; c < C; c += 64) d = fmaf(ldg1(gr + c) / hdiv, ldg1(a.out_heads + (long long)i * a.ld_oh + hc + c), d);
  const float delta = wave_sum(d);
  if (lane == 0) a.delta[item] = delta;
  const float m = a.lse[item], ll = a.lse[a.planes + item];
  for (int c = lane; c < C; c += 64) acc[c] = 0.f;
  for (int t = e0; t < e1; ++t) {
    const int j = ldgi(a.src + t);
    const long long eid = a.perm != nullptr ? a.perm[t] : (long long)t;
    const float* er = a.e != nullptr ? a.e + eid * a.ld_e + hc : nullptr;
    const float* kr = a.k + (long long)j * a.ld_k + hc;
    const float s = wave_sum(row_dot(qr, kr, er, C, lane)) / a.sqrt_c;
    const float dp = wave_sum(row_dot(gr, a.v + (long long)j * a.ld_v + hc, er, C, lane)) / hdiv;
    const float p = expf((s - m) - ll);
    const float g = p * (dp - delta) / a.sqrt_c;
    for (int c = lane; c < C; c += 64) {
      acc[c] = fmaf(g, ldg1(kr + c) + (er != nullptr ? ldg1(er + c) : 0.f), acc[c]);
      if (a.de != nullptr) {
        float* dp_ = a.de + eid * a.ld_de + hc + c;
        const float dv_ = fmaf(p, ldg1(gr + c) / hdiv, g * ldg1(qr + c));
        stg1(dp_, de_add ? dv_ + ldg1(dp_) : dv_);
      }
    }
  }
  for (int c = lane; c < C; c += 64) stg1(a.dq + (long long)i * a.ld_dq + hc + c, acc[c]);
}

template <bool LOOP>
__global__ __launch_bounds__(64) void attn_bwd_dst_long_kernel(AttnArgs a0) {
  __shared__ float acc[kMaxRow];
  const int lane = threadIdx.x;
  const long long n_items = (long long)a0.n_dst * a0.heads;
  if constexpr (LOOP) {
    for (int b = 0; b < a0.batch; ++b) {
      const AttnArgs a = attn_copy(a0, b);
      attn_bwd_dst_long_item(a, blockIdx.x, lane, b > 0, acc);
    }
  } else {
    const long long copy = blockIdx.x / n_items;
    const AttnArgs a = attn_copy(a0, copy);
    attn_bwd_dst_long_item(a, blockIdx.x - copy * n_items, lane, false, acc);
  }
}

__global__ __launch_bounds__(64) void attn_bwd_src_long_kernel(AttnArgs a0) {
  __shared__ float acck[kMaxRow], accv[kMaxRow];
  const int lane = threadIdx.x, C = a0.C;
  const long long n_items = (long long)a0.n_src * a0.heads;
  const long long copy = blockIdx.x / n_items, item = blockIdx.x - copy * n_items;
  const AttnArgs a = attn_copy(a0, copy);
  const int j = (int)(item / a.heads), h = (int)(item % a.heads);
  const long long hc = (long long)h * C, planes = a.planes;
  const int s0 = ldgi(a.src_ptr + j), s1 = ldgi(a.src_ptr + j + 1);
  const float* kr = a.k + (long long)j * a.ld_k + hc;
  const float* vr = a.v + (long long)j * a.ld_v + hc;
  const float hdiv = a.mean ? (float)a.heads : 1.f;
  for (int c = lane; c < C; c += 64) acck[c] = 0.f, accv[c] = 0.f;
  for (int t = s0; t < s1; ++t) {
    const int pos = ldgi(a.src_pos + t);
    const int i = ldgi(a.dst + pos);
    const float* er = a.e != nullptr ? a.e + (a.perm != nullptr ? a.perm[pos] : (long long)pos) * a.ld_e + hc : nullptr;
    const float* qr = a.q + (long long)i * a.ld_q + hc;
    const float* gr = a.dout + (long long)i * a.ld_dout + (a.mean ? 0 : hc);
    const long long ih = (long long)i * a.heads + h;
    const float m = a.lse[ih], ll = a.lse[planes + ih], delta = a.delta[ih];
    const float s = wave_sum(row_dot(qr, kr, er, C, lane)) / a.sqrt_c;
    const float dp = wave_sum(row_dot(gr, vr, er, C, lane)) / hdiv;
    const float p = expf((s - m) - ll);
    const float g = p * (dp - delta) / a.sqrt_c;
    for (int c = lane; c < C; c += 64) {
      acck[c] = fmaf(g, ldg1(qr + c), acck[c]);
      accv[c] = fmaf(p, ldg1(gr + c) / hdiv, accv[c]);
    }
  }
  for (int c = lane; c < C; c += 64) {
    stg1(a.dk + (long long)j * a.ld_dk + hc + c, acck[c]);
    stg1(a.dv + (long long)j * a.ld_dv + hc + c, accv[c]);
  }
}

// fragment variants: 0..3 VEC with dim_head <= 256 / 512 / 1024 / 2048, 4..5 scalar with dim_head <= 128 / 512, 6 the long-row kernels
int attn_variant(int C, bool vec) {
  if (vec && C <= 2048) return C <= 256 ? 0 : C <= 512 ? 1 : C <= 1024 ? 2 : 3;
  return C <= 128 ? 4 : C <= 512 ? 5 : 6;
}

#define GW_GC_VARIANTS(X, LONG) \
  switch (variant) {            \
    case 0: X(4, true, 4); break;    \
    case 1: X(8, true, 4); break;    \
    case 2: X(16, true, 2); break;   \
    case 3: X(32, true, 1); break;   \
    case 4: X(2, false, 4); break;   \
    case 5: X(8, false, 2); break;   \
    default: LONG; break;            \
  }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- activations ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float act_f(float z, int act) {
  if (act == GW_ACT_RELU) return z > 0.f ? z : 0.f;
  if (act == GW_ACT_SILU) return z * sigmoidf_(z);
  return z;
}
__device__ __forceinline__ float act_d(float z, int act) {
  if (act == GW_ACT_RELU) return z > 0.f ? 1.f : 0.f;
  if (act == GW_ACT_SILU) {
    const float sg = sigmoidf_(z);
    return sg * (1.f + z * (1.f - sg));
  }
  return 1.f;
}

// ---- ConditionalLayerNorm: one wave per row, four rows per workgroup ------------------------------------------------------------
__device__ __forceinline__ void row_stats(const float* __restrict__ xr, int width, int lane, float& mean, float& rstd) {
  float s = 0.f;
  for (int c = lane; c < width; c += 64) s += ldg1(xr + c);
  mean = wave_sum(s) / (float)width;
  float v = 0.f;
  for (int c = lane; c < width; c += 64) {
    const float d = ldg1(xr + c) - mean;
    v = fmaf(d, d, v);
  }
  rstd = 1.0f / sqrtf(wave_sum(v) / (float)width + 1e-5f);
}

__global__ __launch_bounds__(256) void cln_fwd_kernel(long long rows, int width, int act, const float* __restrict__ x, long long ld_x,
                                                      const float* __restrict__ scale, long long ld_s, const float* __restrict__ bias,
                                                      long long ld_b, float* __restrict__ out, long long ld_o, long long rpg) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const long long g = rpg == 1 ? r : r / rpg;  // the row of scale and bias
  const float* xr = x + r * ld_x;
  float mean, rstd;
  row_stats(xr, width, lane, mean, rstd);
  for (int c = lane; c < width; c += 64) {
    const float xh = (ldg1(xr + c) - mean) * rstd;
    stg1(out + r * ld_o + c, act_f(ldg1(scale + g * ld_s + c) * xh + ldg1(bias + g * ld_b + c), act));
  }
}

__global__ __launch_bounds__(256) void cln_bwd_kernel(long long rows, int width, int act, const float* __restrict__ x, long long ld_x,
                                                      const float* __restrict__ scale, long long ld_s, const float* __restrict__ bias,
                                                      long long ld_b, const float* __restrict__ dout, long long ld_do,
                                                      float* __restrict__ dx, long long ld_dx, float* __restrict__ dscale,
                                                      float* __restrict__ dbias, long long ld_dsb, long long rpg,
                                                      float* __restrict__ stats) {
  // rpg > 1 (grouped): dscale and dbias are NULL here - cln_cols_kernel forms them from stats [rows][2] = (mean, rstd)
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const long long gr = rpg == 1 ? r : r / rpg;
  const float* xr = x + r * ld_x;
  float mean, rstd;
  row_stats(xr, width, lane, mean, rstd);
  if (stats != nullptr && lane == 0) stats[2 * r] = mean, stats[2 * r + 1] = rstd;
  float sa = 0.f, sb = 0.f;
  for (int c = lane; c < width; c += 64) {
    const float xh = (ldg1(xr + c) - mean) * rstd, sc = ldg1(scale + gr * ld_s + c);
    const float dz = ldg1(dout + r * ld_do + c) * act_d(sc * xh + ldg1(bias + gr * ld_b + c), act);
    if (dscale != nullptr) stg1(dscale + r * ld_dsb + c, dz * xh);
    if (dbias != nullptr) stg1(dbias + r * ld_dsb + c, dz);
    const float g = dz * sc;
    sa += g;
    sb = fmaf(g, xh, sb);
  }
  if (dx == nullptr) return;
  sa = wave_sum(sa) / (float)width;
  sb = wave_sum(sb) / (float)width;
  for (int c = lane; c < width; c += 64) {
    const float xh = (ldg1(xr + c) - mean) * rstd, sc = ldg1(scale + gr * ld_s + c);
    const float g = ldg1(dout + r * ld_do + c) * act_d(sc * xh + ldg1(bias + gr * ld_b + c), act) * sc;
    stg1(dx + r * ld_dx + c, rstd * (g - sa - xh * sb));
  }
}

// part[group][slab][2][width]: one thread per column walks the rows of one slab of one group in order.  fan > 0 (fan-out form):
// rows counts the rows of dout, group g = (sample, member) = (g / fan, g % fan) reads the x rows and statistics of its sample.
__global__ __launch_bounds__(256) void cln_cols_kernel(long long rows, int width, int act, long long rpg, const float* __restrict__ x,
                                                       long long ld_x, const float* __restrict__ scale, long long ld_s,
                                                       const float* __restrict__ bias, long long ld_b, const float* __restrict__ dout,
                                                       long long ld_do, const float* __restrict__ stats, float* __restrict__ part,
                                                       long long fan) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= width) return;
  const long long g = blockIdx.z, g0 = g * rpg, g1 = g0 + rpg < rows ? g0 + rpg : rows;
  const long long r0 = g0 + (long long)blockIdx.y * kGateSlab, r1 = r0 + kGateSlab < g1 ? r0 + kGateSlab : g1;
  const float sc = ldg1(scale + g * ld_s + c), bi = ldg1(bias + g * ld_b + c);
  double a = 0.0, b = 0.0;  // (fp64 for the reason given at gate_cols_kernel)
  const long long x_shift = fan > 0 ? g0 - (g / fan) * rpg : 0;  // dout row r pairs with x row r - x_shift
  for (long long r = r0; r < r1; ++r) {
    const long long rx = r - x_shift;
    const float xh = (ldg1(x + rx * ld_x + c) - stats[2 * rx]) * stats[2 * rx + 1];
    const float dz = ldg1(dout + r * ld_do + c) * act_d(sc * xh + bi, act);
    a += (double)(dz * xh);
    b += (double)dz;
  }
  float* p = part + (g * gridDim.y + blockIdx.y) * 2 * width;
  p[c] = (float)a;
  p[width + c] = (float)b;
}

// dscale[g], dbias[g] = the group's slab partials added in slab order
__global__ __launch_bounds__(256) void cln_sum_kernel(int slabs, int width, const float* __restrict__ part, float* __restrict__ dscale,
                                                      float* __restrict__ dbias, long long ld_dsb) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= width) return;
  const long long g = blockIdx.y;
  double a = 0.0, b = 0.0;
  for (int sl = 0; sl < slabs; ++sl) {
    const float* p = part + (g * slabs + sl) * 2 * width;
    a += (double)ldg1(p + c);
    b += (double)ldg1(p + width + c);
  }
  if (dscale != nullptr) dscale[g * ld_dsb + c] = (float)a;
  if (dbias != nullptr) dbias[g * ld_dsb + c] = (float)b;
}

bool cln_grouped_ok(int64_t rows, int32_t width, int64_t rpg) {
  if (rows < 0 || rows >= ((int64_t)1 << 33) || width < 1 || rpg < 1) return false;
  const int64_t groups = (rows + rpg - 1) / rpg, slabs = (rpg + kGateSlab - 1) / kGateSlab;
  return groups <= 65535 && slabs <= 65535;
}
size_t cln_grouped_bytes(int64_t rows, int32_t width, int64_t rpg) {
  const int64_t groups = (rows + rpg - 1) / rpg, slabs = (rpg + kGateSlab - 1) / kGateSlab;
  return ((size_t)rows * 2 + (size_t)groups * (size_t)slabs * 2 * (size_t)width) * sizeof(float);
}

// ---- fan-out ConditionalLayerNorm: x [B M, W] -> out [B N M, W], out row (b, n, m) = act(scale[b N + n] o LN(x[b M + m]) + bias[b N + n]) --
// One wave per x row: the statistics are formed once, then the wave writes the row's N outputs (lane l owns columns l + 64 j as in
// cln_fwd_kernel, so every output is bitwise what the grouped kernel gives on x repeated per member).
__global__ __launch_bounds__(256) void cln_fan_fwd_kernel(long long x_rows, int width, int act, long long rps, int members,
                                                          const float* __restrict__ x, long long ld_x, const float* __restrict__ scale,
                                                          long long ld_s, const float* __restrict__ bias, long long ld_b,
                                                          float* __restrict__ out, long long ld_o) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= x_rows) return;
  const long long b = r / rps, m = r - b * rps;
  const float* xr = x + r * ld_x;
  float mean, rstd;
  row_stats(xr, width, lane, mean, rstd);
  for (int c = lane; c < width; c += 64) {
    const float xh = (ldg1(xr + c) - mean) * rstd;
    for (int n = 0; n < members; ++n) {
      const long long g = b * members + n;
      stg1(out + (g * rps + m) * ld_o + c, act_f(ldg1(scale + g * ld_s + c) * xh + ldg1(bias + g * ld_b + c), act));
    }
  }
}

// Backward of the fan-out: dx[b M + m] = sum over the members, in member order, of what cln_bwd_kernel gives for output row
// (b, n, m); the owning wave forms the two row sums of every member (lane n % 64 keeps member n's pair, 64 members per pass) and
// then walks its columns once per pass - plain stores, a later pass adds to what the same lane stored.  stats [x_rows][2].
__global__ __launch_bounds__(256) void cln_fan_bwd_kernel(long long x_rows, int width, int act, long long rps, int members,
                                                          const float* __restrict__ x, long long ld_x, const float* __restrict__ scale,
                                                          long long ld_s, const float* __restrict__ bias, long long ld_b,
                                                          const float* __restrict__ dout, long long ld_do, float* dx, long long ld_dx,
                                                          float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= x_rows) return;
  const long long b = r / rps, m = r - b * rps;
  const float* xr = x + r * ld_x;
  float mean, rstd;
  row_stats(xr, width, lane, mean, rstd);
  if (lane == 0) stats[2 * r] = mean, stats[2 * r + 1] = rstd;
  if (dx == nullptr) return;
  for (int n0 = 0; n0 < members; n0 += 64) {
    const int n1 = n0 + 64 < members ? n0 + 64 : members;
    float my_sa = 0.f, my_sb = 0.f;
    for (int n = n0; n < n1; ++n) {
      const long long g = b * members + n;
      const float* dr = dout + (g * rps + m) * ld_do;
      float sa = 0.f, sb = 0.f;
      for (int c = lane; c < width; c += 64) {
        const float xh = (ldg1(xr + c) - mean) * rstd, sc = ldg1(scale + g * ld_s + c);
        const float gg = ldg1(dr + c) * act_d(sc * xh + ldg1(bias + g * ld_b + c), act) * sc;
        sa += gg;
        sb = fmaf(gg, xh, sb);
      }
      sa = wave_sum(sa) / (float)width;
      sb = wave_sum(sb) / (float)width;
      if (lane == n - n0) my_sa = sa, my_sb = sb;
    }
    for (int c0 = 0; c0 < width; c0 += 64) {  // (a loop every lane runs: the shuffles below need the whole wave)
      const int c = c0 + lane;
      const bool on = c < width;
      const float xh = on ? (ldg1(xr + c) - mean) * rstd : 0.f;
      float acc = (on && n0 > 0) ? dx[r * ld_dx + c] : 0.f;
      for (int n = n0; n < n1; ++n) {
        const long long g = b * members + n;
        const float sa = __shfl(my_sa, n - n0), sb = __shfl(my_sb, n - n0);
        if (on) {
          const float sc = ldg1(scale + g * ld_s + c);
          const float gg = ldg1(dout + (g * rps + m) * ld_do + c) * act_d(sc * xh + ldg1(bias + g * ld_b + c), act) * sc;
          acc += rstd * (gg - sa - xh * sb);
        }
      }
      if (on) dx[r * ld_dx + c] = acc;
    }
  }
}

bool cln_fanout_ok(int64_t x_rows, int32_t width, int64_t rps, int32_t members) {
  if (x_rows < 0 || width < 1 || rps < 1 || members < 1 || x_rows % rps != 0) return false;
  if (x_rows >= ((int64_t)1 << 33) || x_rows * members >= ((int64_t)1 << 33)) return false;
  return x_rows / rps * members <= 65535 && (rps + kGateSlab - 1) / kGateSlab <= 65535;
}
size_t cln_fanout_bytes(int64_t x_rows, int32_t width, int64_t rps, int32_t members) {
  const int64_t groups = x_rows / rps * members, slabs = (rps + kGateSlab - 1) / kGateSlab;
  return ((size_t)x_rows * 2 + (size_t)groups * (size_t)slabs * 2 * (size_t)width) * sizeof(float);
}

// ---- the Denoiser's preconditioning (utils/noise.py, denoiser.py): one wave per grid row, sample b = row / grid_rows --------------
// The coefficients in float32 in the reference's order of operations (the intrinsics keep the compiler from fusing a * b + c):
//   c_in = 1 / sqrt(s^2 + d^2), c_skip = d^2 / (s^2 + d^2), c_out = s d / sqrt(s^2 + d^2), c_noise = 1/4 log(s); d = sigma_data
__device__ __forceinline__ float precond_var(float s, float d2) { return __fadd_rn(__fmul_rn(s, s), d2); }
__device__ __forceinline__ float precond_c_in(float s, float d2) { return __fdiv_rn(1.0f, __fsqrt_rn(precond_var(s, d2))); }
__device__ __forceinline__ float precond_c_skip(float s, float d2) { return __fdiv_rn(d2, precond_var(s, d2)); }
__device__ __forceinline__ float precond_c_out(float s, float d, float d2) {
  return __fdiv_rn(__fmul_rn(s, d), __fsqrt_rn(precond_var(s, d2)));
}

// out[r] = (c_in(sigma_b) z[r] | x[r] | stat[r mod grid_rows]); c_noise[b] from the wave of the sample's first row
__global__ __launch_bounds__(256) void precond_in_fwd_kernel(long long rows, long long grid_rows, int wz, int wx, int ws, float d2,
                                                             const float* __restrict__ sigma, const float* __restrict__ z, long long ld_z,
                                                             const float* __restrict__ x, long long ld_x,
                                                             const float* __restrict__ stat, long long ld_s, float* __restrict__ out,
                                                             long long ld_o, float* __restrict__ c_noise) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const long long b = r / grid_rows, g = r - b * grid_rows;
  const float s = sigma[b], cin = precond_c_in(s, d2);
  float* o = out + r * ld_o;
  for (int c = lane; c < wz; c += 64) stg1(o + c, __fmul_rn(cin, ldg1(z + r * ld_z + c)));
  for (int c = lane; c < wx; c += 64) stg1(o + wz + c, ldg1(x + r * ld_x + c));
  for (int c = lane; c < ws; c += 64) stg1(o + wz + wx + c, ldg1(stat + g * ld_s + c));
  if (g == 0 && lane == 0 && c_noise != nullptr) c_noise[b] = __fmul_rn(0.25f, logf(s));
}

// dz[r] = c_in(sigma_b) dout[r, :wz], dx[r] = dout[r, wz : wz + wx] (each may be NULL)
__global__ __launch_bounds__(256) void precond_in_bwd_kernel(long long rows, long long grid_rows, int wz, int wx, float d2,
                                                             const float* __restrict__ sigma, const float* __restrict__ dout,
                                                             long long ld_do, float* __restrict__ dz, long long ld_dz,
                                                             float* __restrict__ dx, long long ld_dx) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float cin = precond_c_in(sigma[r / grid_rows], d2);
  const float* g = dout + r * ld_do;
  if (dz != nullptr)
    for (int c = lane; c < wz; c += 64) stg1(dz + r * ld_dz + c, __fmul_rn(cin, ldg1(g + c)));
  if (dx != nullptr)
    for (int c = lane; c < wx; c += 64) stg1(dx + r * ld_dx + c, ldg1(g + wz + c));
}

// out[r] = c_skip(sigma_b) z[r] + c_out(sigma_b) p[r]
__global__ __launch_bounds__(256) void precond_out_fwd_kernel(long long rows, long long grid_rows, int width, float d, float d2,
                                                              const float* __restrict__ sigma, const float* __restrict__ z, long long ld_z,
                                                              const float* __restrict__ p, long long ld_p, float* __restrict__ out,
                                                              long long ld_o) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float s = sigma[r / grid_rows], cs = precond_c_skip(s, d2), co = precond_c_out(s, d, d2);
  for (int c = lane; c < width; c += 64)
    stg1(out + r * ld_o + c, __fadd_rn(__fmul_rn(cs, ldg1(z + r * ld_z + c)), __fmul_rn(co, ldg1(p + r * ld_p + c))));
}

// dz[r] = c_skip(sigma_b) dout[r], dp[r] = c_out(sigma_b) dout[r] (each may be NULL)
__global__ __launch_bounds__(256) void precond_out_bwd_kernel(long long rows, long long grid_rows, int width, float d, float d2,
                                                              const float* __restrict__ sigma, const float* __restrict__ dout,
                                                              long long ld_do, float* __restrict__ dz, long long ld_dz,
                                                              float* __restrict__ dp, long long ld_dp) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float s = sigma[r / grid_rows], cs = precond_c_skip(s, d2), co = precond_c_out(s, d, d2);
  for (int c = lane; c < width; c += 64) {
    const float g = ldg1(dout + r * ld_do + c);
    if (dz != nullptr) stg1(dz + r * ld_dz + c, __fmul_rn(cs, g));
    if (dp != nullptr) stg1(dp + r * ld_dp + c, __fmul_rn(co, g));
  }
}

bool precond_ok(int32_t batch, int64_t grid_rows, float sigma_data) {
  return batch >= 1 && grid_rows >= 1 && (int64_t)batch * grid_rows < ((int64_t)1 << 33) && sigma_data > 0.f;
}

// ---- beta gate ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gate_fwd_kernel(long long rows, int width, const float* __restrict__ o, long long ld_o,
                                                       const float* __restrict__ xr, long long ld_x, const float* __restrict__ w,
                                                       float* __restrict__ y, long long ld_y, float* __restrict__ gate) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float t = 0.f;
  for (int c = lane; c < width; c += 64) {
    const float ov = ldg1(o + r * ld_o + c), xv = ldg1(xr + r * ld_x + c);
    t = fmaf(ldg1(w + c), ov, t);
    t = fmaf(ldg1(w + width + c), xv, t);
    t = fmaf(ldg1(w + 2 * width + c), ov - xv, t);
  }
  const float g = sigmoidf_(wave_sum(t));
  for (int c = lane; c < width; c += 64) {
    const float ov = ldg1(o + r * ld_o + c), xv = ldg1(xr + r * ld_x + c);
    stg1(y + r * ld_y + c, g * xv + (1.f - g) * ov);
  }
  if (lane == 0) gate[r] = g;
}

__global__ __launch_bounds__(256) void gate_bwd_rows_kernel(long long rows, int width, const float* __restrict__ o, long long ld_o,
                                                            const float* __restrict__ xr, long long ld_x, const float* __restrict__ w,
                                                            const float* __restrict__ gate, const float* __restrict__ dy,
                                                            long long ld_dy, float* __restrict__ d_o, float* __restrict__ d_x,
                                                            long long ld_d, float* __restrict__ dt) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float s = 0.f;
  for (int c = lane; c < width; c += 64)
    s = fmaf(ldg1(dy + r * ld_dy + c), ldg1(xr + r * ld_x + c) - ldg1(o + r * ld_o + c), s);
  const float g = gate[r];
  const float d = wave_sum(s) * g * (1.f - g);
  for (int c = lane; c < width; c += 64) {
    const float dv = ldg1(dy + r * ld_dy + c), wc = ldg1(w + 2 * width + c);
    if (d_o != nullptr) stg1(d_o + r * ld_d + c, dv * (1.f - g) + d * (ldg1(w + c) + wc));
    if (d_x != nullptr) stg1(d_x + r * ld_d + c, dv * g + d * (ldg1(w + width + c) - wc));
  }
  if (lane == 0) dt[r] = d;
}

// part[slab][3][width]: one thread per column walks the slab's rows in order
__global__ __launch_bounds__(256) void gate_cols_kernel(long long rows, int width, const float* __restrict__ o, long long ld_o,
                                                        const float* __restrict__ xr, long long ld_x, const float* __restrict__ dt,
                                                        float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= width) return;
  const long long r0 = (long long)blockIdx.y * kGateSlab, r1 = r0 + kGateSlab < rows ? r0 + kGateSlab : rows;
  double a = 0.0, b = 0.0, d = 0.0;  // fp64: a chain of 256 fp32 additions would cost more than a pairwise float32 sum
  for (long long r = r0; r < r1; ++r) {
    const float t = dt[r], ov = ldg1(o + r * ld_o + c), xv = ldg1(xr + r * ld_x + c);
    a += (double)(t * ov);
    b += (double)(t * xv);
    d += (double)(t * (ov - xv));
  }
  float* p = part + (long long)blockIdx.y * 3 * width;
  p[c] = (float)a;
  p[width + c] = (float)b;
  p[2 * width + c] = (float)d;
}

__global__ __launch_bounds__(256) void gate_sum_kernel(int slabs, int n, const float* __restrict__ part, float* __restrict__ dw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int sl = 0; sl < slabs; ++sl) s += (double)ldg1(part + (long long)sl * n + e);
  dw[e] = (float)s;
}

bool gate_ok(int64_t rows, int width) {
  return rows >= 0 && width >= 1 && width <= (1 << 20) && (rows + kGateSlab - 1) / kGateSlab <= 65535;
}
size_t gate_bytes(int64_t rows, int width) {
  return ((size_t)rows + (size_t)((rows + kGateSlab - 1) / kGateSlab) * 3 * (size_t)width) * sizeof(float);
}

// ---- SiLU, Fourier features -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void silu_fwd_kernel(long long n, const float* __restrict__ x, float* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) y[i] = act_f(x[i], GW_ACT_SILU);
}
__global__ __launch_bounds__(256) void silu_bwd_kernel(long long n, const float* __restrict__ x, const float* __restrict__ dy,
                                                       float* __restrict__ dx) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    dx[i] = dy[i] * act_d(x[i], GW_ACT_SILU);
}

// f_i = exp(-ln(base_period) i / F) in float32, operation by operation as modules.py:184-188 forms it
__device__ __forceinline__ float fourier_freq(int i, int F, float neg_log_base) { return expf(neg_log_base * (float)i / (float)F); }

__global__ __launch_bounds__(256) void fourier_fwd_kernel(long long rows, int F, float neg_log_base, const float* __restrict__ t,
                                                          float* __restrict__ out, long long ld_o) {
  const long long n = rows * F;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long long)gridDim.x * 256) {
    const long long r = idx / F;
    const int i = (int)(idx - r * F);
    const float arg = t[r] * fourier_freq(i, F, neg_log_base);
    out[r * ld_o + i] = cosf(arg);
    out[r * ld_o + F + i] = sinf(arg);
  }
}

__global__ __launch_bounds__(256) void fourier_bwd_kernel(long long rows, int F, float neg_log_base, const float* __restrict__ t,
                                                          const float* __restrict__ dout, long long ld_do, float* __restrict__ dt) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float tv = t[r];
  float s = 0.f;
  for (int i = lane; i < F; i += 64) {
    const float f = fourier_freq(i, F, neg_log_base), arg = tv * f;
    s += f * (cosf(arg) * ldg1(dout + r * ld_do + F + i) - sinf(arg) * ldg1(dout + r * ld_do + i));
  }
  s = wave_sum(s);
  if (lane == 0) dt[r] = s;
}

int attn_check(const char* bad, int32_t batch, int64_t e_bstride, int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads,
               int32_t dim_head) {
  if (n_dst < 0 || n_src < 0 || n_edges < 0 || heads < 1 || dim_head < 1 || batch < 1) return failf(GW_E_BADARG, bad);
  if (e_bstride != 0 && e_bstride < n_edges) return failf(GW_E_BADARG, bad);  // the tables of two copies would overlap
  if ((int64_t)heads * dim_head > kMaxRow) return failf(GW_E_UNSUPPORTED, "graph attention: heads * dim_head must be at most 4096");
  if ((int64_t)batch * n_dst * heads >= ((int64_t)1 << 31) || (int64_t)batch * n_src * heads >= ((int64_t)1 << 31))
    return failf(GW_E_BADARG, bad);
  return GW_OK;
}

}  // namespace

extern "C" {

static int attn_forward(const char* bad, int32_t batch, int64_t e_bstride, int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads,
                        int32_t dim_head, const int32_t* dst_ptr, const int32_t* src, const int64_t* perm, const float* q, int32_t ld_q,
                        const float* k, int32_t ld_k, const float* v, int32_t ld_v, const float* e, int32_t ld_e, int32_t mean, float* out,
                        int32_t ld_out, float* out_heads, int32_t ld_out_heads, float* lse, void* stream) {
  if (int rc = attn_check(bad, batch, e_bstride, n_dst, n_src, n_edges, heads, dim_head)) return rc;
  if (n_dst == 0 || n_edges == 0) return GW_OK;
  const int hc = heads * dim_head;
  if (!dst_ptr || !src || !q || !k || !v || !out || !lse || n_src < 1 || ld_q < hc || ld_k < hc || ld_v < hc || (e && ld_e < hc) ||
      ld_out < (mean ? dim_head : hc) || (out_heads && ld_out_heads < hc))
    return failf(GW_E_BADARG, bad);
  const bool vec = dim_head % 4 == 0 && ld_q % 4 == 0 && ld_k % 4 == 0 && ld_v % 4 == 0 && ld_out % 4 == 0 && (!e || ld_e % 4 == 0) &&
                   (!out_heads || ld_out_heads % 4 == 0) && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(e) &&
                   aligned16(out) && aligned16(out_heads);
  AttnArgs a = {};
  a.n_dst = n_dst, a.n_src = n_src, a.heads = heads, a.C = dim_head, a.mean = mean ? 1 : 0;
  a.dst_ptr = dst_ptr, a.src = src, a.perm = (const long long*)perm;
  a.q = q, a.k = k, a.v = v, a.e = e, a.ld_q = ld_q, a.ld_k = ld_k, a.ld_v = ld_v, a.ld_e = ld_e;
  a.out = out, a.ld_out = ld_out, a.out_heads = mean ? out_heads : nullptr, a.ld_oh = ld_out_heads, a.lse = lse;
  a.sqrt_c = sqrtf((float)dim_head);
  a.batch = batch, a.e_bstride = e_bstride, a.planes = (long long)batch * n_dst * heads;
  const int64_t items = (mean ? (int64_t)n_dst : (int64_t)n_dst * heads) * batch;
  const unsigned grid = (unsigned)((items + 3) / 4);
  const int variant = attn_variant(dim_head, vec);
#define GW_GC_FWD(NE, VEC, U) hipLaunchKernelGGL((attn_fwd_kernel<NE, VEC, U>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a)
  GW_GC_VARIANTS(GW_GC_FWD, hipLaunchKernelGGL(attn_fwd_long_kernel, dim3((unsigned)items), dim3(64), 0, (hipStream_t)stream, a))
#undef GW_GC_FWD
  return check_launch("attn_fwd_kernel launch");
}

int gw_graph_attention_forward(int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads, int32_t dim_head, const int32_t* dst_ptr,
                               const int32_t* src, const int64_t* perm, const float* q, int32_t ld_q, const float* k, int32_t ld_k,
                               const float* v, int32_t ld_v, const float* e, int32_t ld_e, int32_t mean, float* out, int32_t ld_out,
                               float* out_heads, int32_t ld_out_heads, float* lse, void* stream) {
  return attn_forward("gw_graph_attention_forward: bad arguments", 1, 0, n_dst, n_src, n_edges, heads, dim_head, dst_ptr, src, perm, q,
                      ld_q, k, ld_k, v, ld_v, e, ld_e, mean, out, ld_out, out_heads, ld_out_heads, lse, stream);
}

int gw_graph_attention_batched_forward(int32_t batch, int64_t e_batch_stride, int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads,
                                       int32_t dim_head, const int32_t* dst_ptr, const int32_t* src, const int64_t* perm, const float* q,
                                       int32_t ld_q, const float* k, int32_t ld_k, const float* v, int32_t ld_v, const float* e, int32_t ld_e,
                                       int32_t mean, float* out, int32_t ld_out, float* out_heads, int32_t ld_out_heads, float* lse,
                                       void* stream) {
  return attn_forward("gw_graph_attention_batched_forward: bad arguments", batch, e_batch_stride, n_dst, n_src, n_edges, heads, dim_head,
                      dst_ptr, src, perm, q, ld_q, k, ld_k, v, ld_v, e, ld_e, mean, out, ld_out, out_heads, ld_out_heads, lse, stream);
}

static int attn_backward(const char* bad, int32_t batch, int64_t e_bstride, int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads,
                         int32_t dim_head, const int32_t* dst_ptr, const int32_t* src, const int32_t* dst, const int64_t* perm,
                         const int32_t* src_pos, const int32_t* src_ptr, const float* q, int32_t ld_q, const float* k, int32_t ld_k,
                         const float* v, int32_t ld_v, const float* e, int32_t ld_e, int32_t mean, const float* out_heads,
                         int32_t ld_out_heads, const float* dout, int32_t ld_dout, const float* lse, float* delta, float* dq, int32_t ld_dq,
                         float* dk, int32_t ld_dk, float* dv, int32_t ld_dv, float* de, int32_t ld_de, void* stream) {
  if (int rc = attn_check(bad, batch, e_bstride, n_dst, n_src, n_edges, heads, dim_head)) return rc;
  if (n_edges == 0 || n_dst == 0 || n_src == 0) return GW_OK;
  const int hc = heads * dim_head;
  if (!dst_ptr || !src || !dst || !src_pos || !src_ptr || !q || !k || !v || !out_heads || !dout || !lse || !delta || !dq || !dk || !dv ||
      (de && !e) || ld_q < hc || ld_k < hc || ld_v < hc || (e && ld_e < hc) || ld_out_heads < hc || ld_dout < (mean ? dim_head : hc) ||
      ld_dq < hc || ld_dk < hc || ld_dv < hc || (de && ld_de < hc))
    return failf(GW_E_BADARG, bad);
  const bool vec = dim_head % 4 == 0 && ld_q % 4 == 0 && ld_k % 4 == 0 && ld_v % 4 == 0 && (!e || ld_e % 4 == 0) && ld_out_heads % 4 == 0 &&
                   ld_dout % 4 == 0 && ld_dq % 4 == 0 && ld_dk % 4 == 0 && ld_dv % 4 == 0 && (!de || ld_de % 4 == 0) && aligned16(q) &&
                   aligned16(k) && aligned16(v) && aligned16(e) && aligned16(out_heads) && aligned16(dout) && aligned16(dq) &&
                   aligned16(dk) && aligned16(dv) && aligned16(de);
  AttnArgs a = {};
  a.n_dst = n_dst, a.n_src = n_src, a.heads = heads, a.C = dim_head, a.mean = mean ? 1 : 0;
  a.dst_ptr = dst_ptr, a.src = src, a.dst = dst, a.perm = (const long long*)perm, a.src_pos = src_pos, a.src_ptr = src_ptr;
  a.q = q, a.k = k, a.v = v, a.e = e, a.ld_q = ld_q, a.ld_k = ld_k, a.ld_v = ld_v, a.ld_e = ld_e;
  a.out_heads = const_cast<float*>(out_heads), a.ld_oh = ld_out_heads, a.lse = const_cast<float*>(lse);
  a.dout = dout, a.ld_dout = ld_dout, a.delta = delta;
  a.dq = dq, a.dk = dk, a.dv = dv, a.de = de, a.ld_dq = ld_dq, a.ld_dk = ld_dk, a.ld_dv = ld_dv, a.ld_de = ld_de;
  a.sqrt_c = sqrtf((float)dim_head);
  a.batch = batch, a.e_bstride = e_bstride, a.planes = (long long)batch * n_dst * heads;
  a.de_loop = (de != nullptr && batch > 1 && e_bstride == 0) ? 1 : 0;  // one de table for every copy: summed by the owning wave
  const int variant = attn_variant(dim_head, vec);
  const int64_t items_d = (int64_t)n_dst * heads * (a.de_loop ? 1 : batch), items_s = (int64_t)n_src * heads * batch;
  const unsigned grid_d = (unsigned)((items_d + 3) / 4), grid_s = (unsigned)((items_s + 3) / 4);
#define GW_GC_BWD_DST(NE, VEC, U)                                                                                      \
  if (a.de_loop)                                                                                                       \
    hipLaunchKernelGGL((attn_bwd_dst_kernel<NE, VEC, true>), dim3(grid_d), dim3(256), 0, (hipStream_t)stream, a);       \
  else                                                                                                                 \
    hipLaunchKernelGGL((attn_bwd_dst_kernel<NE, VEC, false>), dim3(grid_d), dim3(256), 0, (hipStream_t)stream, a)
  GW_GC_VARIANTS(GW_GC_BWD_DST, if (a.de_loop) hipLaunchKernelGGL(attn_bwd_dst_long_kernel<true>, dim3((unsigned)items_d), dim3(64), 0,
                                                                   (hipStream_t)stream, a);
                                else hipLaunchKernelGGL(attn_bwd_dst_long_kernel<false>, dim3((unsigned)items_d), dim3(64), 0,
                                                        (hipStream_t)stream, a))
#undef GW_GC_BWD_DST
  if (int rc = check_launch("attn_bwd_dst_kernel launch")) return rc;
#define GW_GC_BWD_SRC(NE, VEC, U) hipLaunchKernelGGL((attn_bwd_src_kernel<NE, VEC>), dim3(grid_s), dim3(256), 0, (hipStream_t)stream, a)
  GW_GC_VARIANTS(GW_GC_BWD_SRC, hipLaunchKernelGGL(attn_bwd_src_long_kernel, dim3((unsigned)items_s), dim3(64), 0,
                                                   (hipStream_t)stream, a))
#undef GW_GC_BWD_SRC
  return check_launch("attn_bwd_src_kernel launch");
}

int gw_graph_attention_backward(int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads, int32_t dim_head, const int32_t* dst_ptr,
                                const int32_t* src, const int32_t* dst, const int64_t* perm, const int32_t* src_pos,
                                const int32_t* src_ptr, const float* q, int32_t ld_q, const float* k, int32_t ld_k, const float* v,
                                int32_t ld_v, const float* e, int32_t ld_e, int32_t mean, const float* out_heads, int32_t ld_out_heads,
                                const float* dout, int32_t ld_dout, const float* lse, float* delta, float* dq, int32_t ld_dq, float* dk,
                                int32_t ld_dk, float* dv, int32_t ld_dv, float* de, int32_t ld_de, void* stream) {
  return attn_backward("gw_graph_attention_backward: bad arguments", 1, 0, n_dst, n_src, n_edges, heads, dim_head, dst_ptr, src, dst, perm,
                       src_pos, src_ptr, q, ld_q, k, ld_k, v, ld_v, e, ld_e, mean, out_heads, ld_out_heads, dout, ld_dout, lse, delta, dq,
                       ld_dq, dk, ld_dk, dv, ld_dv, de, ld_de, stream);
}

int gw_graph_attention_batched_backward(int32_t batch, int64_t e_batch_stride, int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t heads,
                                        int32_t dim_head, const int32_t* dst_ptr, const int32_t* src, const int32_t* dst,
                                        const int64_t* perm, const int32_t* src_pos, const int32_t* src_ptr, const float* q, int32_t ld_q,
                                        const float* k, int32_t ld_k, const float* v, int32_t ld_v, const float* e, int32_t ld_e,
                                        int32_t mean, const float* out_heads, int32_t ld_out_heads, const float* dout, int32_t ld_dout,
                                        const float* lse, float* delta, float* dq, int32_t ld_dq, float* dk, int32_t ld_dk, float* dv,
                                        int32_t ld_dv, float* de, int32_t ld_de, void* stream) {
  return attn_backward("gw_graph_attention_batched_backward: bad arguments", batch, e_batch_stride, n_dst, n_src, n_edges, heads, dim_head,
                       dst_ptr, src, dst, perm, src_pos, src_ptr, q, ld_q, k, ld_k, v, ld_v, e, ld_e, mean, out_heads, ld_out_heads, dout,
                       ld_dout, lse, delta, dq, ld_dq, dk, ld_dk, dv, ld_dv, de, ld_de, stream);
}

int gw_cond_layernorm_forward(int64_t rows, int32_t width, int32_t act, const float* x, int32_t ld_x, const float* scale, int32_t ld_scale,
                              const float* bias, int32_t ld_bias, float* out, int32_t ld_out, void* stream) {
  if (!x || !scale || !bias || !out || rows < 0 || rows >= ((int64_t)1 << 33) || width < 1 || act < GW_ACT_NONE || act > GW_ACT_SILU ||
      ld_x < width || ld_scale < width || ld_bias < width || ld_out < width)
    return failf(GW_E_BADARG, "gw_cond_layernorm_forward: bad arguments");
  if (rows == 0) return GW_OK;
  hipLaunchKernelGGL(cln_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long long)rows, (int)width,
                     (int)act, x, (long long)ld_x, scale, (long long)ld_scale, bias, (long long)ld_bias, out, (long long)ld_out, 1LL);
  return check_launch("cln_fwd_kernel launch");
}

int gw_cond_layernorm_backward(int64_t rows, int32_t width, int32_t act, const float* x, int32_t ld_x, const float* scale,
                               int32_t ld_scale, const float* bias, int32_t ld_bias, const float* dout, int32_t ld_dout, float* dx,
                               int32_t ld_dx, float* dscale, float* dbias, int32_t ld_dsb, void* stream) {
  if (!x || !scale || !bias || !dout || (!dx && !dscale && !dbias) || rows < 0 || rows >= ((int64_t)1 << 33) || width < 1 ||
      act < GW_ACT_NONE || act > GW_ACT_SILU || ld_x < width || ld_scale < width || ld_bias < width || ld_dout < width ||
      (dx && ld_dx < width) || ((dscale || dbias) && ld_dsb < width))
    return failf(GW_E_BADARG, "gw_cond_layernorm_backward: bad arguments");
  if (rows == 0) return GW_OK;
  hipLaunchKernelGGL(cln_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long long)rows, (int)width,
                     (int)act, x, (long long)ld_x, scale, (long long)ld_scale, bias, (long long)ld_bias, dout, (long long)ld_dout, dx,
                     (long long)ld_dx, dscale, dbias, (long long)ld_dsb, 1LL, (float*)nullptr);
  return check_launch("cln_bwd_kernel launch");
}

int gw_cond_layernorm_grouped_forward(int64_t rows, int32_t width, int32_t act, int64_t rows_per_group, const float* x, int32_t ld_x,
                                      const float* scale, int32_t ld_scale, const float* bias, int32_t ld_bias, float* out, int32_t ld_out,
                                      void* stream) {
  if (!x || !scale || !bias || !out || !cln_grouped_ok(rows, width, rows_per_group) || act < GW_ACT_NONE || act > GW_ACT_SILU ||
      ld_x < width || ld_scale < width || ld_bias < width || ld_out < width)
    return failf(GW_E_BADARG, "gw_cond_layernorm_grouped_forward: bad arguments");
  if (rows == 0) return GW_OK;
  hipLaunchKernelGGL(cln_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long long)rows, (int)width,
                     (int)act, x, (long long)ld_x, scale, (long long)ld_scale, bias, (long long)ld_bias, out, (long long)ld_out,
                     (long long)rows_per_group);
  return check_launch("cln_fwd_kernel launch");
}

size_t gw_cond_layernorm_grouped_workspace_bytes(int64_t rows, int32_t width, int64_t rows_per_group) {
  if (!cln_grouped_ok(rows, width, rows_per_group) || rows < 1) {
    failf(GW_E_BADARG, "gw_cond_layernorm_grouped_workspace_bytes: bad arguments");
    return 0;
  }
  return cln_grouped_bytes(rows, width, rows_per_group);
}

int gw_cond_layernorm_grouped_backward(int64_t rows, int32_t width, int32_t act, int64_t rows_per_group, const float* x, int32_t ld_x,
                                       const float* scale, int32_t ld_scale, const float* bias, int32_t ld_bias, const float* dout,
                                       int32_t ld_dout, void* workspace, size_t workspace_bytes, float* dx, int32_t ld_dx, float* dscale,
                                       float* dbias, int32_t ld_dsb, void* stream) {
  const char* bad = "gw_cond_layernorm_grouped_backward: bad arguments";
  if (!x || !scale || !bias || !dout || !workspace || (!dx && !dscale && !dbias) || !cln_grouped_ok(rows, width, rows_per_group) ||
      act < GW_ACT_NONE || act > GW_ACT_SILU || ld_x < width || ld_scale < width || ld_bias < width || ld_dout < width ||
      (dx && ld_dx < width) || ((dscale || dbias) && ld_dsb < width))
    return failf(GW_E_BADARG, bad);
  if (rows == 0) return GW_OK;
  if (workspace_bytes < cln_grouped_bytes(rows, width, rows_per_group))
    return failf(GW_E_BADARG, "gw_cond_layernorm_grouped_backward: bad arguments (workspace)");
  float* stats = (float*)workspace;
  float* part = stats + 2 * rows;
  hipStream_t st = (hipStream_t)stream;
  // (with dx NULL the row kernel still leaves the statistics the column pass reads)
  hipLaunchKernelGGL(cln_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (long long)rows, (int)width, (int)act, x,
                     (long long)ld_x, scale, (long long)ld_scale, bias, (long long)ld_bias, dout, (long long)ld_dout, dx, (long long)ld_dx,
                     (float*)nullptr, (float*)nullptr, (long long)ld_dsb, (long long)rows_per_group, stats);
  if (int rc = check_launch("cln_bwd_kernel launch")) return rc;
  if (!dscale && !dbias) return GW_OK;
  const int64_t groups = (rows + rows_per_group - 1) / rows_per_group;
  // slabs of the longest group (a shorter last group leaves its later slabs empty: zero partials)
  const int slabs = (int)(((rows_per_group < rows ? rows_per_group : rows) + kGateSlab - 1) / kGateSlab);
  hipLaunchKernelGGL(cln_cols_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)slabs, (unsigned)groups), dim3(256), 0, st,
                     (long long)rows, (int)width, (int)act, (long long)rows_per_group, x, (long long)ld_x, scale, (long long)ld_scale, bias,
                     (long long)ld_bias, dout, (long long)ld_dout, (const float*)stats, part, 0LL);
  if (int rc = check_launch("cln_cols_kernel launch")) return rc;
  hipLaunchKernelGGL(cln_sum_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)groups), dim3(256), 0, st, slabs, (int)width,
                     (const float*)part, dscale, dbias, (long long)ld_dsb);
  return check_launch("cln_sum_kernel launch");
}

int gw_cond_layernorm_fanout_forward(int64_t x_rows, int32_t width, int32_t act, int64_t rows_per_sample, int32_t members, const float* x,
                                     int32_t ld_x, const float* scale, int32_t ld_scale, const float* bias, int32_t ld_bias, float* out,
                                     int32_t ld_out, void* stream) {
  if (!x || !scale || !bias || !out || !cln_fanout_ok(x_rows, width, rows_per_sample, members) || act < GW_ACT_NONE || act > GW_ACT_SILU ||
      ld_x < width || ld_scale < width || ld_bias < width || ld_out < width)
    return failf(GW_E_BADARG, "gw_cond_layernorm_fanout_forward: bad arguments");
  if (x_rows == 0) return GW_OK;
  hipLaunchKernelGGL(cln_fan_fwd_kernel, dim3((unsigned)((x_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long long)x_rows,
                     (int)width, (int)act, (long long)rows_per_sample, (int)members, x, (long long)ld_x, scale, (long long)ld_scale, bias,
                     (long long)ld_bias, out, (long long)ld_out);
  return check_launch("cln_fan_fwd_kernel launch");
}

size_t gw_cond_layernorm_fanout_workspace_bytes(int64_t x_rows, int32_t width, int64_t rows_per_sample, int32_t members) {
  if (!cln_fanout_ok(x_rows, width, rows_per_sample, members) || x_rows < 1) {
    failf(GW_E_BADARG, "gw_cond_layernorm_fanout_workspace_bytes: bad arguments");
    return 0;
  }
  return cln_fanout_bytes(x_rows, width, rows_per_sample, members);
}

int gw_cond_layernorm_fanout_backward(int64_t x_rows, int32_t width, int32_t act, int64_t rows_per_sample, int32_t members, const float* x,
                                      int32_t ld_x, const float* scale, int32_t ld_scale, const float* bias, int32_t ld_bias,
                                      const float* dout, int32_t ld_dout, void* workspace, size_t workspace_bytes, float* dx, int32_t ld_dx,
                                      float* dscale, float* dbias, int32_t ld_dsb, void* stream) {
  if (!x || !scale || !bias || !dout || !workspace || (!dx && !dscale && !dbias) ||
      !cln_fanout_ok(x_rows, width, rows_per_sample, members) || act < GW_ACT_NONE || act > GW_ACT_SILU || ld_x < width || ld_scale < width ||
      ld_bias < width || ld_dout < width || (dx && ld_dx < width) || ((dscale || dbias) && ld_dsb < width))
    return failf(GW_E_BADARG, "gw_cond_layernorm_fanout_backward: bad arguments");
  if (x_rows == 0) return GW_OK;
  if (workspace_bytes < cln_fanout_bytes(x_rows, width, rows_per_sample, members))
    return failf(GW_E_BADARG, "gw_cond_layernorm_fanout_backward: bad arguments (workspace)");
  float* stats = (float*)workspace;
  float* part = stats + 2 * x_rows;
  hipStream_t st = (hipStream_t)stream;
  // (with dx NULL the row kernel still leaves the statistics the column pass reads)
  hipLaunchKernelGGL(cln_fan_bwd_kernel, dim3((unsigned)((x_rows + 3) / 4)), dim3(256), 0, st, (long long)x_rows, (int)width, (int)act,
                     (long long)rows_per_sample, (int)members, x, (long long)ld_x, scale, (long long)ld_scale, bias, (long long)ld_bias,
                     dout, (long long)ld_dout, dx, (long long)ld_dx, stats);
  if (int rc = check_launch("cln_fan_bwd_kernel launch")) return rc;
  if (!dscale && !dbias) return GW_OK;
  const int64_t groups = x_rows / rows_per_sample * members;
  const int slabs = (int)((rows_per_sample + kGateSlab - 1) / kGateSlab);
  hipLaunchKernelGGL(cln_cols_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)slabs, (unsigned)groups), dim3(256), 0, st,
                     (long long)(groups * rows_per_sample), (int)width, (int)act, (long long)rows_per_sample, x, (long long)ld_x, scale,
                     (long long)ld_scale, bias, (long long)ld_bias, dout, (long long)ld_dout, (const float*)stats, part, (long long)members);
  if (int rc = check_launch("cln_cols_kernel launch")) return rc;
  hipLaunchKernelGGL(cln_sum_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)groups), dim3(256), 0, st, slabs, (int)width,
                     (const float*)part, dscale, dbias, (long long)ld_dsb);
  return check_launch("cln_sum_kernel launch");
}

int gw_gencast_precond_input_forward(int32_t batch, int64_t grid_rows, int32_t w_z, int32_t w_x, int32_t w_s, float sigma_data,
                                     const float* sigma, const float* z, int32_t ld_z, const float* x, int32_t ld_x, const float* stat,
                                     int32_t ld_stat, float* out, int32_t ld_out, float* c_noise, void* stream) {
  if (!precond_ok(batch, grid_rows, sigma_data) || !sigma || !out || w_z < 0 || w_x < 0 || w_s < 0 || (w_z && (!z || ld_z < w_z)) ||
      (w_x && (!x || ld_x < w_x)) || (w_s && (!stat || ld_stat < w_s)) || (int64_t)w_z + w_x + w_s < 1 || ld_out < (int64_t)w_z + w_x + w_s)
    return failf(GW_E_BADARG, "gw_gencast_precond_input_forward: bad arguments");
  const long long rows = (long long)batch * grid_rows;
  hipLaunchKernelGGL(precond_in_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, rows, (long long)grid_rows,
                     (int)w_z, (int)w_x, (int)w_s, (float)((double)sigma_data * sigma_data), sigma, z, (long long)ld_z, x, (long long)ld_x, stat,
                     (long long)ld_stat, out, (long long)ld_out, c_noise);
  return check_launch("precond_in_fwd_kernel launch");
}

int gw_gencast_precond_input_backward(int32_t batch, int64_t grid_rows, int32_t w_z, int32_t w_x, float sigma_data, const float* sigma,
                                      const float* dout, int32_t ld_dout, float* dz, int32_t ld_dz, float* dx, int32_t ld_dx,
                                      void* stream) {
  if (!precond_ok(batch, grid_rows, sigma_data) || !sigma || !dout || (!dz && !dx) || w_z < 0 || w_x < 0 || ld_dout < (int64_t)w_z + w_x ||
      (dz && ld_dz < w_z) || (dx && ld_dx < w_x))
    return failf(GW_E_BADARG, "gw_gencast_precond_input_backward: bad arguments");
  const long long rows = (long long)batch * grid_rows;
  hipLaunchKernelGGL(precond_in_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, rows, (long long)grid_rows,
                     (int)w_z, (int)w_x, (float)((double)sigma_data * sigma_data), sigma, dout, (long long)ld_dout, dz, (long long)ld_dz, dx,
                     (long long)ld_dx);
  return check_launch("precond_in_bwd_kernel launch");
}

int gw_gencast_precond_output_forward(int32_t batch, int64_t grid_rows, int32_t width, float sigma_data, const float* sigma, const float* z,
                                      int32_t ld_z, const float* preds, int32_t ld_preds, float* out, int32_t ld_out, void* stream) {
  if (!precond_ok(batch, grid_rows, sigma_data) || !sigma || !z || !preds || !out || width < 1 || ld_z < width || ld_preds < width ||
      ld_out < width)
    return failf(GW_E_BADARG, "gw_gencast_precond_output_forward: bad arguments");
  const long long rows = (long long)batch * grid_rows;
  hipLaunchKernelGGL(precond_out_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, rows,
                     (long long)grid_rows, (int)width, sigma_data, (float)((double)sigma_data * sigma_data), sigma, z, (long long)ld_z, preds,
                     (long long)ld_preds, out, (long long)ld_out);
  return check_launch("precond_out_fwd_kernel launch");
}

int gw_gencast_precond_output_backward(int32_t batch, int64_t grid_rows, int32_t width, float sigma_data, const float* sigma,
                                       const float* dout, int32_t ld_dout, float* dz, int32_t ld_dz, float* dpreds, int32_t ld_dpreds,
                                       void* stream) {
  if (!precond_ok(batch, grid_rows, sigma_data) || !sigma || !dout || (!dz && !dpreds) || width < 1 || ld_dout < width ||
      (dz && ld_dz < width) || (dpreds && ld_dpreds < width))
    return failf(GW_E_BADARG, "gw_gencast_precond_output_backward: bad arguments");
  const long long rows = (long long)batch * grid_rows;
  hipLaunchKernelGGL(precond_out_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, rows,
                     (long long)grid_rows, (int)width, sigma_data, (float)((double)sigma_data * sigma_data), sigma, dout, (long long)ld_dout, dz,
                     (long long)ld_dz, dpreds, (long long)ld_dpreds);
  return check_launch("precond_out_bwd_kernel launch");
}

int gw_beta_gate_forward(int64_t rows, int32_t width, const float* out, int32_t ld_out, const float* x_r, int32_t ld_xr, const float* w,
                         float* y, int32_t ld_y, float* gate, void* stream) {
  if (!out || !x_r || !w || !y || !gate || !gate_ok(rows, width) || ld_out < width || ld_xr < width || ld_y < width)
    return failf(GW_E_BADARG, "gw_beta_gate_forward: bad arguments");
  if (rows == 0) return GW_OK;
  hipLaunchKernelGGL(gate_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long long)rows, (int)width, out,
                     (long long)ld_out, x_r, (long long)ld_xr, w, y, (long long)ld_y, gate);
  return check_launch("gate_fwd_kernel launch");
}

size_t gw_beta_gate_workspace_bytes(int64_t rows, int32_t width) {
  if (!gate_ok(rows, width) || rows < 1) {
    failf(GW_E_BADARG, "gw_beta_gate_workspace_bytes: bad arguments");
    return 0;
  }
  return gate_bytes(rows, width);
}

int gw_beta_gate_backward(int64_t rows, int32_t width, const float* out, int32_t ld_out, const float* x_r, int32_t ld_xr, const float* w,
                          const float* gate, const float* dy, int32_t ld_dy, void* workspace, size_t workspace_bytes, float* d_out,
                          float* d_xr, int32_t ld_d, float* dw, void* stream) {
  const char* bad = "gw_beta_gate_backward: bad arguments";
  if (!out || !x_r || !w || !gate || !dy || !workspace || !dw || !gate_ok(rows, width) || ld_out < width || ld_xr < width ||
      ld_dy < width || ((d_out || d_xr) && ld_d < width))
    return failf(GW_E_BADARG, bad);
  if (rows == 0) return GW_OK;
  if (workspace_bytes < gate_bytes(rows, width)) return failf(GW_E_BADARG, "gw_beta_gate_backward: bad arguments (workspace)");
  float* dt = (float*)workspace;
  float* part = dt + rows;
  const int slabs = (int)((rows + kGateSlab - 1) / kGateSlab);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gate_bwd_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (long long)rows, (int)width, out,
                     (long long)ld_out, x_r, (long long)ld_xr, w, gate, dy, (long long)ld_dy, d_out, d_xr, (long long)ld_d, dt);
  if (int rc = check_launch("gate_bwd_rows_kernel launch")) return rc;
  hipLaunchKernelGGL(gate_cols_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)slabs), dim3(256), 0, st, (long long)rows,
                     (int)width, out, (long long)ld_out, x_r, (long long)ld_xr, (const float*)dt, part);
  if (int rc = check_launch("gate_cols_kernel launch")) return rc;
  hipLaunchKernelGGL(gate_sum_kernel, dim3((unsigned)((3 * width + 255) / 256)), dim3(256), 0, st, slabs, 3 * (int)width, (const float*)part,
                     dw);
  return check_launch("gate_sum_kernel launch");
}

int gw_silu_forward(int64_t n, const float* x, float* y, void* stream) {
  if (!x || !y || n < 0) return failf(GW_E_BADARG, "gw_silu_forward: bad arguments");
  if (n == 0) return GW_OK;
  hipLaunchKernelGGL(silu_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (long long)n, x, y);
  return check_launch("silu_fwd_kernel launch");
}

int gw_silu_backward(int64_t n, const float* x, const float* dy, float* dx, void* stream) {
  if (!x || !dy || !dx || n < 0) return failf(GW_E_BADARG, "gw_silu_backward: bad arguments");
  if (n == 0) return GW_OK;
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (long long)n, x, dy, dx);
  return check_launch("silu_bwd_kernel launch");
}

int gw_fourier_forward(int64_t rows, int32_t num_frequencies, float base_period, const float* t, float* out, int32_t ld_out, void* stream) {
  if (!t || !out || rows < 0 || num_frequencies < 1 || !(base_period > 0.f) || ld_out < 2 * num_frequencies)
    return failf(GW_E_BADARG, "gw_fourier_forward: bad arguments");
  if (rows == 0) return GW_OK;
  hipLaunchKernelGGL(fourier_fwd_kernel, dim3(grid_for(rows * num_frequencies)), dim3(256), 0, (hipStream_t)stream, (long long)rows,
                     (int)num_frequencies, (float)(-log((double)base_period)), t, out, (long long)ld_out);
  return check_launch("fourier_fwd_kernel launch");
}

int gw_fourier_backward(int64_t rows, int32_t num_frequencies, float base_period, const float* t, const float* dout, int32_t ld_dout,
                        float* dt, void* stream) {
  if (!t || !dout || !dt || rows < 0 || rows >= ((int64_t)1 << 33) || num_frequencies < 1 || !(base_period > 0.f) ||
      ld_dout < 2 * num_frequencies)
    return failf(GW_E_BADARG, "gw_fourier_backward: bad arguments");
  if (rows == 0) return GW_OK;
  hipLaunchKernelGGL(fourier_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long long)rows,
                     (int)num_frequencies, (float)(-log((double)base_period)), t, dout, (long long)ld_dout, dt);
  return check_launch("fourier_bwd_kernel launch");
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The Sampler's state updates (sampler.py) and WeightedMSELoss (weighted_mse_loss.py).
//   combine_kernel   out = a x + b y + c z on n dense floats with host scalars; a null operand is skipped.  float4 body and a
//                    scalar tail through one expression (a x, then fmaf for y, then fmaf for z), so an element's result does
//                    not depend on where it sits.  out may alias x (every element is read before it is written, by its own thread).
//   wmse_fwd_kernel  per slab of kWmseSlab elements of [B, lon, lat, var]: sum of (pred - target)^2 aw[lat] fw[var] lambda(sigma_b)
//                    in fp64, lambda(s) = (s^2 + d^2) / (s d)^2 formed in float32 as the reference forms it, and a flag that a
//                    squared residual was NaN; wmse_final_kernel adds the slabs' sums as a fixed-shape tree and ORs the flags.
//   wmse_bwd_kernel  dpred = dloss * 2 (pred - target) aw fw lambda / n.
// No atomics: equal inputs give bitwise equal results.
namespace {

constexpr int kWmseSlab = 4096;  // elements per workgroup of wmse_fwd_kernel (16 per thread)

__device__ inline float combine1(bool hx, bool hy, bool hz, float a, float b, float c, float x, float y, float z) {
  float r = hx ? __fmul_rn(a, x) : 0.f;
  if (hy) r = hx ? fmaf(b, y, r) : __fmul_rn(b, y);
  if (hz) r = (hx || hy) ? fmaf(c, z, r) : __fmul_rn(c, z);
  return r;
}

__global__ __launch_bounds__(256) void combine_kernel(long long n, long long n4, float a, float b, float c, const float* x, const float* y,
                                                      const float* z, float* out) {
  const bool hx = x != nullptr, hy = y != nullptr, hz = z != nullptr;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 vx = hx ? ((const float4*)x)[i] : zero, vy = hy ? ((const float4*)y)[i] : zero, vz = hz ? ((const float4*)z)[i] : zero;
    float4 r;
    r.x = combine1(hx, hy, hz, a, b, c, vx.x, vy.x, vz.x);
    r.y = combine1(hx, hy, hz, a, b, c, vx.y, vy.y, vz.y);
    r.z = combine1(hx, hy, hz, a, b, c, vx.z, vy.z, vz.z);
    r.w = combine1(hx, hy, hz, a, b, c, vx.w, vy.w, vz.w);
    ((float4*)out)[i] = r;
  }
  for (long long i = 4 * n4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
    out[i] = combine1(hx, hy, hz, a, b, c, hx ? x[i] : 0.f, hy ? y[i] : 0.f, hz ? z[i] : 0.f);
}

__device__ inline float wmse_lambda(float s, float d) {
  const float sd = __fmul_rn(s, d);
  return __fdiv_rn(__fadd_rn(__fmul_rn(s, s), __fmul_rn(d, d)), __fmul_rn(sd, sd));
}

// weight of element e of [B, lon, lat, var]: aw[lat] fw[var] (each optional), and its sample
__device__ inline float wmse_weight(long long e, int nlat, int nvar, long long per_sample, const float* aw, const float* fw, int* sample) {
  const long long row = e / nvar;
  float w = 1.f;
  if (aw) w = aw[(int)(row % nlat)];
  if (fw) w = __fmul_rn(w, fw[(int)(e - row * nvar)]);
  *sample = (int)(e / per_sample);
  return w;
}

__global__ __launch_bounds__(256) void wmse_fwd_kernel(long long n, int nlat, int nvar, long long per_sample, float d,
                                                       const float* __restrict__ pred, const float* __restrict__ target,
                                                       const float* __restrict__ sigma, const float* __restrict__ aw,
                                                       const float* __restrict__ fw, double* __restrict__ part, int* __restrict__ flags) {
  __shared__ double red[256];
  __shared__ int bad[256];
  const long long e0 = (long long)blockIdx.x * kWmseSlab;
  double s = 0.0;
  int nan = 0;
  for (int i = 0; i < kWmseSlab / 256; ++i) {
    const long long e = e0 + i * 256 + threadIdx.x;
    if (e >= n) break;
    const float r = __fsub_rn(pred[e], target[e]), sq = __fmul_rn(r, r);
    nan |= (sq != sq);
    int b;
    const float w = wmse_weight(e, nlat, nvar, per_sample, aw, fw, &b);
    s += (double)__fmul_rn(sq, w) * (double)wmse_lambda(sigma[b], d);
  }
  red[threadIdx.x] = s;
  bad[threadIdx.x] = nan;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      red[threadIdx.x] += red[threadIdx.x + w];
      bad[threadIdx.x] |= bad[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[blockIdx.x] = red[0];
    flags[blockIdx.x] = bad[0];
  }
}

// one workgroup
__global__ __launch_bounds__(256) void wmse_final_kernel(long long slabs, long long n, const double* __restrict__ part,
                                                         const int* __restrict__ flags, float* __restrict__ loss, int* __restrict__ nan_flag) {
  __shared__ double red[256];
  __shared__ int bad[256];
  double s = 0.0;
  int nan = 0;
  for (long long i = threadIdx.x; i < slabs; i += 256) {
    s += part[i];
    nan |= flags[i];
  }
  red[threadIdx.x] = s;
  bad[threadIdx.x] = nan;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      red[threadIdx.x] += red[threadIdx.x + w];
      bad[threadIdx.x] |= bad[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *loss = (float)(red[0] / (double)n);
    *nan_flag = bad[0];
  }
}

__global__ __launch_bounds__(256) void wmse_bwd_kernel(long long n, int nlat, int nvar, long long per_sample, float d,
                                                       const float* __restrict__ pred, const float* __restrict__ target,
                                                       const float* __restrict__ sigma, const float* __restrict__ aw,
                                                       const float* __restrict__ fw, const float* __restrict__ dloss,
                                                       float* __restrict__ dpred) {
  const float g = (float)(2.0 * (double)*dloss / (double)n);
  const long long stride = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
    int b;
    const float w = wmse_weight(e, nlat, nvar, per_sample, aw, fw, &b);
    dpred[e] = __fmul_rn(__fmul_rn(g, __fsub_rn(pred[e], target[e])), __fmul_rn(w, wmse_lambda(sigma[b], d)));
  }
}

bool wmse_ok(int32_t batch, int32_t nlon, int32_t nlat, int32_t nvar, float sigma_data) {
  return batch >= 1 && nlon >= 1 && nlat >= 1 && nvar >= 1 && sigma_data > 0.f;
}

long long wmse_count(int32_t batch, int32_t nlon, int32_t nlat, int32_t nvar) { return (long long)batch * nlon * nlat * nvar; }

size_t wmse_bytes(long long n) { return (size_t)((n + kWmseSlab - 1) / kWmseSlab) * (sizeof(double) + sizeof(int)); }

}  // namespace

extern "C" {

int gw_gencast_sampler_combine(int64_t n, float a, const float* x, float b, const float* y, float c, const float* z, float* out,
                               void* stream) {
  if (n < 0 || !out || (!x && !y && !z)) return failf(GW_E_BADARG, "gw_gencast_sampler_combine: bad arguments");
  if (n == 0) return GW_OK;
  const uintptr_t bits = (uintptr_t)out | (uintptr_t)x | (uintptr_t)y | (uintptr_t)z;  // (a null operand adds no bits)
  const long long n4 = (bits & 15) ? 0 : n / 4;
  hipLaunchKernelGGL(combine_kernel, dim3(grid_for(n4 ? n4 : n)), dim3(256), 0, (hipStream_t)stream, (long long)n, n4, a, b, c, x, y, z,
                     out);
  return check_launch("combine_kernel launch");
}

size_t gw_gencast_weighted_mse_workspace_bytes(int32_t batch, int32_t nlon, int32_t nlat, int32_t nvar) {
  if (!wmse_ok(batch, nlon, nlat, nvar, 1.f)) {
    failf(GW_E_BADARG, "gw_gencast_weighted_mse_workspace_bytes: bad arguments");
    return 0;
  }
  return wmse_bytes(wmse_count(batch, nlon, nlat, nvar));
}

int gw_gencast_weighted_mse_forward(int32_t batch, int32_t nlon, int32_t nlat, int32_t nvar, float sigma_data, const float* pred,
                                    const float* target, const float* sigma, const float* area_weights, const float* features_weights,
                                    void* workspace, size_t workspace_bytes, float* loss, int32_t* nan_flag, void* stream) {
  if (!wmse_ok(batch, nlon, nlat, nvar, sigma_data) || !pred || !target || !sigma || !loss || !nan_flag)
    return failf(GW_E_BADARG, "gw_gencast_weighted_mse_forward: bad arguments");
  const long long n = wmse_count(batch, nlon, nlat, nvar), slabs = (n + kWmseSlab - 1) / kWmseSlab;
  if (slabs > INT32_MAX) return failf(GW_E_UNSUPPORTED, "gw_gencast_weighted_mse_forward: shape too large");
  if (!workspace || workspace_bytes < wmse_bytes(n)) return failf(GW_E_BADARG, "gw_gencast_weighted_mse_forward: bad arguments (workspace)");
  double* part = (double*)workspace;
  int* flags = (int*)(part + slabs);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wmse_fwd_kernel, dim3((unsigned)slabs), dim3(256), 0, st, n, (int)nlat, (int)nvar, n / batch, sigma_data, pred, target,
                     sigma, area_weights, features_weights, part, flags);
  if (int rc = check_launch("wmse_fwd_kernel launch")) return rc;
  hipLaunchKernelGGL(wmse_final_kernel, dim3(1), dim3(256), 0, st, slabs, n, (const double*)part, (const int*)flags, loss, (int*)nan_flag);
  return check_launch("wmse_final_kernel launch");
}

int gw_gencast_weighted_mse_backward(int32_t batch, int32_t nlon, int32_t nlat, int32_t nvar, float sigma_data, const float* pred,
                                     const float* target, const float* sigma, const float* area_weights, const float* features_weights,
                                     const float* dloss, float* dpred, void* stream) {
  if (!wmse_ok(batch, nlon, nlat, nvar, sigma_data) || !pred || !target || !sigma || !dloss || !dpred)
    return failf(GW_E_BADARG, "gw_gencast_weighted_mse_backward: bad arguments");
  const long long n = wmse_count(batch, nlon, nlat, nvar);
  hipLaunchKernelGGL(wmse_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, n, (int)nlat, (int)nvar, n / batch, sigma_data,
                     pred, target, sigma, area_weights, features_weights, dloss, dpred);
  return check_launch("wmse_bwd_kernel launch");
}

}  // extern "C"
