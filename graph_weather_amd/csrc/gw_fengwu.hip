// gw_fengwu.hip - the kernels of the FengWu-GHR models (graph_weather/models/fengwu_ghr/layers.py) that the wide path
// (gw_wide.hip: Linear, LayerNorm, add) does not have:
//
//   gw_attention_forward    out = softmax(scale . Q K^T) V per (batch, head), flash style: online softmax, the N x N scores are
//                           never written; Q, K, V are read in place from the [rows, 3 . heads . dim_head] output of to_qkv and the
//                           result is written in the "b n (h d)" order to_out consumes; the per-row log-sum-exp is kept (in two parts:
//                           the row maximum and log sum exp(s - max) - one fp32 of their sum would round every recomputed
//                           probability by 4e-6 at scores of 100)
//   gw_attention_backward   recomputes P from Q, K and the log-sum-exp; delta = rowsum(dO o O) by a prologue, then one launch over
//                           key blocks (dK, dV resident across the query sweep) and one over query blocks (dQ): no atomics, no
//                           hand-off between workgroups, bitwise reproducible
//   gw_attention_axial_forward / _backward   the same kernels on sequences that lie along one axis of a token grid (CaFA,
//                           graph_weather/models/cafa/factorize.py): a sequence is (outer o, inner s) and its token i starts at
//                           x + o st[0] + s st[1] + i st[2] (64-bit strides), so attention along the height of [B, H, W, 3 inner]
//                           rows needs no transposing copy; the two entry points above are inner = 1, st = (n ld, 0, ld)
//   gw_knn_interpolate_forward / _backward   inverse-squared-distance interpolation over k = 4 neighbours through strides
//   gw_gelu_forward / _backward              exact (erf) GELU
//
// Attention products run on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate; gfx950 has no xf32).  One wave owns 16
// "stationary" rows (queries in the forward and the dQ launch, keys in the dK / dV launch) whose fragments stay in registers with
// the row on the MFMA lane (column index of the B operand); the "streamed" rows (keys, or queries) pass through LDS in tiles.
// Every score tile is computed TRANSPOSED - S^T[streamed][stationary] = X_streamed . X_stationary^T - so that
//   * a lane holds values of ONE stationary row: the softmax row maximum and sum are 16 register operations and two shuffles
//     over the four lane groups, never a serial walk over lanes;
//   * the accumulator tile (lane = stationary row, registers = streamed rows 16 t + 4 (lane >> 4) + r) IS the B operand of the
//     product that follows (O^T += V^T P^T, dQ^T += K^T dS^T, dV^T += dO^T P, dK^T += Q^T dS): K-step (t, r) takes register
//     p[t][r] as it lies, and the A operand is read from the LDS tile at the matching streamed row.  Nothing crosses lanes.
// Two launch forms of every attention kernel:
//   tile    a workgroup = 4 waves = 64 stationary rows of one (batch, head) pair, sharing the streamed tiles (64 rows, 32 at
//           dim_head > 64) - the long-sequence regime (4 050 tokens x 8 pairs: 512 workgroups)
//   packed  N <= 16 (the wrappers' window attention, N = s_h . s_w): every WAVE is one pair with its own 16-row LDS slice, four
//           pairs per workgroup, one pass, instead of a 64-row tile for 9 rows
// dim_head is zero padded to DP in {16, 32, 64, 128} (the K dimension of S and the row count of the second products).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/gw_amd.h"
#include "gw_device.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

int failf(int code, const char* msg) { return set_error(code, msg); }

struct AttnArgs {
  int batch, heads, n, d;
  int64_t pairs;
  int inner;  // batch = outer * inner sequences; pair = ((o, s), h) with s the fast sequence index
  const float *q, *k, *v;
  // token i of head h of sequence (o, s) starts at x + o st[0] + s st[1] + i st[2] + h d (strides in floats); the plain
  // [batch n, ld] rows are inner = 1, st = (n ld, 0, ld)
  int64_t sq[3];  // q, k, v
  float scale;
  float* out;  // forward: written; backward: the forward's output
  int64_t so[3];
  float* lse;  // [2, pairs, n]: the row maximum m of the scaled scores, then log sum exp(s - m) - the log-sum-exp in two parts
  const float* dout;
  int64_t sg[3];
  float* delta;  // [pairs, n]
  float *dq, *dk, *dv;
  int64_t sd[3];  // dq, dk, dv
  int vec;  // every pointer 16-byte aligned, every stride and dim_head a multiple of 4
  const float* bias;  // MASKED kernels: [batch, n] added to the scaled scores of every head and query of a sequence, 0 or -inf per key
};

template <int DP>
struct Cfg {
  static constexpr int LD = DP + 4;  // LDS row stride: 16-byte aligned rows; the four lane groups of a b32 column read land 16 banks apart
  static constexpr int NC = DP / 16;
  static constexpr int TB = DP > 64 ? 32 : 64;  // streamed rows per tile (tile form)
  static constexpr int PW = DP > 64 ? 2 : 4;    // waves (= pairs) per workgroup of the packed form: two 16-row slices per wave fit 64 KiB
};

__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// four consecutive features d0 .. d0 + 3 of a row (NULL row or features past D: zeros)
__device__ __forceinline__ f32x4 load4(const float* row, int d0, int D, bool vec) {
  if (row == nullptr || d0 >= D) return zero4();
  if (vec) return ldg4(row + d0);
  f32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = d0 + j < D ? ldg1(row + d0 + j) : 0.f;
  return r;
}

__device__ __forceinline__ void store4(float* row, int d0, int D, bool vec, f32x4 v) {
  if (d0 >= D) return;
  if (vec) {
    stg4(row + d0, v);
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (d0 + j < D) stg1(row + d0 + j, v[j]);
}

// rows r0 .. r0 + ROWS - 1 of one pair (base = its row 0, or NULL) into an LDS tile, zero filled past n and past D
template <int DP, int ROWS>
__device__ __forceinline__ void stage_rows(float* lds, const float* base, int64_t ld, int r0, int n, int D, bool vec, int tid, int nthreads) {
  constexpr int C4 = DP / 4, LD = Cfg<DP>::LD;
  for (int idx = tid; idx < ROWS * C4; idx += nthreads) {
    const int row = idx / C4, c4 = idx - row * C4;
    const float* rp = (base != nullptr && r0 + row < n) ? base + (int64_t)(r0 + row) * ld : nullptr;
    *(f32x4*)(lds + row * LD + 4 * c4) = load4(rp, 4 * c4, D, vec);
  }
}

// acc[t][r] += sum_d tile[16 t + 4 kq + r][d] * frag_row(i)[d]   (S^T: streamed row in the registers, stationary row on the lane).
// The d a lane feeds into K-step (c, ks) is 16 c + 4 kq + ks for both operands: the tile side is one ds_read_b128.
template <int DP, int NT>
__device__ __forceinline__ void prod_rows(f32x4 (&acc)[NT], const float* tile, const f32x4 (&frag)[DP / 16], int i, int kq) {
  constexpr int LD = Cfg<DP>::LD;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int c = 0; c < DP / 16; ++c) {
      const f32x4 a4 = *(const f32x4*)(tile + (16 * t + i) * LD + 16 * c + 4 * kq);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[ks], frag[c][ks], acc[t], 0, 0, 0);
    }
  }
}

// out[dt][r'] += sum over the tile's rows of tile[row][16 dt + 4 kq + r'] * p(row, lane's stationary row), p[t][r] holding row
// 16 t + 4 kq + r as prod_rows left it: K-step (t, r) reads the A operand at exactly that row.
template <int DP, int NT>
__device__ __forceinline__ void prod_acc(f32x4 (&out)[DP / 16], const float* tile, const f32x4 (&p)[NT], int i, int kq) {
  constexpr int LD = Cfg<DP>::LD;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* row = tile + (16 * t + 4 * kq + r) * LD + i;
#pragma unroll
      for (int dt = 0; dt < DP / 16; ++dt) out[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[16 * dt], p[t][r], out[dt], 0, 0, 0);
    }
  }
}

// The scaled score as ONE rounded product.  Written s * scale, the compiler contracts the subtraction of the row maximum that
// follows into fma(s, scale, -max): the unrounded product minus a maximum that IS a rounded product leaves the rounding residual
// (half an ulp of the score: 4e-6 at scores of 100) in the exponent of the very keys that dominate the row, in the forward and -
// without a normalisation to cancel it - in every probability the backward recomputes.
// (HIP's __fmul_rn is a plain product and contracts as well; the empty asm statement makes the rounded product a value the
// compiler cannot look through.)
__device__ __forceinline__ float scaled(float s, float scale) {
  float r = s * scale;
  asm("" : "+v"(r));
  return r;
}

__device__ __forceinline__ float group_max(float v) {  // over the four lane groups that share lane & 15
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// which pair and which 16 stationary rows this wave owns
struct Place {
  int64_t pair;
  int row0;
  bool ok;        // the pair exists
  int o, s;       // its sequence
  int h;
  int64_t seq;    // o * inner + s: the row of the key bias
  // offset in floats of token 0 of the sequence in an operand with strides st; the head offset h d is added by the caller
  __device__ __forceinline__ int64_t at(const int64_t (&st)[3]) const { return o * st[0] + s * st[1]; }
};
template <bool PACKED, int PW>
__device__ __forceinline__ Place place_of(const AttnArgs& a, int wave) {
  Place p;
  if (PACKED) {
    p.pair = (int64_t)blockIdx.x * PW + wave;
    p.row0 = 0;
  } else {
    const int nt = (a.n + 63) / 64;
    p.pair = (int64_t)(blockIdx.x / nt);
    p.row0 = (int)(blockIdx.x % nt) * 64 + 16 * wave;
  }
  p.ok = p.pair < a.pairs;
  const int64_t pr = p.ok ? p.pair : 0;
  const int64_t b = pr / a.heads;
  p.h = (int)(pr - b * a.heads);
  p.o = (int)(b / a.inner);
  p.s = (int)(b - (int64_t)p.o * a.inner);
  p.seq = b;
  return p;
}

// ---- forward -----------------------------------------------------------------------------------------------------------
template <int DP, bool PACKED, bool MASKED>
__device__ __forceinline__ void attn_fwd_body(const AttnArgs& a) {
  constexpr int LD = Cfg<DP>::LD, NC = Cfg<DP>::NC, TB = PACKED ? 16 : Cfg<DP>::TB, NT = TB / 16;
  constexpr int LROWS = PACKED ? 16 * Cfg<DP>::PW : TB;
  __shared__ __attribute__((aligned(16))) float Ks[LROWS * LD];
  __shared__ __attribute__((aligned(16))) float Vs[LROWS * LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  const Place pl = place_of<PACKED, Cfg<DP>::PW>(a, wave);
  const bool vec = a.vec != 0;
  const int D = a.d, n = a.n;
  const size_t col = (size_t)pl.h * D;
  const int qrow = pl.row0 + i;
  const bool qok = pl.ok && qrow < n;
  const int64_t bq = pl.at(a.sq), tq = a.sq[2];
  const float* qp = qok ? a.q + bq + qrow * tq + col : nullptr;
  f32x4 qf[NC], o[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    qf[c] = load4(qp, 16 * c + 4 * kq, D, vec);
    o[c] = zero4();
  }
  float m = -INFINITY, l = 0.f;
  const float* kbase = pl.ok ? a.k + bq + col : nullptr;
  const float* vbase = pl.ok ? a.v + bq + col : nullptr;
  float* ks = PACKED ? Ks + wave * 16 * LD : Ks;
  float* vs = PACKED ? Vs + wave * 16 * LD : Vs;
  for (int k0 = 0; k0 < n; k0 += TB) {
    __syncthreads();
    if (PACKED) {
      stage_rows<DP, 16>(ks, kbase, tq, k0, n, D, vec, lane, 64);
      stage_rows<DP, 16>(vs, vbase, tq, k0, n, D, vec, lane, 64);
    } else {
      stage_rows<DP, TB>(ks, kbase, tq, k0, n, D, vec, threadIdx.x, 256);
      stage_rows<DP, TB>(vs, vbase, tq, k0, n, D, vec, threadIdx.x, 256);
    }
    __syncthreads();
    f32x4 s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) s[t] = zero4();
    prod_rows<DP, NT>(s, ks, qf, i, kq);
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sc = scaled(s[t][r], a.scale);
        const int key = k0 + 16 * t + 4 * kq + r;
        float v = (key < n) ? sc : -INFINITY;  // the ragged tail of the keys
        if constexpr (MASKED) {
          if (key < n && pl.ok) v += ldg1(a.bias + pl.seq * n + key);  // 0 or -inf
        }
        s[t][r] = v;
        mx = fmaxf(mx, v);
      }
    float m_new = fmaxf(m, group_max(mx));  // finite: key k0 is valid
    float m_ref = m_new;                    // what the exponents are taken against
    if constexpr (MASKED) {
      // every key so far masked: the maximum is still -inf, and -inf - -inf is NaN.  Against 0 every p and alpha are exp(-inf) = 0
      // and the running state stays (m, l, o) = (-inf, 0, 0) until the first kept key arrives.
      if (m_new == -INFINITY) m_ref = 0.f;
    }
    const float alpha = expf(m - m_ref);          // 0 on the first tile (m = -inf)
    float rs = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = expf(s[t][r] - m_ref);
        s[t][r] = p;
        rs += p;
      }
    l = l * alpha + rs;  // this lane's share of the row sum (alpha is the same in the four lane groups)
    m = m_new;
#pragma unroll
    for (int c = 0; c < NC; ++c) o[c] *= alpha;
    prod_acc<DP, NT>(o, vs, s, i, kq);
  }
  l = group_sum(l);
  if (qok) {
    const float inv = 1.0f / l;
    float* op = a.out + pl.at(a.so) + qrow * a.so[2] + col;
#pragma unroll
    for (int c = 0; c < NC; ++c) store4(op, 16 * c + 4 * kq, D, vec, o[c] * inv);
    if (kq == 0) {
      stg1(a.lse + (size_t)pl.pair * n + qrow, m);
      stg1(a.lse + (size_t)(a.pairs + pl.pair) * n + qrow, logf(l));
    }
  }
}

// ---- backward prologue: delta[pair, i] = sum_d dO[i, d] O[i, d] ----------------------------------------------------------
__global__ __launch_bounds__(256) void attn_delta_kernel(const AttnArgs a) {
  const int64_t total = a.pairs * a.n;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t pair = t / a.n;
    const int i = (int)(t - pair * a.n);
    const int64_t b = pair / a.heads;
    const int h = (int)(pair - b * a.heads);
    const int64_t o = b / a.inner, sq = b - o * a.inner;
    const float* op = a.out + o * a.so[0] + sq * a.so[1] + i * a.so[2] + (size_t)h * a.d;
    const float* gp = a.dout + o * a.sg[0] + sq * a.sg[1] + i * a.sg[2] + (size_t)h * a.d;
    // one fmaf chain in the order the MFMAs of dP = dO . V^T walk the features (chunk c, K-step ks, lane group kq: d = 16 c + 4 kq +
    // ks): delta and dP then round alike, and with a single key (O = V, p = 1) dS = p (dP - delta) is exactly zero
    // (an fp32-input MFMA accumulates as a k-ordered fmaf chain; should that ever change, the single-key case shows one rounding
    // instead of an exact zero and nothing else is affected)
    float s = 0.f;
    for (int c = 0; c < a.d; c += 16)
      for (int ks = 0; ks < 4; ++ks)
        for (int kq = 0; kq < 4; ++kq) {
          const int d = c + 4 * kq + ks;
          if (d < a.d) s = fmaf(ldg1(gp + d), ldg1(op + d), s);
        }
    stg1(a.delta + t, s);
  }
}

// ---- dQ: queries stationary, keys streamed ----------------------------------------------------------------------------------
template <int DP, bool PACKED, bool MASKED>
__device__ __forceinline__ void attn_dq_body(const AttnArgs& a) {
  constexpr int LD = Cfg<DP>::LD, NC = Cfg<DP>::NC, TB = PACKED ? 16 : Cfg<DP>::TB, NT = TB / 16;
  constexpr int LROWS = PACKED ? 16 * Cfg<DP>::PW : TB;
  __shared__ __attribute__((aligned(16))) float Ks[LROWS * LD];
  __shared__ __attribute__((aligned(16))) float Vs[LROWS * LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  const Place pl = place_of<PACKED, Cfg<DP>::PW>(a, wave);
  const bool vec = a.vec != 0;
  const int D = a.d, n = a.n;
  const size_t col = (size_t)pl.h * D;
  const int qrow = pl.row0 + i;
  const bool qok = pl.ok && qrow < n;
  const int64_t bq = pl.at(a.sq), tq = a.sq[2];
  const float* qp = qok ? a.q + bq + qrow * tq + col : nullptr;
  const float* gp = qok ? a.dout + pl.at(a.sg) + qrow * a.sg[2] + col : nullptr;
  f32x4 qf[NC], gf[NC], dq[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    qf[c] = load4(qp, 16 * c + 4 * kq, D, vec);
    gf[c] = load4(gp, 16 * c + 4 * kq, D, vec);
    dq[c] = zero4();
  }
  // rows past the end: m = +inf makes every p zero
  const float mrow = qok ? ldg1(a.lse + (size_t)pl.pair * n + qrow) : INFINITY;
  const float lrow = qok ? ldg1(a.lse + (size_t)(a.pairs + pl.pair) * n + qrow) : 0.f;
  const float delta = qok ? ldg1(a.delta + (size_t)pl.pair * n + qrow) : 0.f;
  const float* kbase = pl.ok ? a.k + bq + col : nullptr;
  const float* vbase = pl.ok ? a.v + bq + col : nullptr;
  float* ks = PACKED ? Ks + wave * 16 * LD : Ks;
  float* vs = PACKED ? Vs + wave * 16 * LD : Vs;
  for (int k0 = 0; k0 < n; k0 += TB) {
    __syncthreads();
    if (PACKED) {
      stage_rows<DP, 16>(ks, kbase, tq, k0, n, D, vec, lane, 64);
      stage_rows<DP, 16>(vs, vbase, tq, k0, n, D, vec, lane, 64);
    } else {
      stage_rows<DP, TB>(ks, kbase, tq, k0, n, D, vec, threadIdx.x, 256);
      stage_rows<DP, TB>(vs, vbase, tq, k0, n, D, vec, threadIdx.x, 256);
    }
    __syncthreads();
    f32x4 s[NT], dp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      s[t] = zero4();
      dp[t] = zero4();
    }
    prod_rows<DP, NT>(s, ks, qf, i, kq);
    prod_rows<DP, NT>(dp, vs, gf, i, kq);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + 16 * t + 4 * kq + r;
        const bool kok = key < n;
        float sc = scaled(s[t][r], a.scale);
        if constexpr (MASKED) {
          if (kok && pl.ok) sc += ldg1(a.bias + pl.seq * n + key);  // -inf: p = exp(-inf) = 0
        }
        const float p = kok ? expf((sc - mrow) - lrow) : 0.f;
        s[t][r] = p * (dp[t][r] - delta) * a.scale;  // dS
      }
    prod_acc<DP, NT>(dq, ks, s, i, kq);
  }
  if (qok) {
    float* op = a.dq + pl.at(a.sd) + qrow * a.sd[2] + col;
#pragma unroll
    for (int c = 0; c < NC; ++c) store4(op, 16 * c + 4 * kq, D, vec, dq[c]);
  }
}

// ---- dK, dV: keys stationary (accumulators resident), queries streamed ------------------------------------------------------------
template <int DP, bool PACKED, bool MASKED>
__device__ __forceinline__ void attn_dkv_body(const AttnArgs& a) {
  constexpr int LD = Cfg<DP>::LD, NC = Cfg<DP>::NC, TB = PACKED ? 16 : Cfg<DP>::TB, NT = TB / 16;
  constexpr int LROWS = PACKED ? 16 * Cfg<DP>::PW : TB;
  __shared__ __attribute__((aligned(16))) float Qs[LROWS * LD];
  __shared__ __attribute__((aligned(16))) float Gs[LROWS * LD];
  __shared__ __attribute__((aligned(16))) float Ms[LROWS];
  __shared__ __attribute__((aligned(16))) float Ls[LROWS];
  __shared__ __attribute__((aligned(16))) float Ds[LROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  const Place pl = place_of<PACKED, Cfg<DP>::PW>(a, wave);
  const bool vec = a.vec != 0;
  const int D = a.d, n = a.n;
  const size_t col = (size_t)pl.h * D;
  const int krow = pl.row0 + i;
  const bool kok = pl.ok && krow < n;
  const int64_t bq = pl.at(a.sq), tq = a.sq[2], tg = a.sg[2];
  const float* kp = kok ? a.k + bq + krow * tq + col : nullptr;
  const float* vp = kok ? a.v + bq + krow * tq + col : nullptr;
  f32x4 kf[NC], vf[NC], dk[NC], dv[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    kf[c] = load4(kp, 16 * c + 4 * kq, D, vec);
    vf[c] = load4(vp, 16 * c + 4 * kq, D, vec);
    dk[c] = zero4();
    dv[c] = zero4();
  }
  const float* qbase = pl.ok ? a.q + bq + col : nullptr;
  const float* gbase = pl.ok ? a.dout + pl.at(a.sg) + col : nullptr;
  float kbias = 0.f;  // of this lane's key: -inf makes its p, and with it dK and dV, exactly zero
  if constexpr (MASKED) {
    if (kok) kbias = ldg1(a.bias + pl.seq * n + krow);
  }
  const int off = PACKED ? wave * 16 : 0;
  float* qs = Qs + off * LD;
  float* gs = Gs + off * LD;
  float* ms = Ms + off;
  float* ls = Ls + off;
  float* ds = Ds + off;
  for (int q0 = 0; q0 < n; q0 += TB) {
    __syncthreads();
    if (PACKED) {
      stage_rows<DP, 16>(qs, qbase, tq, q0, n, D, vec, lane, 64);
      stage_rows<DP, 16>(gs, gbase, tg, q0, n, D, vec, lane, 64);
      if (lane < 16) {
        const bool ok = pl.ok && q0 + lane < n;
        ms[lane] = ok ? ldg1(a.lse + (size_t)pl.pair * n + q0 + lane) : INFINITY;  // rows past the end: p = 0
        ls[lane] = ok ? ldg1(a.lse + (size_t)(a.pairs + pl.pair) * n + q0 + lane) : 0.f;
        ds[lane] = ok ? ldg1(a.delta + (size_t)pl.pair * n + q0 + lane) : 0.f;
      }
    } else {
      stage_rows<DP, TB>(qs, qbase, tq, q0, n, D, vec, threadIdx.x, 256);
      stage_rows<DP, TB>(gs, gbase, tg, q0, n, D, vec, threadIdx.x, 256);
      if ((int)threadIdx.x < TB) {
        const bool ok = pl.ok && q0 + (int)threadIdx.x < n;
        ms[threadIdx.x] = ok ? ldg1(a.lse + (size_t)pl.pair * n + q0 + threadIdx.x) : INFINITY;
        ls[threadIdx.x] = ok ? ldg1(a.lse + (size_t)(a.pairs + pl.pair) * n + q0 + threadIdx.x) : 0.f;
        ds[threadIdx.x] = ok ? ldg1(a.delta + (size_t)pl.pair * n + q0 + threadIdx.x) : 0.f;
      }
    }
    __syncthreads();
    f32x4 s[NT], dp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      s[t] = zero4();
      dp[t] = zero4();
    }
    prod_rows<DP, NT>(s, qs, kf, i, kq);   // S[query][key i]
    prod_rows<DP, NT>(dp, gs, vf, i, kq);  // dP[query][key i]
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const f32x4 m4 = *(const f32x4*)(ms + 16 * t + 4 * kq);
      const f32x4 l4 = *(const f32x4*)(ls + 16 * t + 4 * kq);
      const f32x4 d4 = *(const f32x4*)(ds + 16 * t + 4 * kq);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sc = scaled(s[t][r], a.scale);
        if constexpr (MASKED) sc += kbias;
        const float p = kok ? expf((sc - m4[r]) - l4[r]) : 0.f;
        s[t][r] = p;
        dp[t][r] = p * (dp[t][r] - d4[r]) * a.scale;  // dS
      }
    }
    prod_acc<DP, NT>(dv, gs, s, i, kq);
    prod_acc<DP, NT>(dk, qs, dp, i, kq);
  }
  if (kok) {
    const int64_t bd = pl.at(a.sd) + krow * a.sd[2] + col;
    float* okp = a.dk + bd;
    float* ovp = a.dv + bd;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      store4(okp, 16 * c + 4 * kq, D, vec, dk[c]);
      store4(ovp, 16 * c + 4 * kq, D, vec, dv[c]);
    }
  }
}

// The kernels proper: the unmasked ones keep their names and template signature <DP, PACKED>; the MASKED ones (a key bias, see
// AttnArgs::bias) are kernels of their own.
template <int DP, bool PACKED>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const AttnArgs a) { attn_fwd_body<DP, PACKED, false>(a); }
template <int DP, bool PACKED>
__global__ __launch_bounds__(256) void attn_dq_kernel(const AttnArgs a) { attn_dq_body<DP, PACKED, false>(a); }
template <int DP, bool PACKED>
__global__ __launch_bounds__(256) void attn_dkv_kernel(const AttnArgs a) { attn_dkv_body<DP, PACKED, false>(a); }
template <int DP, bool PACKED>
__global__ __launch_bounds__(256) void attn_fwd_masked_kernel(const AttnArgs a) { attn_fwd_body<DP, PACKED, true>(a); }
template <int DP, bool PACKED>
__global__ __launch_bounds__(256) void attn_dq_masked_kernel(const AttnArgs a) { attn_dq_body<DP, PACKED, true>(a); }
template <int DP, bool PACKED>
__global__ __launch_bounds__(256) void attn_dkv_masked_kernel(const AttnArgs a) { attn_dkv_body<DP, PACKED, true>(a); }

template <typename F>
int by_dim_head(int d, F f) {
  if (d <= 16) return f(std::integral_constant<int, 16>{});
  if (d <= 32) return f(std::integral_constant<int, 32>{});
  if (d <= 64) return f(std::integral_constant<int, 64>{});
  return f(std::integral_constant<int, 128>{});
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int attn_check(const char* what, int32_t batch, int32_t heads, int32_t n, int32_t d, int64_t ld_min, int32_t ld) {
  static char msg[160];
  if (batch <= 0 || heads <= 0 || n <= 0 || d <= 0 || ld < ld_min) {
    snprintf(msg, sizeof msg, "%s: bad arguments", what);
    return failf(GW_E_BADARG, msg);
  }
  if (d > 128) {
    snprintf(msg, sizeof msg, "%s: dim_head above 128 is not implemented", what);
    return failf(GW_E_UNSUPPORTED, msg);
  }
  if ((int64_t)batch * n >= ((int64_t)1 << 31) || (int64_t)batch * heads >= ((int64_t)1 << 31)) {
    snprintf(msg, sizeof msg, "%s: row count exceeds int32", what);
    return failf(GW_E_UNSUPPORTED, msg);
  }
  return GW_OK;
}

// workgroups of the tile / packed form
unsigned attn_grid(const AttnArgs& a, bool packed) {
  const int pw = a.d > 64 ? 2 : 4;  // Cfg<DP>::PW
  if (packed) return (unsigned)((a.pairs + pw - 1) / pw);
  return (unsigned)(a.pairs * ((a.n + 63) / 64));
}

// ---- knn_interpolate ---------------------------------------------------------------------------------------------------------
// y[b, t, c] = sum_k w[t, k] x[b, idx[t, k], c] / sum_k w[t, k]; element (b, r, c) of a tensor lies at b sb + r sr + c sc.
__global__ __launch_bounds__(256) void knn_fwd_kernel(int batch, int n_tgt, int channels, int k, const int* __restrict__ idx,
                                                      const float* __restrict__ w, const float* __restrict__ x, int64_t xsb, int64_t xsr,
                                                      int64_t xsc, float* __restrict__ y, int64_t ysb, int64_t ysr, int64_t ysc, int c_fast) {
  const int64_t total = (int64_t)batch * n_tgt * channels;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    int b, t, c;
    if (c_fast) {
      c = (int)(e % channels);
      t = (int)((e / channels) % n_tgt);
      b = (int)(e / ((int64_t)channels * n_tgt));
    } else {
      t = (int)(e % n_tgt);
      c = (int)((e / n_tgt) % channels);
      b = (int)(e / ((int64_t)channels * n_tgt));
    }
    const float* xb = x + b * xsb + c * xsc;
    float num = 0.f, den = 0.f;
    for (int j = 0; j < k; ++j) {
      const float wj = ldg1(w + (size_t)t * k + j);
      num = fmaf(wj, ldg1(xb + (int64_t)ldgi(idx + (size_t)t * k + j) * xsr), num);
      den += wj;
    }
    stg1(y + b * ysb + t * ysr + c * ysc, num / den);
  }
}

// dx[b, s, c] = sum over the CSR row of source s (entries e: target tgt[e], weight cw[e] = w / den of that target) cw[e] dy[b, tgt[e], c]
__global__ __launch_bounds__(256) void knn_bwd_kernel(int batch, int n_src, int channels, const int* __restrict__ ptr,
                                                      const int* __restrict__ tgt, const float* __restrict__ cw, const float* __restrict__ dy,
                                                      int64_t ysb, int64_t ysr, int64_t ysc, float* __restrict__ dx, int64_t xsb, int64_t xsr,
                                                      int64_t xsc, int c_fast) {
  const int64_t total = (int64_t)batch * n_src * channels;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    int b, s, c;
    if (c_fast) {
      c = (int)(e % channels);
      s = (int)((e / channels) % n_src);
      b = (int)(e / ((int64_t)channels * n_src));
    } else {
      s = (int)(e % n_src);
      c = (int)((e / n_src) % channels);
      b = (int)(e / ((int64_t)channels * n_src));
    }
    const float* gb = dy + b * ysb + c * ysc;
    float acc = 0.f;
    for (int j = ldgi(ptr + s), j1 = ldgi(ptr + s + 1); j < j1; ++j) acc = fmaf(ldg1(cw + j), ldg1(gb + (int64_t)ldgi(tgt + j) * ysr), acc);
    stg1(dx + b * xsb + s * xsr + c * xsc, acc);
  }
}

// ---- exact GELU ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gelu_fwd_kernel(int64_t n, const float* __restrict__ x, float* __restrict__ y) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const float v = ldg1(x + e);
    stg1(y + e, 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)));
  }
}
// d/dx [x Phi(x)] = Phi(x) + x phi(x)
__global__ __launch_bounds__(256) void gelu_bwd_kernel(int64_t n, const float* __restrict__ x, const float* __restrict__ dy,
                                                       float* __restrict__ dx) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const float v = ldg1(x + e);
    const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * expf(-0.5f * v * v);
    stg1(dx + e, ldg1(dy + e) * (cdf + v * pdf));
  }
}

unsigned stream_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

void set3(int64_t (&st)[3], const int64_t* from) { st[0] = from[0], st[1] = from[1], st[2] = from[2]; }
void rows3(int64_t (&st)[3], int32_t n, int32_t ld) { st[0] = (int64_t)n * ld, st[1] = 0, st[2] = ld; }
bool mult4(const int64_t (&st)[3]) { return st[0] % 4 == 0 && st[1] % 4 == 0 && st[2] % 4 == 0; }

// sizes of the axial entry points (the strides are the caller's statement of where the sequences lie)
int axial_args(AttnArgs& a, const char* what, int32_t outer, int32_t inner, int32_t heads, int32_t n, int32_t d) {
  static char msg[160];
  if (outer <= 0 || inner <= 0 || heads <= 0 || n <= 0 || d <= 0 || d > 128) {
    snprintf(msg, sizeof msg, "%s: bad arguments", what);
    return failf(GW_E_BADARG, msg);
  }
  const int64_t seqs = (int64_t)outer * inner;
  if (seqs * n >= ((int64_t)1 << 31) || seqs * heads >= ((int64_t)1 << 31)) {
    snprintf(msg, sizeof msg, "%s: row count exceeds int32", what);
    return failf(GW_E_UNSUPPORTED, msg);
  }
  a.batch = (int)seqs, a.inner = inner, a.heads = heads, a.n = n, a.d = d, a.pairs = seqs * heads;
  return GW_OK;
}

int attn_forward_launch(AttnArgs& a, void* stream) {
  a.vec = a.d % 4 == 0 && mult4(a.sq) && mult4(a.so) && al16(a.q) && al16(a.k) && al16(a.v) && al16(a.out);
  const bool packed = a.n <= 16;
  const dim3 grid(attn_grid(a, packed));
  by_dim_head(a.d, [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    if (a.bias != nullptr) {
      if (packed)
        hipLaunchKernelGGL((attn_fwd_masked_kernel<DP, true>), grid, dim3(64 * Cfg<DP>::PW), 0, (hipStream_t)stream, a);
      else
        hipLaunchKernelGGL((attn_fwd_masked_kernel<DP, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    } else if (packed)
      hipLaunchKernelGGL((attn_fwd_kernel<DP, true>), grid, dim3(64 * Cfg<DP>::PW), 0, (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL((attn_fwd_kernel<DP, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    return 0;
  });
  return check_launch("attn_fwd_kernel launch");
}

int attn_backward_launch(AttnArgs& a, void* stream) {
  a.vec = a.d % 4 == 0 && mult4(a.sq) && mult4(a.sg) && mult4(a.sd) && al16(a.q) && al16(a.k) && al16(a.v) && al16(a.dout) &&
          al16(a.dq) && al16(a.dk) && al16(a.dv);
  hipLaunchKernelGGL(attn_delta_kernel, dim3(stream_blocks(a.pairs * a.n)), dim3(256), 0, (hipStream_t)stream, a);
  int rc = check_launch("attn_delta_kernel launch");
  if (rc != GW_OK) return rc;
  const bool packed = a.n <= 16;
  const dim3 grid(attn_grid(a, packed));
  by_dim_head(a.d, [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    if (a.bias != nullptr) {
      if (packed) {
        hipLaunchKernelGGL((attn_dkv_masked_kernel<DP, true>), grid, dim3(64 * Cfg<DP>::PW), 0, (hipStream_t)stream, a);
        hipLaunchKernelGGL((attn_dq_masked_kernel<DP, true>), grid, dim3(64 * Cfg<DP>::PW), 0, (hipStream_t)stream, a);
      } else {
        hipLaunchKernelGGL((attn_dkv_masked_kernel<DP, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
        hipLaunchKernelGGL((attn_dq_masked_kernel<DP, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
      }
    } else if (packed) {
      hipLaunchKernelGGL((attn_dkv_kernel<DP, true>), grid, dim3(64 * Cfg<DP>::PW), 0, (hipStream_t)stream, a);
      hipLaunchKernelGGL((attn_dq_kernel<DP, true>), grid, dim3(64 * Cfg<DP>::PW), 0, (hipStream_t)stream, a);
    } else {
      hipLaunchKernelGGL((attn_dkv_kernel<DP, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
      hipLaunchKernelGGL((attn_dq_kernel<DP, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    }
    return 0;
  });
  return check_launch("attn_dkv_kernel / attn_dq_kernel launch");
}

}  // namespace

extern "C" {

int gw_attention_axial_forward(int32_t outer, int32_t inner, int32_t heads, int32_t n, int32_t dim_head, const float* q, const float* k,
                               const float* v, const int64_t* stride_qkv, float scale, float* out, const int64_t* stride_out, float* lse,
                               void* stream) {
  if (!q || !k || !v || !out || !lse || !stride_qkv || !stride_out) return failf(GW_E_BADARG, "gw_attention_axial_forward: bad arguments");
  AttnArgs a = {};
  int rc = axial_args(a, "gw_attention_axial_forward", outer, inner, heads, n, dim_head);
  if (rc != GW_OK) return rc;
  a.q = q, a.k = k, a.v = v, a.scale = scale, a.out = out, a.lse = lse;
  set3(a.sq, stride_qkv), set3(a.so, stride_out);
  return attn_forward_launch(a, stream);
}

int gw_attention_axial_backward(int32_t outer, int32_t inner, int32_t heads, int32_t n, int32_t dim_head, const float* q, const float* k,
                                const float* v, const int64_t* stride_qkv, float scale, const float* out, const int64_t* stride_out,
                                const float* dout, const int64_t* stride_dout, const float* lse, float* delta, float* dq, float* dk,
                                float* dv, const int64_t* stride_dqkv, void* stream) {
  if (!q || !k || !v || !out || !dout || !lse || !delta || !dq || !dk || !dv || !stride_qkv || !stride_out || !stride_dout || !stride_dqkv)
    return failf(GW_E_BADARG, "gw_attention_axial_backward: bad arguments");
  AttnArgs a = {};
  int rc = axial_args(a, "gw_attention_axial_backward", outer, inner, heads, n, dim_head);
  if (rc != GW_OK) return rc;
  a.q = q, a.k = k, a.v = v, a.scale = scale, a.out = const_cast<float*>(out), a.lse = const_cast<float*>(lse);
  a.dout = dout, a.delta = delta, a.dq = dq, a.dk = dk, a.dv = dv;
  set3(a.sq, stride_qkv), set3(a.so, stride_out), set3(a.sg, stride_dout), set3(a.sd, stride_dqkv);
  return attn_backward_launch(a, stream);
}

// the axial entry points with a key bias [outer * inner, n] (0 keeps a key, -inf drops it for every query and head of its sequence)
int gw_attention_masked_forward(int32_t outer, int32_t inner, int32_t heads, int32_t n, int32_t dim_head, const float* q, const float* k,
                                const float* v, const int64_t* stride_qkv, const float* key_bias, float scale, float* out,
                                const int64_t* stride_out, float* lse, void* stream) {
  if (!q || !k || !v || !out || !lse || !stride_qkv || !stride_out || !key_bias)
    return failf(GW_E_BADARG, "gw_attention_masked_forward: bad arguments");
  AttnArgs a = {};
  int rc = axial_args(a, "gw_attention_masked_forward", outer, inner, heads, n, dim_head);
  if (rc != GW_OK) return rc;
  a.q = q, a.k = k, a.v = v, a.scale = scale, a.out = out, a.lse = lse, a.bias = key_bias;
  set3(a.sq, stride_qkv), set3(a.so, stride_out);
  return attn_forward_launch(a, stream);
}

int gw_attention_masked_backward(int32_t outer, int32_t inner, int32_t heads, int32_t n, int32_t dim_head, const float* q, const float* k,
                                 const float* v, const int64_t* stride_qkv, const float* key_bias, float scale, const float* out,
                                 const int64_t* stride_out, const float* dout, const int64_t* stride_dout, const float* lse, float* delta,
                                 float* dq, float* dk, float* dv, const int64_t* stride_dqkv, void* stream) {
  if (!q || !k || !v || !out || !dout || !lse || !delta || !dq || !dk || !dv || !stride_qkv || !stride_out || !stride_dout || !stride_dqkv ||
      !key_bias)
    return failf(GW_E_BADARG, "gw_attention_masked_backward: bad arguments");
  AttnArgs a = {};
  int rc = axial_args(a, "gw_attention_masked_backward", outer, inner, heads, n, dim_head);
  if (rc != GW_OK) return rc;
  a.q = q, a.k = k, a.v = v, a.scale = scale, a.out = const_cast<float*>(out), a.lse = const_cast<float*>(lse), a.bias = key_bias;
  a.dout = dout, a.delta = delta, a.dq = dq, a.dk = dk, a.dv = dv;
  set3(a.sq, stride_qkv), set3(a.so, stride_out), set3(a.sg, stride_dout), set3(a.sd, stride_dqkv);
  return attn_backward_launch(a, stream);
}

// the plain [batch n, ld] rows: one sequence per outer index
int gw_attention_forward(int32_t batch, int32_t heads, int32_t n, int32_t dim_head, const float* q, const float* k, const float* v,
                         int32_t ld_qkv, float scale, float* out, int32_t ld_out, float* lse, void* stream) {
  if (!q || !k || !v || !out || !lse) return failf(GW_E_BADARG, "gw_attention_forward: bad arguments");
  int rc = attn_check("gw_attention_forward", batch, heads, n, dim_head, (int64_t)heads * dim_head, ld_qkv);
  if (rc != GW_OK) return rc;
  if (ld_out < heads * dim_head) return failf(GW_E_BADARG, "gw_attention_forward: bad arguments");
  AttnArgs a = {};
  a.batch = batch, a.inner = 1, a.heads = heads, a.n = n, a.d = dim_head, a.pairs = (int64_t)batch * heads;
  a.q = q, a.k = k, a.v = v, a.scale = scale, a.out = out, a.lse = lse;
  rows3(a.sq, n, ld_qkv), rows3(a.so, n, ld_out);
  return attn_forward_launch(a, stream);
}

int gw_attention_backward(int32_t batch, int32_t heads, int32_t n, int32_t dim_head, const float* q, const float* k, const float* v,
                          int32_t ld_qkv, float scale, const float* out, int32_t ld_out, const float* dout, int32_t ld_dout,
                          const float* lse, float* delta, float* dq, float* dk, float* dv, int32_t ld_dqkv, void* stream) {
  if (!q || !k || !v || !out || !dout || !lse || !delta || !dq || !dk || !dv)
    return failf(GW_E_BADARG, "gw_attention_backward: bad arguments");
  int rc = attn_check("gw_attention_backward", batch, heads, n, dim_head, (int64_t)heads * dim_head, ld_qkv);
  if (rc != GW_OK) return rc;
  const int inner = heads * dim_head;
  if (ld_out < inner || ld_dout < inner || ld_dqkv < inner) return failf(GW_E_BADARG, "gw_attention_backward: bad arguments");
  AttnArgs a = {};
  a.batch = batch, a.inner = 1, a.heads = heads, a.n = n, a.d = dim_head, a.pairs = (int64_t)batch * heads;
  a.q = q, a.k = k, a.v = v, a.scale = scale, a.out = const_cast<float*>(out), a.lse = const_cast<float*>(lse);
  a.dout = dout, a.delta = delta, a.dq = dq, a.dk = dk, a.dv = dv;
  rows3(a.sq, n, ld_qkv), rows3(a.so, n, ld_out), rows3(a.sg, n, ld_dout), rows3(a.sd, n, ld_dqkv);
  return attn_backward_launch(a, stream);
}

int gw_knn_interpolate_forward(int32_t batch, int32_t n_tgt, int32_t channels, int32_t k, const int32_t* idx, const float* w,
                               const float* x, int64_t x_stride_b, int64_t x_stride_row, int64_t x_stride_c, float* y,
                               int64_t y_stride_b, int64_t y_stride_row, int64_t y_stride_c, void* stream) {
  if (!idx || !w || !x || !y || batch < 0 || n_tgt < 0 || channels < 0 || k <= 0)
    return failf(GW_E_BADARG, "gw_knn_interpolate_forward: bad arguments");
  const int64_t total = (int64_t)batch * n_tgt * channels;
  if (total == 0) return GW_OK;
  hipLaunchKernelGGL(knn_fwd_kernel, dim3(stream_blocks(total)), dim3(256), 0, (hipStream_t)stream, batch, n_tgt, channels, k, idx, w, x,
                     x_stride_b, x_stride_row, x_stride_c, y, y_stride_b, y_stride_row, y_stride_c, y_stride_c == 1 ? 1 : 0);
  return check_launch("knn_fwd_kernel launch");
}

int gw_knn_interpolate_backward(int32_t batch, int32_t n_src, int32_t channels, const int32_t* src_ptr, const int32_t* src_tgt,
                                const float* src_w, const float* dy, int64_t y_stride_b, int64_t y_stride_row, int64_t y_stride_c,
                                float* dx, int64_t x_stride_b, int64_t x_stride_row, int64_t x_stride_c, void* stream) {
  if (!src_ptr || !src_tgt || !src_w || !dy || !dx || batch < 0 || n_src < 0 || channels < 0)
    return failf(GW_E_BADARG, "gw_knn_interpolate_backward: bad arguments");
  const int64_t total = (int64_t)batch * n_src * channels;
  if (total == 0) return GW_OK;
  hipLaunchKernelGGL(knn_bwd_kernel, dim3(stream_blocks(total)), dim3(256), 0, (hipStream_t)stream, batch, n_src, channels, src_ptr, src_tgt,
                     src_w, dy, y_stride_b, y_stride_row, y_stride_c, dx, x_stride_b, x_stride_row, x_stride_c, x_stride_c == 1 ? 1 : 0);
  return check_launch("knn_bwd_kernel launch");
}

int gw_gelu_forward(int64_t n, const float* x, float* y, void* stream) {
  if (!x || !y || n < 0) return failf(GW_E_BADARG, "gw_gelu_forward: bad arguments");
  if (n == 0) return GW_OK;
  hipLaunchKernelGGL(gelu_fwd_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, n, x, y);
  return check_launch("gelu_fwd_kernel launch");
}

int gw_gelu_backward(int64_t n, const float* x, const float* dy, float* dx, void* stream) {
  if (!x || !dy || !dx || n < 0) return failf(GW_E_BADARG, "gw_gelu_backward: bad arguments");
  if (n == 0) return GW_OK;
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, n, x, dy, dx);
  return check_launch("gelu_bwd_kernel launch");
}

}  // extern "C"
