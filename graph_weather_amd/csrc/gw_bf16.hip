// gw_bf16.hip - bf16-MFMA variant of the fused MLP kernels (BASELINE.json configs[2]: "bf16 MFMA node-MLPs").
//
// Same transposed, register-resident scheme as the fp32 kernels (gw_kernels.hip / gw_edge.hip):
//       H_out[feature][column] = W[feature][k] . H_in[k][column],
// but on v_mfma_f32_16x16x32_bf16 (fp32 accumulate): weights are the A operand (lane: row = lane & 15, 8 consecutive
// packed k's selected by lane >> 4), activations the B operand (column = lane & 15), converted fp32 -> bf16 (RNE) in
// registers.  With the K order
//       k(s, q, i) = 32 s + 16 (i >> 2) + 4 q + (i & 3)        (s = K-step, q = lane >> 4, i = 0..7)
// the 8 values a lane must supply for K-step s of the next layer are exactly its accumulator entries of row tiles
// 2s and 2s+1, so the chain of layers + LayerNorm + residual stays in registers as in fp32.
// Everything that is not a matrix product (bias, LayerNorm statistics, residual adds, segment sums, and every tensor
// in HBM) stays fp32.
//
// bf16 matrix cores are 16x faster than the fp32 ones, so the balance moves to the weight stream: one A fragment
// (1 KiB per wave) read from LDS feeds 4 MFMAs here - every wave works on FOUR 16-column groups (64 columns, 256 per
// workgroup) - which keeps LDS reads at a quarter of their peak and the L2->LDS weight DMA at 0.5 KiB per column
// and layer.  That needs ~420 VGPRs per wave: one workgroup (4 waves) per CU.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "gw_chain16_common.hpp"

using namespace gw;
using namespace gw::chain16;

#ifdef GW_TUNING
#define GW_TUNE16(a) ((a).tune16)
#else
#define GW_TUNE16(a) 0
#endif

namespace {

// A workgroup is NW waves x NG 16-column groups per wave.  4 x 2 (128 columns, one wave per SIMD, ~450 registers: every A
// fragment read from LDS feeds two MFMAs) is the form of the general kernels; the row-wise launches of the fused forward are
// bound by their row loads / stores, which one lock-stepped workgroup per CU cannot overlap with anything, and run as 4 x 1
// (64 columns, <= 256 registers, TWO workgroups per CU: twice the weight DMA and LDS reads per column, but one workgroup's
// row traffic under the other's MFMA phases - measured 14-30 % faster; 8 x 1 in one workgroup sits between).
constexpr int kBufBytes = 32768;            // one weight chunk buffer (2 K-steps x 16 tiles x 1 KiB)
constexpr int kLdsWeights = 2 * kBufBytes;  // double buffered
constexpr int kLdsEdge = kLdsWeights + (kStageFloats + 64) * 4;

__device__ __forceinline__ bf16x8 pack8(f32x4 lo, f32x4 hi) {
  bf16x8 r;
  r[0] = (__bf16)lo.x; r[1] = (__bf16)lo.y; r[2] = (__bf16)lo.z; r[3] = (__bf16)lo.w;
  r[4] = (__bf16)hi.x; r[5] = (__bf16)hi.y; r[6] = (__bf16)hi.z; r[7] = (__bf16)hi.w;
  return r;
}
// layer-1 node products as fp16 rows (GW_LAYOUT_ROWS_F16): 11 significant bits in front of the consumer's bf16 rounding of
// the layer-1 activations; clamped to the fp16 range (an overflow would turn into inf, then NaN under LayerNorm)
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void stg_half4(void* p, f32x4 v) {
  half4_t h;
#pragma unroll
  for (int r = 0; r < 4; ++r) h[r] = (_Float16)fminf(fmaxf(v[r], -65504.f), 65504.f);
  *(GW_AS1 half4_t*)p = h;
}

// One layer pass: acc[g][t] += W[16t.., k] . bin[g][k], K = 32 KS, NT row tiles, NTP = tiles per K-step in the packed
// stream (NT rounded up to 4).  The stream of this pass starts at gw; its first chunk has already been issued into
// buffer `parity`; while the last chunk computes, the first chunk of the next pass (next_gw, next_bytes) is issued.
template <int NW, int NG, int KS, int BKS, int NT, int NTP>
__device__ __forceinline__ void pass16(f32x4 (&acc)[NG][NT], const bf16x8 (&bin)[NG][BKS], const char* __restrict__ gw,
                                       const char* __restrict__ next_gw, int next_bytes, const char* lds, int& parity,
                                       int lane, int wave, int tune = 0) {
  constexpr int STEP_BYTES = NTP * 1024;
  constexpr int CS = (2 * STEP_BYTES <= kBufBytes) ? 2 : 1;  // K-steps per chunk
  constexpr int NCH = (KS + CS - 1) / CS;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    constexpr int dummy = 0;
    (void)dummy;
    const int steps_c = (KS - c * CS) < CS ? (KS - c * CS) : CS;
    wait_vm<0>();
    if (!(tune & 4)) lds_barrier();  // chunk c has landed for every wave; nobody still reads the other buffer
    if (!(tune & 1)) {
      if (c + 1 < NCH) {
        const int sn = (KS - (c + 1) * CS) < CS ? (KS - (c + 1) * CS) : CS;
        issue_bytes<NW>(gw + (size_t)(c + 1) * CS * STEP_BYTES, sn * STEP_BYTES, (unsigned)((parity ^ 1) * kBufBytes), lane, wave);
      } else if (next_gw != nullptr) {
        issue_bytes<NW>(next_gw, next_bytes, (unsigned)((parity ^ 1) * kBufBytes), lane, wave);
      }
    }
    if (tune & 2) {
      parity ^= 1;
      continue;
    }
    const char* buf = lds + parity * kBufBytes + lane * 16;
    // The A fragments (4 row tiles = one "unit" of 4 ds_read_b128) travel through a ring of three register sets, requested two
    // units ahead of the MFMAs that use them: this kernel runs ONE wave per SIMD, so an LDS round trip that is waited for right
    // after its request (what the compiler schedules on its own: 2 reads, wait, 2 MFMAs) is exposed in full (measured: 6 % of
    // the row-wise launches; the rest of their per-chunk time is not the weight stream either - neither two chunks in flight
    // nor a per-workgroup rotation of the piece order moved it, profiles/r03 notes in DESIGN.md).
    constexpr int UPS = NTP / 4;           // units per K-step
    const int NU = steps_c * UPS;          // units of this chunk (<= 2 * UPS)
    bf16x8 af[3][4];
    auto ldu = [&](bf16x8 (&f)[4], int u) {
      const int su = u / UPS, t4 = u - su * UPS;
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) f[tt] = *(const bf16x8*)(buf + su * STEP_BYTES + (t4 * 4 + tt) * 1024);
    };
    ldu(af[0], 0);
    if (NU > 1) ldu(af[1], 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < CS * UPS; ++u) {
      if (u < NU) {
        if (u + 2 < NU) ldu(af[(u + 2) % 3], u + 2);
        const int su = u / UPS, t4 = u - su * UPS;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          if (t4 * 4 + tt < NT) {
#pragma unroll
            for (int g = 0; g < NG; ++g)
              acc[g][t4 * 4 + tt] =
                  __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u % 3][tt], bin[g][c * CS + su], acc[g][t4 * 4 + tt], 0, 0, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    parity ^= 1;
  }
}

// bin[s] <- bf16(row[k(s,q,i)]) for a raw operand row (valid features [0, kvalid))
template <int KS, bool FULL, int DEPTH = 4>
__device__ __forceinline__ void load_raw16(bf16x8 (&bin)[KS], const float* __restrict__ row, int kvalid, int q) {
  load_raw_steps<KS, FULL, DEPTH>(row, kvalid, q, [&](int s, f32x4 lo, f32x4 hi) { bin[s] = pack8(lo, hi); });
}

template <int NT>
__device__ __forceinline__ void relu_to_bin(bf16x8 (&bin)[NT / 2], const f32x4 (&acc)[NT]) {
#pragma unroll
  for (int s = 0; s < NT / 2; ++s) bin[s] = pack8(relu4(acc[2 * s]), relu4(acc[2 * s + 1]));
}

// K1S: 32-wide K-steps of a raw layer-1 operand (8: k = 256, 4: k <= 128, 1: k <= 32); HT / OT: hidden / output row tiles.
template <int K1S, bool K1FULL, int NSEG, int HT, int OT, int EPI, bool SINGLE, bool POST = false, bool HEAD = false, int NW = 4,
          int NG = 2>
__global__ __launch_bounds__(NW * 64, (NW * NG == 4 ? 2 : 1)) void chain16_kernel(const ChainArgs a) {
  constexpr int kCols16 = NW * NG * 16;  // columns per workgroup
  static_assert(EPI != EPI_EDGE || (NW == 4 && NG == 2), "the segment-sum epilogue walks 64 columns per round on 4 waves");
  extern __shared__ __attribute__((aligned(16))) char lds16[];
  constexpr int HTP = (HT + 3) / 4 * 4, OTP = (OT + 3) / 4 * 4;
  constexpr int HKS = HT / 2;  // K-steps of a layer fed by the hidden activations
  constexpr int H_STEP = HTP * 1024, O_STEP = OTP * 1024;
  constexpr int H_CS = (2 * H_STEP <= kBufBytes) ? 2 : 1, O_CS = (2 * O_STEP <= kBufBytes) ? 2 : 1;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15;
  const int q = lane >> 4;
  const int tile_c0 = blockIdx.x * kCols16;
  // (measured and dropped: per-batch tiles walked batch-innermost and XCD-aware, so that batch-shared operand rows come from the
  // XCD's L2 - the head launch 1.19 -> 1.18 ms, the mesh-sized node updates 0.168 -> 0.175 ms)

  GW_CHAIN16_COLUMN_COORDS(NW, NG)

  GW_CHAIN16_OPERAND_SCHEDULE(NSEG, SINGLE)
  constexpr int K1_CS = H_CS;
  constexpr int K1FIRST = (K1S < K1_CS ? K1S : K1_CS) * H_STEP;
  const char* after_l1 = SINGLE ? nullptr : (a.n_mid > 0 ? w_mid : w_out);
  const int after_l1_bytes = SINGLE ? 0 : (a.n_mid > 0 ? H_CS * H_STEP : O_CS * O_STEP);
  int parity = 0;
  issue_first_chunk<NW>(on, w1, K1FIRST, after_l1, after_l1_bytes, lane, wave);

  // ---- layer 1 ----
  // One accumulator array and one B-operand array serve every layer (the output layer gets its own accumulator only
  // when its tile count differs from the hidden one): register allocation does not reuse them otherwise.
  constexpr int BKS = K1S > HKS ? K1S : HKS;
  constexpr bool SHARE_ACC = (OT == HT);
  f32x4 acc[NG][HT];
  bf16x8 bin[NG][BKS];
  init_bias<NG, HT>(acc, a.b1, q);
  {
#pragma unroll
    for (int i = 0; i < NSEG; ++i) {
      if (on[i]) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          if (K1S == 8 && a.seg_bf16k[i]) {
            // bf16 rows in K order (GW_LAYOUT_ROWS_BF16K: the aggregate written by the segment-aligned edge kernel): position
            // 32 s + 8 q + i holds feature k(s, q, i) - the lane's B fragment of K-step s is one 16-byte load, no conversion
            const __bf16* rowb = (const __bf16*)a.seg_ptr[i] + ((size_t)bb[g] * (size_t)a.seg_rows_pb[i] + (size_t)kk[g]) * (size_t)a.seg_ld[i];
#pragma unroll
            for (int s = 0; s < (K1S == 8 ? 8 : 0); ++s) bin[g][s] = *(const GW_AS1 bf16x8*)(rowb + 32 * s + 8 * q);
          } else {
            const float* row = operand_row(a.seg_ptr[i], a.seg_idx[i], a.seg_rows_pb[i], a.seg_ld[i], bb[g], kk[g]);
            load_raw16<K1S, K1FULL, (NG == 1 ? 8 : 4)>(reinterpret_cast<bf16x8(&)[K1S]>(bin[g]), row, a.seg_k[i], q);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        const char* nx = after_l1;
        int nb = after_l1_bytes;
#pragma unroll
        for (int i2 = NSEG - 1; i2 > i; --i2)
          if (on[i2]) {
            nx = w1[i2];
            nb = K1FIRST;
          }
        pass16<NW, NG, K1S, BKS, HT, HTP>(acc, bin, w1[i], nx, nb, lds16, parity, lane, wave, GW_TUNE16(a));
      } else if (prj[i]) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          if (a.seg_half[i]) {  // fp16 product rows (GW_LAYOUT_ROWS_F16): 8 bytes per row tile and lane
            const int r = a.seg_idx[i] ? ldgi(a.seg_idx[i] + kk[g]) : kk[g];
            const _Float16* row = (const _Float16*)a.seg_ptr[i] + ((size_t)bb[g] * (size_t)a.seg_rows_pb[i] + (size_t)r) * (size_t)a.seg_ld[i];
#pragma unroll
            for (int t = 0; t < HT; ++t) {
              const half4_t h = *(const GW_AS1 half4_t*)(row + 16 * t + 4 * q);
              acc[g][t] += f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
              if ((t & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
          } else {
            const float* row = operand_row(a.seg_ptr[i], a.seg_idx[i], a.seg_rows_pb[i], a.seg_ld[i], bb[g], kk[g]);
#pragma unroll
            for (int t = 0; t < HT; ++t) {
              acc[g][t] += ldg4(row + 16 * t + 4 * q);
              if ((t & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
      }
    }
  }

  f32x4 o_sep[SHARE_ACC ? 1 : NG][SHARE_ACC ? 1 : OT];
  f32x4 (&o)[NG][OT] = *reinterpret_cast<f32x4(*)[NG][OT]>(SHARE_ACC ? (void*)acc : (void*)o_sep);
  if constexpr (!SINGLE) {
    // ---- middle layers (hidden -> hidden) ----
#pragma unroll 1
    for (int l = 0; l < a.n_mid; ++l) {
#pragma unroll
      for (int g = 0; g < NG; ++g) relu_to_bin<HT>(reinterpret_cast<bf16x8(&)[HKS]>(bin[g]), acc[g]);
      __builtin_amdgcn_sched_barrier(0);
      init_bias<NG, HT>(acc, a.b_mid + l * (HT * 16), q);
      const bool last = (l + 1 == a.n_mid);
      const char* nx = last ? w_out : w_mid + (size_t)(l + 1) * HKS * H_STEP;
      const int nb = last ? O_CS * O_STEP : H_CS * H_STEP;
      pass16<NW, NG, HKS, BKS, HT, HTP>(acc, bin, w_mid + (size_t)l * HKS * H_STEP, nx, nb, lds16, parity, lane, wave, GW_TUNE16(a));
    }
    // ---- output layer ----
#pragma unroll
    for (int g = 0; g < NG; ++g) relu_to_bin<HT>(reinterpret_cast<bf16x8(&)[HKS]>(bin[g]), acc[g]);
    __builtin_amdgcn_sched_barrier(0);
    init_bias<NG, OT>(o, a.b_out, q);
    pass16<NW, NG, HKS, BKS, OT, OTP>(o, bin, w_out, POST ? (const char*)a.proj_w[0] : (HEAD ? (const char*)a.hd_w1 : nullptr),
                              POST ? H_CS * H_STEP : (HEAD ? 2 * 8 * 1024 : 0), lds16, parity, lane, wave, GW_TUNE16(a));
  }

  // ---- LayerNorm over the OT*16 features of each column (eps 1e-5, biased variance), fp32 ----
  if (!SINGLE && a.gamma != nullptr) {
    GW_CHAIN16_LAYERNORM(o, NG, OT, false)
  }

  // ---- residual ----
  if (!SINGLE && !HEAD && a.res_ptr != nullptr && !(GW_TUNE16(a) & 16)) {
    GW_CHAIN16_ADD_RESIDUAL(o, NG, OT, EPI)
  }

  // ---- store ----
  float* outp = SINGLE ? a.proj_out[blockIdx.y] : a.out;
  if (!HEAD && outp != nullptr && !(GW_TUNE16(a) & 8)) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (valid[g]) {
        float* orow = outp + (size_t)cc[g] * (size_t)a.out_ld;
#pragma unroll
        for (int t = 0; t < OT; ++t) {
          const int f0 = 16 * t + 4 * q;
          if (SINGLE && a.proj_half) {  // (out_ld counts halves)
            stg_half4((_Float16*)outp + (size_t)cc[g] * (size_t)a.out_ld + f0, o[g][t]);
          } else {
            store_tile<EPI>(orow, f0, o[g][t], a.out_cols);
          }
        }
      }
    }
  }


  // ---- HEAD: the output head on the new rows while they are still in registers (ChainArgs): 256 -> 128 relu -> 128 relu ->
  // <= 80 features (+ residual rows), e.g. AssimilatorDecoder.node_decoder + the Decoder residual (assimilator_decoder.py:197,
  // decoder.py:93) behind the decoder's node update: the [rows, 256] table between them (1 GB at 1 degree, batch 16) is never
  // written or read ----
  if constexpr (HEAD) {
    static_assert(!HEAD || (OT == 16 && HT == 16 && SHARE_ACC && !POST && !SINGLE), "HEAD follows a 256-wide node update");
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int s = 0; s < 8; ++s) bin[g][s] = pack8(o[g][2 * s], o[g][2 * s + 1]);  // (no relu: the head's input is the LayerNorm output)
    __builtin_amdgcn_sched_barrier(0);
    constexpr int HS = 8 * 1024;  // bytes of one K-step of a packed slice with <= 8 row tiles
    f32x4 hh[NG][8];
    init_bias<NG, 8>(hh, a.hd_b1, q);
    pass16<NW, NG, 8, BKS, 8, 8>(hh, bin, (const char*)a.hd_w1, (const char*)a.hd_w2, 2 * HS, lds16, parity, lane, wave, GW_TUNE16(a));
#pragma unroll
    for (int g = 0; g < NG; ++g) relu_to_bin<8>(reinterpret_cast<bf16x8(&)[4]>(bin[g]), hh[g]);
    __builtin_amdgcn_sched_barrier(0);
    init_bias<NG, 8>(hh, a.hd_b2, q);
    pass16<NW, NG, 4, BKS, 8, 8>(hh, bin, (const char*)a.hd_w2, (const char*)a.hd_w3, 2 * HS, lds16, parity, lane, wave, GW_TUNE16(a));
#pragma unroll
    for (int g = 0; g < NG; ++g) relu_to_bin<8>(reinterpret_cast<bf16x8(&)[4]>(bin[g]), hh[g]);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 y[NG][5];
    init_bias<NG, 5>(y, a.hd_b3, q);
    pass16<NW, NG, 4, BKS, 5, 8>(y, bin, (const char*)a.hd_w3, nullptr, 0, lds16, parity, lane, wave, GW_TUNE16(a));
    GW_CHAIN16_STORE_HEAD_ROWS(y, NG)
  }

  // ---- POST: the next block's layer-1 products of the new rows, while they are still in registers (see ChainArgs) ----
  if constexpr (POST) {
    static_assert(!POST || (OT == 16 && HT == 16 && SHARE_ACC), "POST works on 256-wide rows");
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int s = 0; s < 8; ++s) bin[g][s] = pack8(o[g][2 * s], o[g][2 * s + 1]);
    __builtin_amdgcn_sched_barrier(0);
    if (a.zero_rows != nullptr) {
      GW_CHAIN16_ZERO_FILL(NG)
    }
#pragma unroll 1
    for (int sl = 0; sl < a.n_post; ++sl) {
      init_bias<NG, HT>(acc, nullptr, q);  // (acc aliases o: the new rows have been stored and packed into bin)
      const char* nx = sl + 1 < a.n_post ? (const char*)a.proj_w[sl + 1] : nullptr;
      pass16<NW, NG, 8, BKS, HT, HTP>(acc, bin, (const char*)a.proj_w[sl], nx, H_CS * H_STEP, lds16, parity, lane, wave, GW_TUNE16(a));
#pragma unroll
      for (int g = 0; g < NG; ++g)
        if (valid[g] && !(GW_TUNE16(a) & 32)) {
          if (a.proj_half) {
            _Float16* prow = (_Float16*)a.proj_out[sl] + (size_t)cc[g] * 256;
#pragma unroll
            for (int t = 0; t < HT; ++t) stg_half4(prow + 16 * t + 4 * q, acc[g][t]);
          } else {
            store_tiles<HT>(a.proj_out[sl] + (size_t)cc[g] * 256, acc[g], q);
          }
        }
    }
  }

  // ---- segment sum over destination-sorted columns, 64 columns at a time through LDS (see gw_edge.hip) ----
  if (EPI == EPI_EDGE) {
    GW_CHAIN16_SEGMENT_SUM(o, (float*)(lds16 + kLdsWeights), NW, NG, OT, 0, wave)
  }
}

// ---- weight packing: nn.Linear [n_out, k_total] slice -> bf16 MFMA A-operand stream -------------------------------
// out[s][tile][lane][i] = bf16(W[16 tile + (lane & 15)][k_lo + 32 s + 16 (i >> 2) + 4 (lane >> 4) + (i & 3)]), 0 outside
__global__ void pack_linear_bf16_kernel(const float* __restrict__ w, int n_out, int k_total, int k_lo, int kseg, int ntp,
                                        int nsteps, __bf16* __restrict__ out) {
  const size_t total = (size_t)nsteps * ntp * 512;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e & 7);
    const int lane = (int)((e >> 3) & 63);
    const int tile = (int)((e >> 9) % ntp);
    const int s = (int)((e >> 9) / ntp);
    const int f = 16 * tile + (lane & 15);
    const int kx = 32 * s + 16 * (i >> 2) + 4 * (lane >> 4) + (i & 3);
    out[e] = (__bf16)((f < n_out && kx < kseg) ? w[(size_t)f * k_total + k_lo + kx] : 0.f);
  }
}

template <typename K>
int launch16(K kernel, ChainArgs& a, void* stream, int grid_y, int lds_bytes, int threads = 256, int cols = 128) {
  return launch_chain16(kernel, a, stream, grid_y, lds_bytes, threads, cols, kLdsEdge, "chain16_kernel launch");
}

}  // namespace

namespace gw {

int chain16_launch(int kind, ChainArgs& a, int k_in, int hidden, int n_out, int grid_y, void* stream) {
#ifdef GW_TUNING
  {
    static const int t16 = GW_TUNE("GW_CHAIN16_TUNE", 0);
    a.tune16 = t16;
  }
#endif
  // The row-wise launches of the fused forward (node update, + post products, + head, node encoder + post products) run as
  // 4 waves x 1 group with two workgroups per CU (see the note above).  Tuning builds: GW_CHAIN16_NW=4 selects 4 x 2, 8 selects 8 x 1.
#ifdef GW_TUNING
  static const int nw = GW_TUNE("GW_CHAIN16_NW", 41);
  if (nw == 8) {
    switch (kind) {
      case 2:
        return launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, false, false, 8, 1>, a, stream, 1, kLdsWeights, 512);
      case 4:
        return launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, true, false, 8, 1>, a, stream, 1, kLdsWeights, 512);
      case 6:
        return launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, false, true, 8, 1>, a, stream, 1, kLdsWeights, 512);
      case 5:
        if (hidden == 256 && n_out == 256 && k_in <= 128 && k_in > 32)
          return launch16(chain16_kernel<4, false, 1, 16, 16, EPI_ROWS, false, true, false, 8, 1>, a, stream, 1, kLdsWeights, 512);
        break;
      default:
        break;
    }
  }
  if (nw == 12 || nw == 16) {  // one workgroup of 12 / 16 waves per CU: 192 / 256 columns share one weight stream
    const int th = nw * 64, cl = nw * 16;
    switch (kind) {
      case 2:
        return nw == 12 ? launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, false, false, 12, 1>, a, stream, 1, kLdsWeights, th, cl)
                        : launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, false, false, 16, 1>, a, stream, 1, kLdsWeights, th, cl);
      case 4:
        return nw == 12 ? launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, true, false, 12, 1>, a, stream, 1, kLdsWeights, th, cl)
                        : launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, true, false, 16, 1>, a, stream, 1, kLdsWeights, th, cl);
      case 6:
        return nw == 12 ? launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, false, true, 12, 1>, a, stream, 1, kLdsWeights, th, cl)
                        : launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, false, true, 16, 1>, a, stream, 1, kLdsWeights, th, cl);
      case 5:
        if (hidden == 256 && n_out == 256 && k_in <= 128 && k_in > 32)
          return nw == 12 ? launch16(chain16_kernel<4, false, 1, 16, 16, EPI_ROWS, false, true, false, 12, 1>, a, stream, 1, kLdsWeights, th, cl)
                          : launch16(chain16_kernel<4, false, 1, 16, 16, EPI_ROWS, false, true, false, 16, 1>, a, stream, 1, kLdsWeights, th, cl);
        break;
      default:
        break;
    }
  }
  if (nw == 4) {
    switch (kind) {
      case 2:
        return launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false>, a, stream, 1, kLdsWeights);
      case 4:
        return launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, true>, a, stream, 1, kLdsWeights);
      case 6:
        return launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, false, true>, a, stream, 1, kLdsWeights);
      case 5:
        if (hidden == 256 && n_out == 256 && k_in <= 128 && k_in > 32)
          return launch16(chain16_kernel<4, false, 1, 16, 16, EPI_ROWS, false, true>, a, stream, 1, kLdsWeights);
        break;
      default:
        break;
    }
  }
#endif
  switch (kind) {
    case 0:  // mlp rows
      if (hidden == 256 && n_out == 256) {
        if (k_in <= 32) return launch16(chain16_kernel<1, false, 1, 16, 16, EPI_ROWS, false>, a, stream, 1, kLdsWeights);
        if (k_in <= 128) return launch16(chain16_kernel<4, false, 1, 16, 16, EPI_ROWS, false>, a, stream, 1, kLdsWeights);
        if (k_in == 256) return launch16(chain16_kernel<8, true, 1, 16, 16, EPI_ROWS, false>, a, stream, 1, kLdsWeights);
      } else if (hidden == 256 && n_out <= 80 && k_in == 256) {
        return launch16(chain16_kernel<8, true, 1, 16, 5, EPI_DEC, false>, a, stream, 1, kLdsWeights);
      } else if (hidden == 128 && n_out <= 80 && k_in == 256) {
        return launch16(chain16_kernel<8, true, 1, 8, 5, EPI_DEC, false>, a, stream, 1, kLdsWeights);
      }
      return set_error(GW_E_UNSUPPORTED, "bf16 mlp: unsupported (hidden, n_out, k) combination");
    case 1:
      return launch16(chain16_kernel<8, true, 3, 16, 16, EPI_EDGE, false>, a, stream, 1, kLdsEdge);
    case 2:
      return launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, false, false, 4, 1>, a, stream, 1, kLdsWeights, 256, 64);
    case 3:
      return launch16(chain16_kernel<8, true, 1, 16, 16, EPI_ROWS, true>, a, stream, grid_y, kLdsWeights);
    case 4:
      return launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, true, false, 4, 1>, a, stream, 1, kLdsWeights, 256, 64);
    case 6:  // node update + output head (decoder)
      return launch16(chain16_kernel<8, true, 2, 16, 16, EPI_ROWS, false, false, true, 4, 1>, a, stream, 1, kLdsWeights, 256, 64);
    case 5:  // mlp rows + POST products of the output rows (node encoder -> layer-1 products of the encoder's edge MLP)
      if (hidden == 256 && n_out == 256 && k_in <= 128 && k_in > 32)
        return launch16(chain16_kernel<4, false, 1, 16, 16, EPI_ROWS, false, true, false, 4, 1>, a, stream, 1, kLdsWeights, 256, 64);
      return set_error(GW_E_UNSUPPORTED, "bf16 mlp + post products: hidden 256, 256 outputs, 33..128 inputs");
  }
  return set_error(GW_E_BADARG, "chain16_launch: bad kind");
}

}  // namespace gw

extern "C" {

size_t gw_packed_bytes_bf16(int n_out, int k_lo, int k_hi) {
  const int kseg = k_hi - k_lo;
  const int nsteps = packed_steps16(kseg);
  const int ntp = padded_tiles(n_out);
  return (size_t)nsteps * ntp * 1024;
}

int gw_pack_linear_bf16(const float* w, int n_out, int k_total, int k_lo, int k_hi, void* out, void* stream) {
  if (!w || !out || n_out <= 0 || k_lo < 0 || k_hi <= k_lo || k_hi > k_total)
    return gw::set_error(GW_E_BADARG, "gw_pack_linear_bf16: bad arguments");
  const int kseg = k_hi - k_lo;
  const int nsteps = packed_steps16(kseg);
  const int ntp = padded_tiles(n_out);
  const size_t total = (size_t)nsteps * ntp * 512;
  int grid = (int)((total + 255) / 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(pack_linear_bf16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, n_out, k_total, k_lo, kseg, ntp,
                     nsteps, (__bf16*)out);
  return gw::check_launch("pack_linear_bf16_kernel launch");
}

}  // extern "C"
