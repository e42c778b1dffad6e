// gw_modulate.hip - the reference's two per-channel modulation layers on [B, C, *spatial] activations:
// StochasticDecompositionLayer (layers/stochastic_decomposition.py: out = x + alpha * style(z) * eps) and FiLMApplier
// (layers/film.py: out = x * gamma + beta).  A tensor is rows = B * C dense rows of S = prod(spatial) floats; the two small
// dense parts (style_net, the FiLM generator) are gw_linear_forward launches made from Python.  Pure streaming: no matrix cores.
//
//   apply_kernel        one thread per aligned group of four flat elements: 16-byte loads / stores when the pointers allow
//                       and the group is whole, scalar ones otherwise; the row (-> channel, scale) of every element comes
//                       from the flat index, so S need not be a multiple of four.  SDL: the noise is made in registers.
//   reduce_wave_kernel  S >= kShortRow: one wave per (row, chunk of kChunk elements) -> fp64 partial sums of dy * eps (SDL; eps
//                       regenerated from the key) or of dy * x and dy (FiLM; dx = dy * gamma is stored on the way)
//   reduce_row_kernel   S <  kShortRow: one thread per row, the same sums in element order
//   sdl_final_kernel    per row: R = the chunk partials added in chunk order; d_style = alpha * R
//   sdl_alpha_kernel    per channel: d_alpha = sum_b style * R in batch order
//   film_final_kernel   per row: d_gamma, d_beta from the chunk partials in chunk order
// Every sum has one fixed order (lane-strided fp32 in a chunk, a fixed butterfly across the wave and the chunk order in fp64):
// bitwise reproducible, no atomics.
//
// The noise eps(key, i) is specified in include/gw_amd.h: Philox4x32-10 on the group index i / 4, Box-Muller on the 24 high
// bits of each word.  It is evaluated from the integers so that the result does not depend on the accuracy of the hardware
// transcendentals: with t = 2 (w >> 8) + 1 (25 bits, odd) u = t / 2^25;
//   ln u      = logf(float(t) / 2^25) + (t - float(t)) / float(t)   (float(t) rounds above 2^24: without the second term
//               r = sqrt(-2 ln u) would be 0 instead of 2.4e-4 at the largest t)
//   2 pi u    : quadrant t >> 23, then the low 23 bits folded into [0, pi / 4] exactly and the single-precision minimax
//               polynomials of sine and cosine on that interval (Cephes sinf / cosf, about 1 ulp)
// which keeps |eps - exact| below 2e-6 (the angle carries 1e-7, times r <= 5.89; the radius 1 - 2 ulp).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gw_amd.h"
#include "gw_internal.hpp"

using namespace gw;

namespace {

int failm(int code, const char* msg) { return set_error(code, msg); }

constexpr int kShortRow = 64;   // rows shorter than this are reduced by one thread each
constexpr int kChunk = 2048;    // elements of a row per wave of reduce_wave_kernel: 8 groups of four per lane

enum { M_SDL_KEY = 0, M_SDL_NOISE = 1, M_FILM = 2, M_NOISE_ONLY = 3 };

__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// (r cos(2 pi u_b), r sin(2 pi u_b)) with r = sqrt(-2 ln u_a), u = ((w >> 8) + 0.5) / 2^24 = t / 2^25.  Every multiply-add is
// an explicit fmaf and no product is ever an addend, so there is nothing left for the compiler to contract one way or another.
__device__ inline void box_muller(uint32_t wa, uint32_t wb, float& e_cos, float& e_sin) {
#pragma clang fp contract(off)
  const uint32_t ta = 2u * (wa >> 8) + 1u;
  const float tf = (float)ta;                       // rounds to even above 2^24
  const float delta = (float)((int)ta - (int)tf);   // -1, 0 or 1
  // the correction term is below 6e-8: 1 ulp of the hardware reciprocal is nothing
  const float lnu = fmaf(delta, __builtin_amdgcn_rcpf(tf), logf(tf * 2.98023223876953125e-8f /* 2^-25 */));
  const float r = sqrtf(-2.0f * lnu);
  const uint32_t tb = 2u * (wb >> 8) + 1u;
  const uint32_t quad = tb >> 23, m = tb & 0x7FFFFFu;  // angle = (quad + m / 2^23) * pi / 2, m odd
  const bool fold = m > 0x400000u;
  const float th = (float)(fold ? 0x800000u - m : m) * (float)(3.14159265358979323846 / 16777216.0) /* pi / 2^24 */;  // in (0, pi / 4)
  const float z = th * th;
  const float ps = fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
  const float pc = fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
  float s = fmaf(ps * z, th, th);
  float c = fmaf(pc * z, z, fmaf(-0.5f, z, 1.0f));
  if (fold) {
    const float t = s;
    s = c, c = t;
  }
  const float cq = (quad & 1u) ? -s : c, sq = (quad & 1u) ? c : s;
  const float sign = (quad & 2u) ? -r : r;
  e_cos = sign * cq;
  e_sin = sign * sq;
}

// the noise of the elements 4 j .. 4 j + 3.  Not inlined on purpose: every kernel then runs the one compiled instruction
// sequence, which is what makes the forward, the backward and gw_sdl_forward's raw-noise mode agree bit for bit.
__device__ __noinline__ float4 eps4_values(uint32_t k0, uint32_t k1, uint64_t j) {
  uint32_t w[4];
  float4 e;
  philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), 0u, 0u, k0, k1, w);
  box_muller(w[0], w[1], e.x, e.y);
  box_muller(w[2], w[3], e.z, e.w);
  return e;  // in registers
}

__device__ inline void eps4(uint32_t k0, uint32_t k1, uint64_t j, float e[4]) {
  const float4 v = eps4_values(k0, k1, j);
  e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
}

__device__ inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// loads the elements [i, i + 4) that lie inside [lo, hi) (the others: 0); one 16-byte load when all four do and vec says so
__device__ inline void load4(const float* __restrict__ p, int64_t i, int64_t lo, int64_t hi, bool vec, float v[4]) {
  if (vec && i >= lo && i + 4 <= hi) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = (i + q >= lo && i + q < hi) ? p[i + q] : 0.f;
  }
}

__device__ inline void store4(float* __restrict__ p, int64_t i, int64_t lo, int64_t hi, bool vec, const float v[4]) {
  if (vec && i >= lo && i + 4 <= hi) {
    *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (i + q >= lo && i + q < hi) p[i + q] = v[q];
  }
}

struct ApplyArgs {
  int64_t n, groups, spatial;  // n = rows * spatial elements in groups = ceil(n / 4) groups
  int channels;
  const float* x;      // SDL, FiLM
  const float* a;      // SDL: style [rows];  FiLM: gamma [rows]
  const float* b;      // SDL: alpha [channels];  FiLM: beta [rows]
  const uint32_t* key;
  const float* noise;
  float* out;
};

template <int MODE>
__global__ __launch_bounds__(256) void apply_kernel(ApplyArgs a) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.groups) return;
  const int64_t i0 = 4 * j, S = a.spatial;
  float e[4], x[4], y[4];
  if (MODE == M_SDL_KEY || MODE == M_NOISE_ONLY) eps4(a.key[0], a.key[1], (uint64_t)j, e);
  const bool vec_out = aligned16(a.out);
  if (MODE == M_NOISE_ONLY) {
    store4(a.out, i0, 0, a.n, vec_out, e);
    return;
  }
  if (MODE == M_SDL_NOISE) load4(a.noise, i0, 0, a.n, aligned16(a.noise), e);
  load4(a.x, i0, 0, a.n, aligned16(a.x), x);
  // row of the group's first element (32-bit division whenever the tensor allows it), then walked forward element by element
  int64_t row = (a.n <= 0xFFFFFFFFll) ? (int64_t)((uint32_t)i0 / (uint32_t)S) : i0 / S;
  int64_t s = i0 - row * S;
  float p0 = 0.f, p1 = 0.f;
  int64_t have = -1;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (s >= S) s -= S, ++row;
    if (i0 + q < a.n && row != have) {
      have = row;
      if (MODE == M_FILM) {
        p0 = a.a[row], p1 = a.b[row];
      } else {
        p0 = a.b[(uint32_t)row % (uint32_t)a.channels] * a.a[row];
      }
    }
    y[q] = MODE == M_FILM ? x[q] * p0 + p1 : x[q] + p0 * e[q];
    ++s;
  }
  store4(a.out, i0, 0, a.n, vec_out, y);
}

struct ReduceArgs {
  int64_t rows, spatial, units;  // units = rows * chunks_per_row (reduce_wave_kernel) or rows
  int chunks_per_row;
  const float* dy;
  const float* x;       // FiLM: the forward's input (NULL: no d_gamma)
  const float* gamma;   // FiLM: [rows] (with dx)
  const uint32_t* key;
  const float* noise;
  float* dx;            // FiLM: dy * gamma, or NULL
  double* part;         // [2][units]: plane 0 = sum dy * (eps | x), plane 1 = sum dy (FiLM)
};

// sums of one group of four (elements outside [lo, hi) are zero in dy) into the lane's accumulators
template <int MODE>
__device__ inline void accumulate(const ReduceArgs& a, int64_t i, int64_t lo, int64_t hi, float g, float& a0, float& a1) {
  float dy[4], w[4];
  load4(a.dy, i, lo, hi, aligned16(a.dy), dy);
  if (MODE == M_SDL_KEY) {
    eps4(a.key[0], a.key[1], (uint64_t)(i >> 2), w);
  } else if (MODE == M_SDL_NOISE) {
    load4(a.noise, i, lo, hi, aligned16(a.noise), w);
  } else if (a.x) {
    load4(a.x, i, lo, hi, aligned16(a.x), w);
  } else {
    w[0] = w[1] = w[2] = w[3] = 0.f;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    a0 += dy[q] * w[q];
    if (MODE == M_FILM) a1 += dy[q];
  }
  if (MODE == M_FILM && a.dx) {
    float d[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = dy[q] * g;
    store4(a.dx, i, lo, hi, aligned16(a.dx), d);
  }
}

// grid ceil(units / 4), block 256: wave -> (row, chunk).  The aligned groups of four that overlap the chunk are dealt to the
// lanes in turn; a group that straddles a chunk or row border is visited by both neighbours, each taking its own elements.
template <int MODE>
__global__ __launch_bounds__(256) void reduce_wave_kernel(ReduceArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= a.units) return;
  const int64_t row = unit / a.chunks_per_row;
  const int chunk = (int)(unit - row * a.chunks_per_row);
  const int64_t base = row * a.spatial;
  const int64_t lo = base + (int64_t)chunk * kChunk;
  const int64_t hi = min(base + a.spatial, lo + kChunk);
  const float g = (MODE == M_FILM && a.dx) ? a.gamma[row] : 0.f;
  float a0 = 0.f, a1 = 0.f;
  for (int64_t j = (lo >> 2) + lane; 4 * j < hi; j += 64) accumulate<MODE>(a, 4 * j, lo, hi, g, a0, a1);
  double s0 = a0, s1 = a1;
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {  // fixed butterfly: every lane ends with the same sum
    s0 += __shfl_xor(s0, w, 64);
    if (MODE == M_FILM) s1 += __shfl_xor(s1, w, 64);
  }
  if (lane == 0) {
    a.part[unit] = s0;
    if (MODE == M_FILM) a.part[a.units + unit] = s1;
  }
}

// one thread per row of fewer than kShortRow elements, in element order
template <int MODE>
__global__ __launch_bounds__(256) void reduce_row_kernel(ReduceArgs a) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= a.rows) return;
  const int64_t lo = row * a.spatial, hi = lo + a.spatial;
  const float g = (MODE == M_FILM && a.dx) ? a.gamma[row] : 0.f;
  float a0 = 0.f, a1 = 0.f;
  for (int64_t j = lo >> 2; 4 * j < hi; ++j) accumulate<MODE>(a, 4 * j, lo, hi, g, a0, a1);
  a.part[row] = (double)a0;
  if (MODE == M_FILM) a.part[a.units + row] = (double)a1;
}

__device__ inline double chunk_sum(const double* __restrict__ part, int64_t row, int cpr) {
  double s = 0.0;
  for (int k = 0; k < cpr; ++k) s += part[row * cpr + k];
  return s;
}

__global__ __launch_bounds__(256) void sdl_final_kernel(int64_t rows, int channels, int cpr, const double* __restrict__ part,
                                                        const float* __restrict__ alpha, double* __restrict__ R,
                                                        float* __restrict__ d_style) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const double r = chunk_sum(part, row, cpr);
  R[row] = r;
  if (d_style) d_style[row] = alpha[(uint32_t)row % (uint32_t)channels] * (float)r;
}

__global__ __launch_bounds__(256) void sdl_alpha_kernel(int64_t rows, int channels, const double* __restrict__ R,
                                                        const float* __restrict__ style, float* __restrict__ d_alpha) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= channels) return;
  double s = 0.0;
  for (int64_t r = c; r < rows; r += channels) s += (double)style[r] * R[r];
  d_alpha[c] = (float)s;
}

__global__ __launch_bounds__(256) void film_final_kernel(int64_t rows, int64_t units, int cpr, const double* __restrict__ part,
                                                         float* __restrict__ d_gamma, float* __restrict__ d_beta) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  if (d_gamma) d_gamma[row] = (float)chunk_sum(part, row, cpr);
  if (d_beta) d_beta[row] = (float)chunk_sum(part + units, row, cpr);
}

struct Plan {
  int cpr = 1;         // chunks per row
  int64_t units = 0;   // rows * cpr
  size_t r_off = 0, bytes = 0;
};

// shapes one launch covers: rows and row chunks must index a 32-bit grid
int plan_of(int64_t rows, int64_t spatial, Plan& p, const char* who) {
  static char msg[160];
  if (rows <= 0 || spatial <= 0) {
    snprintf(msg, sizeof(msg), "%s: bad arguments", who);
    return failm(GW_E_BADARG, msg);
  }
  const int64_t cpr = spatial < kShortRow ? 1 : (spatial + kChunk - 1) / kChunk;
  if (rows > INT32_MAX || spatial > INT32_MAX || rows * cpr > INT32_MAX || rows > (INT64_MAX / 8) / spatial) {
    snprintf(msg, sizeof(msg), "%s: more than 2^31-1 rows, row elements or row chunks", who);
    return failm(GW_E_UNSUPPORTED, msg);
  }
  p.cpr = (int)cpr;
  p.units = rows * cpr;
  p.r_off = (size_t)2 * p.units * sizeof(double);
  p.bytes = p.r_off + (size_t)rows * sizeof(double);
  return GW_OK;
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

template <int MODE>
int launch_apply(const ApplyArgs& a, hipStream_t s) {
  if (a.groups / 256 >= INT32_MAX) return failm(GW_E_UNSUPPORTED, "gw_modulate: more than 2^41 elements");
  hipLaunchKernelGGL(apply_kernel<MODE>, dim3(blocks_of(a.groups, 256)), dim3(256), 0, s, a);
  return check_launch("apply_kernel launch");
}

template <int MODE>
int launch_reduce(const ReduceArgs& a, hipStream_t s) {
  if (a.spatial < kShortRow) {
    hipLaunchKernelGGL(reduce_row_kernel<MODE>, dim3(blocks_of(a.rows, 256)), dim3(256), 0, s, a);
    return check_launch("reduce_row_kernel launch");
  }
  hipLaunchKernelGGL(reduce_wave_kernel<MODE>, dim3(blocks_of(a.units, 4)), dim3(256), 0, s, a);
  return check_launch("reduce_wave_kernel launch");
}

}  // namespace

extern "C" {

size_t gw_modulate_workspace_bytes(int64_t rows, int64_t spatial) {
  Plan p;
  if (plan_of(rows, spatial, p, "gw_modulate_workspace_bytes") != GW_OK) return 0;
  return p.bytes;
}

int gw_sdl_forward(int64_t rows, int32_t channels, int64_t spatial, const float* x, const float* style, const float* alpha,
                   const uint32_t* key, const float* noise, float* out, void* stream) {
  Plan p;
  int rc = plan_of(rows, spatial, p, "gw_sdl_forward");
  if (rc != GW_OK) return rc;
  const bool raw = !x && !style && !alpha;  // out = the noise itself
  if (!out || channels <= 0 || rows % channels || (!key && !noise) || (raw ? !key : (!x || !style || !alpha)))
    return failm(GW_E_BADARG, "gw_sdl_forward: bad arguments");
  ApplyArgs a = {};
  a.n = rows * spatial;
  a.groups = (a.n + 3) / 4;
  a.spatial = spatial;
  a.channels = channels;
  a.x = x, a.a = style, a.b = alpha, a.key = key, a.noise = noise, a.out = out;
  hipStream_t s = (hipStream_t)stream;
  if (raw) return launch_apply<M_NOISE_ONLY>(a, s);
  return noise ? launch_apply<M_SDL_NOISE>(a, s) : launch_apply<M_SDL_KEY>(a, s);
}

int gw_sdl_backward(int64_t rows, int32_t channels, int64_t spatial, const float* dy, const float* style, const float* alpha,
                    const uint32_t* key, const float* noise, void* workspace, size_t workspace_bytes, float* d_style,
                    float* d_alpha, void* stream) {
  Plan p;
  int rc = plan_of(rows, spatial, p, "gw_sdl_backward");
  if (rc != GW_OK) return rc;
  if (!dy || channels <= 0 || rows % channels || (!key && !noise) || (d_style && !alpha) || (d_alpha && !style))
    return failm(GW_E_BADARG, "gw_sdl_backward: bad arguments");
  if (!workspace || workspace_bytes < p.bytes)
    return failm(GW_E_BADARG, "gw_sdl_backward: workspace smaller than gw_modulate_workspace_bytes");
  if (!d_style && !d_alpha) return GW_OK;
  hipStream_t s = (hipStream_t)stream;
  ReduceArgs a = {};
  a.rows = rows, a.spatial = spatial, a.units = p.units, a.chunks_per_row = p.cpr;
  a.dy = dy, a.key = key, a.noise = noise, a.part = (double*)workspace;
  rc = noise ? launch_reduce<M_SDL_NOISE>(a, s) : launch_reduce<M_SDL_KEY>(a, s);
  if (rc != GW_OK) return rc;
  double* R = (double*)((char*)workspace + p.r_off);
  hipLaunchKernelGGL(sdl_final_kernel, dim3(blocks_of(rows, 256)), dim3(256), 0, s, rows, channels, p.cpr, a.part, alpha, R, d_style);
  if ((rc = check_launch("sdl_final_kernel launch")) != GW_OK) return rc;
  if (!d_alpha) return GW_OK;
  hipLaunchKernelGGL(sdl_alpha_kernel, dim3(blocks_of(channels, 256)), dim3(256), 0, s, rows, channels, R, style, d_alpha);
  return check_launch("sdl_alpha_kernel launch");
}

int gw_film_forward(int64_t rows, int64_t spatial, const float* x, const float* gamma, const float* beta, float* out, void* stream) {
  Plan p;
  int rc = plan_of(rows, spatial, p, "gw_film_forward");
  if (rc != GW_OK) return rc;
  if (!x || !gamma || !beta || !out) return failm(GW_E_BADARG, "gw_film_forward: bad arguments");
  ApplyArgs a = {};
  a.n = rows * spatial;
  a.groups = (a.n + 3) / 4;
  a.spatial = spatial;
  a.channels = 1;
  a.x = x, a.a = gamma, a.b = beta, a.out = out;
  return launch_apply<M_FILM>(a, (hipStream_t)stream);
}

int gw_film_backward(int64_t rows, int64_t spatial, const float* dy, const float* x, const float* gamma, void* workspace,
                     size_t workspace_bytes, float* dx, float* d_gamma, float* d_beta, void* stream) {
  Plan p;
  int rc = plan_of(rows, spatial, p, "gw_film_backward");
  if (rc != GW_OK) return rc;
  if (!dy || (dx && !gamma) || (d_gamma && !x)) return failm(GW_E_BADARG, "gw_film_backward: bad arguments");
  if (!workspace || workspace_bytes < p.bytes)
    return failm(GW_E_BADARG, "gw_film_backward: workspace smaller than gw_modulate_workspace_bytes");
  if (!dx && !d_gamma && !d_beta) return GW_OK;
  hipStream_t s = (hipStream_t)stream;
  ReduceArgs a = {};
  a.rows = rows, a.spatial = spatial, a.units = p.units, a.chunks_per_row = p.cpr;
  a.dy = dy, a.x = d_gamma ? x : nullptr, a.gamma = gamma, a.dx = dx, a.part = (double*)workspace;
  if ((rc = launch_reduce<M_FILM>(a, s)) != GW_OK) return rc;
  if (!d_gamma && !d_beta) return GW_OK;
  hipLaunchKernelGGL(film_final_kernel, dim3(blocks_of(rows, 256)), dim3(256), 0, s, rows, p.units, p.cpr, a.part, d_gamma, d_beta);
  return check_launch("film_final_kernel launch");
}

}  // extern "C"
