// gw_genda.hip - the two row kernels that frame GenDA's forward and its one-pass classifier-free guidance
// (graph_weather/models/genda/model.py of the reference).
//
// GenDA is the GenCast Denoiser with up to two extra grid columns (a sensor mask and sensor values).  ``guided_forward`` evaluates
// the model on the same Z, X and sigma with the conditioning (copy 0) and with zero conditioning (copy 1) and combines the two
// outputs; here both evaluations are ONE pass at batch 2 B over one graph, copy k of sample b in the rows of sample k B + b.
//
//   genda_in_fwd_kernel   one wave per SOURCE row r = b G + g: it reads z[r], x[r], the conditioning columns and stat[g] once and
//                         writes (c_in(sigma_b) z | x | c0 | c1 | stat) to row r and, with two copies, the same with zero
//                         conditioning to row (B + b) G + g.  `drop` (the training-time conditioning dropout, a host decision)
//                         writes zeros in copy 0 too and reads no conditioning.  c_noise[k B + b] from the wave of the sample's
//                         first row.  With one copy and no conditioning this is precond_in_fwd_kernel of gw_gencast.hip, value
//                         for value: the same float32 operations in the same order.
//   genda_in_bwd_kernel   dz = c_in (d_copy0 + d_copy1), dx = d_copy0 + d_copy1 (copies added in copy order), the conditioning
//                         gradients from copy 0 only (zeros with `drop`: the columns did not depend on their inputs).
//   genda_out_fwd_kernel  o_c = c_skip z + c_out p_c, o_u = c_skip z + c_out p_u, out = o_u + gamma (o_c - o_u) per element, in the
//                         reference's order of operations (no fused multiply-add).
//   genda_out_bwd_kernel  dp_c = c_out (gamma dout), dp_u = c_out ((1 - gamma) dout), dz = c_skip dout.
//
// The kernels keep the shape of the Denoiser's preconditioning kernels: one wave per row, four rows per 256-thread workgroup, 64-bit
// row offsets.  fp32, plain stores, no atomics, no host reads: equal inputs give bitwise equal results and every call can be
// captured in a graph.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gw_amd.h"
#include "gw_device.hpp"
#include "gw_internal.hpp"

using namespace gw;

namespace {

int failf(int code, const char* msg) { return set_error(code, msg); }

// the coefficients as gw_gencast.hip forms them (float32, the reference's order of operations; d2 = sigma_data^2 from the host)
__device__ __forceinline__ float genda_var(float s, float d2) { return __fadd_rn(__fmul_rn(s, s), d2); }
__device__ __forceinline__ float genda_c_in(float s, float d2) { return __fdiv_rn(1.0f, __fsqrt_rn(genda_var(s, d2))); }
__device__ __forceinline__ float genda_c_skip(float s, float d2) { return __fdiv_rn(d2, genda_var(s, d2)); }
__device__ __forceinline__ float genda_c_out(float s, float d, float d2) {
  return __fdiv_rn(__fmul_rn(s, d), __fsqrt_rn(genda_var(s, d2)));
}

struct InArgs {
  long long rows, grid_rows;  // source rows B G; G
  int batch, copies, drop, wz, wx, nc, ws;
  float d2;
  const float* sigma;
  const float* z;
  long long ld_z;
  const float* x;
  long long ld_x;
  const float* c[2];  // the nc conditioning columns in output order, one float per source row
  long long ld_c[2];
  const float* stat;
  long long ld_s;
};

__global__ __launch_bounds__(256) void genda_in_fwd_kernel(InArgs a, float* __restrict__ out, long long ld_o, float* __restrict__ c_noise) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.rows) return;
  const long long b = r / a.grid_rows, g = r - b * a.grid_rows;
  const float s = a.sigma[b], cin = genda_c_in(s, a.d2);
  const int c0 = a.wz + a.wx, s0 = c0 + a.nc;
  float* o0 = out + r * ld_o;
  float* o1 = out + (a.rows + r) * ld_o;  // (written with two copies only)
  const bool two = a.copies == 2;
  for (int c = lane; c < a.wz; c += 64) {
    const float v = __fmul_rn(cin, ldg1(a.z + r * a.ld_z + c));
    stg1(o0 + c, v);
    if (two) stg1(o1 + c, v);
  }
  for (int c = lane; c < a.wx; c += 64) {
    const float v = ldg1(a.x + r * a.ld_x + c);
    stg1(o0 + a.wz + c, v);
    if (two) stg1(o1 + a.wz + c, v);
  }
  if (lane < a.nc) {
    const float* col = lane == 0 ? a.c[0] : a.c[1];
    const long long ld = lane == 0 ? a.ld_c[0] : a.ld_c[1];
    const float v = a.drop ? 0.f : ldg1(col + r * ld);
    stg1(o0 + c0 + lane, v);
    if (two) stg1(o1 + c0 + lane, 0.f);
  }
  for (int c = lane; c < a.ws; c += 64) {
    const float v = ldg1(a.stat + g * a.ld_s + c);
    stg1(o0 + s0 + c, v);
    if (two) stg1(o1 + s0 + c, v);
  }
  if (g == 0 && lane == 0 && c_noise != nullptr) {
    const float v = __fmul_rn(0.25f, logf(s));
    c_noise[b] = v;
    if (two) c_noise[a.batch + b] = v;
  }
}

// dout [copies B G, wz + wx + nc + ...]; dz, dx, dc[j] each may be NULL
__global__ __launch_bounds__(256) void genda_in_bwd_kernel(long long rows, long long grid_rows, int copies, int drop, int wz, int wx, int nc,
                                                           float d2, const float* __restrict__ sigma, const float* __restrict__ dout,
                                                           long long ld_do, float* __restrict__ dz, long long ld_dz,
                                                           float* __restrict__ dx, long long ld_dx, float* __restrict__ dc0,
                                                           long long ld_dc0, float* __restrict__ dc1, long long ld_dc1) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float cin = genda_c_in(sigma[r / grid_rows], d2);
  const float* g0 = dout + r * ld_do;
  const float* g1 = dout + (rows + r) * ld_do;  // (read with two copies only)
  const bool two = copies == 2;
  if (dz != nullptr)
    for (int c = lane; c < wz; c += 64) {
      float v = ldg1(g0 + c);
      if (two) v = __fadd_rn(v, ldg1(g1 + c));
      stg1(dz + r * ld_dz + c, __fmul_rn(cin, v));
    }
  if (dx != nullptr)
    for (int c = lane; c < wx; c += 64) {
      float v = ldg1(g0 + wz + c);
      if (two) v = __fadd_rn(v, ldg1(g1 + wz + c));
      stg1(dx + r * ld_dx + c, v);
    }
  if (lane < nc) {
    float* d = lane == 0 ? dc0 : dc1;
    const long long ld = lane == 0 ? ld_dc0 : ld_dc1;
    if (d != nullptr) stg1(d + r * ld, drop ? 0.f : ldg1(g0 + wz + wx + lane));
  }
}

// out[r] = o_u + gamma (o_c - o_u), o_k = c_skip(sigma_b) z[r] + c_out(sigma_b) p[k rows + r]
__global__ __launch_bounds__(256) void genda_out_fwd_kernel(long long rows, long long grid_rows, int width, float d, float d2, float gamma,
                                                            const float* __restrict__ sigma, const float* __restrict__ z, long long ld_z,
                                                            const float* __restrict__ p, long long ld_p, float* __restrict__ out,
                                                            long long ld_o) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float s = sigma[r / grid_rows], cs = genda_c_skip(s, d2), co = genda_c_out(s, d, d2);
  for (int c = lane; c < width; c += 64) {
    const float skip = __fmul_rn(cs, ldg1(z + r * ld_z + c));
    const float oc = __fadd_rn(skip, __fmul_rn(co, ldg1(p + r * ld_p + c)));
    const float ou = __fadd_rn(skip, __fmul_rn(co, ldg1(p + (rows + r) * ld_p + c)));
    stg1(out + r * ld_o + c, __fadd_rn(ou, __fmul_rn(gamma, __fsub_rn(oc, ou))));
  }
}

// dz[r] = c_skip dout[r]; dp[r] = c_out (gamma dout[r]), dp[rows + r] = c_out (omg dout[r]), omg = 1 - gamma (each of dz, dp may be NULL)
__global__ __launch_bounds__(256) void genda_out_bwd_kernel(long long rows, long long grid_rows, int width, float d, float d2, float gamma,
                                                            float omg, const float* __restrict__ sigma, const float* __restrict__ dout,
                                                            long long ld_do, float* __restrict__ dz, long long ld_dz,
                                                            float* __restrict__ dp, long long ld_dp) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float s = sigma[r / grid_rows], cs = genda_c_skip(s, d2), co = genda_c_out(s, d, d2);
  for (int c = lane; c < width; c += 64) {
    const float g = ldg1(dout + r * ld_do + c);
    if (dz != nullptr) stg1(dz + r * ld_dz + c, __fmul_rn(cs, g));
    if (dp != nullptr) {
      stg1(dp + r * ld_dp + c, __fmul_rn(co, __fmul_rn(gamma, g)));
      stg1(dp + (rows + r) * ld_dp + c, __fmul_rn(co, __fmul_rn(omg, g)));
    }
  }
}

// `copies` row sets of batch * grid_rows rows each; the launch takes one wave per row of ONE set
bool genda_ok(int32_t batch, int64_t grid_rows, int32_t copies, float sigma_data) {
  return batch >= 1 && grid_rows >= 1 && (copies == 1 || copies == 2) && (int64_t)batch * grid_rows < ((int64_t)1 << 32) && sigma_data > 0.f &&
         !(sigma_data != sigma_data);
}

unsigned row_blocks(long long rows) { return (unsigned)((rows + 3) / 4); }

}  // namespace

extern "C" {

int gw_genda_input_forward(int32_t batch, int64_t grid_rows, int32_t copies, int32_t drop, int32_t w_z, int32_t w_x, int32_t w_s,
                           float sigma_data, const float* sigma, const float* z, int32_t ld_z, const float* x, int32_t ld_x, const float* c0,
                           int32_t ld_c0, const float* c1, int32_t ld_c1, const float* stat, int32_t ld_stat, float* out, int32_t ld_out,
                           float* c_noise, void* stream) {
  const int nc = (c0 != nullptr) + (c1 != nullptr);
  if (!genda_ok(batch, grid_rows, copies, sigma_data) || (drop != 0 && drop != 1) || !sigma || !out || w_z < 0 || w_x < 0 || w_s < 0 ||
      (w_z && (!z || ld_z < w_z)) || (w_x && (!x || ld_x < w_x)) || (w_s && (!stat || ld_stat < w_s)) || (c0 && ld_c0 < 1) ||
      (c1 && ld_c1 < 1) || (int64_t)w_z + w_x + nc + w_s < 1 || ld_out < (int64_t)w_z + w_x + nc + w_s)
    return failf(GW_E_BADARG, "gw_genda_input_forward: bad arguments");
  InArgs a;
  a.rows = (long long)batch * grid_rows, a.grid_rows = grid_rows;
  a.batch = batch, a.copies = copies, a.drop = drop, a.wz = w_z, a.wx = w_x, a.nc = nc, a.ws = w_s;
  a.d2 = (float)((double)sigma_data * sigma_data);
  a.sigma = sigma, a.z = z, a.ld_z = ld_z, a.x = x, a.ld_x = ld_x, a.stat = stat, a.ld_s = ld_stat;
  a.c[0] = c0 ? c0 : c1, a.ld_c[0] = c0 ? ld_c0 : ld_c1;  // (the columns that are present, in order)
  a.c[1] = c1, a.ld_c[1] = ld_c1;
  hipLaunchKernelGGL(genda_in_fwd_kernel, dim3(row_blocks(a.rows)), dim3(256), 0, (hipStream_t)stream, a, out, (long long)ld_out, c_noise);
  return check_launch("genda_in_fwd_kernel launch");
}

int gw_genda_input_backward(int32_t batch, int64_t grid_rows, int32_t copies, int32_t drop, int32_t w_z, int32_t w_x, int32_t n_cond,
                            float sigma_data, const float* sigma, const float* dout, int32_t ld_dout, float* dz, int32_t ld_dz, float* dx,
                            int32_t ld_dx, float* dc0, int32_t ld_dc0, float* dc1, int32_t ld_dc1, void* stream) {
  if (!genda_ok(batch, grid_rows, copies, sigma_data) || (drop != 0 && drop != 1) || !sigma || !dout || (!dz && !dx && !dc0 && !dc1) ||
      w_z < 0 || w_x < 0 || n_cond < 0 || n_cond > 2 || ld_dout < (int64_t)w_z + w_x + n_cond || (dz && ld_dz < w_z) || (dx && ld_dx < w_x) ||
      (dc0 && (n_cond < 1 || ld_dc0 < 1)) || (dc1 && (n_cond < 2 || ld_dc1 < 1)))
    return failf(GW_E_BADARG, "gw_genda_input_backward: bad arguments");
  const long long rows = (long long)batch * grid_rows;
  hipLaunchKernelGGL(genda_in_bwd_kernel, dim3(row_blocks(rows)), dim3(256), 0, (hipStream_t)stream, rows, (long long)grid_rows, (int)copies,
                     (int)drop, (int)w_z, (int)w_x, (int)n_cond, (float)((double)sigma_data * sigma_data), sigma, dout, (long long)ld_dout, dz,
                     (long long)ld_dz, dx, (long long)ld_dx, dc0, (long long)ld_dc0, dc1, (long long)ld_dc1);
  return check_launch("genda_in_bwd_kernel launch");
}

int gw_genda_guided_output_forward(int32_t batch, int64_t grid_rows, int32_t width, float sigma_data, float gamma, const float* sigma,
                                   const float* z, int32_t ld_z, const float* preds, int32_t ld_preds, float* out, int32_t ld_out,
                                   void* stream) {
  if (!genda_ok(batch, grid_rows, 2, sigma_data) || gamma != gamma || !sigma || !z || !preds || !out || width < 1 || ld_z < width ||
      ld_preds < width || ld_out < width)
    return failf(GW_E_BADARG, "gw_genda_guided_output_forward: bad arguments");
  const long long rows = (long long)batch * grid_rows;
  hipLaunchKernelGGL(genda_out_fwd_kernel, dim3(row_blocks(rows)), dim3(256), 0, (hipStream_t)stream, rows, (long long)grid_rows, (int)width,
                     sigma_data, (float)((double)sigma_data * sigma_data), gamma, sigma, z, (long long)ld_z, preds, (long long)ld_preds, out,
                     (long long)ld_out);
  return check_launch("genda_out_fwd_kernel launch");
}

int gw_genda_guided_output_backward(int32_t batch, int64_t grid_rows, int32_t width, float sigma_data, float gamma, const float* sigma,
                                    const float* dout, int32_t ld_dout, float* dz, int32_t ld_dz, float* dpreds, int32_t ld_dpreds,
                                    void* stream) {
  if (!genda_ok(batch, grid_rows, 2, sigma_data) || gamma != gamma || !sigma || !dout || (!dz && !dpreds) || width < 1 || ld_dout < width ||
      (dz && ld_dz < width) || (dpreds && ld_dpreds < width))
    return failf(GW_E_BADARG, "gw_genda_guided_output_backward: bad arguments");
  const long long rows = (long long)batch * grid_rows;
  hipLaunchKernelGGL(genda_out_bwd_kernel, dim3(row_blocks(rows)), dim3(256), 0, (hipStream_t)stream, rows, (long long)grid_rows, (int)width,
                     sigma_data, (float)((double)sigma_data * sigma_data), gamma, (float)(1.0 - (double)gamma), sigma, dout,
                     (long long)ld_dout, dz, (long long)ld_dz, dpreds, (long long)ld_dpreds);
  return check_launch("genda_out_bwd_kernel launch");
}

}  // extern "C"
