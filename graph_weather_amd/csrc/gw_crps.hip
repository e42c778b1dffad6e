// gw_crps.hip - EnsembleCRPSLoss: the (almost) fair continuous ranked probability score of an ensemble against the truth.
//
// pred [B, N, lon, lat, C] (FGN's output layout), target [B, lon, lat, C], both dense fp32.  At one (sample, grid point, feature)
//   v = (1/N) sum_i |x_i - y| - 2 c2 sum_{i<j} |x_i - x_j|,   c2 = alpha / (2 N (N-1)) + (1 - alpha) / (2 N^2)   (0 at N = 1)
//   dv/dx_i = (1/N) sign(x_i - y) - 2 c2 sum_j sign(x_i - x_j),   sign(0) = 0
// and the loss is w v with w = aw[lat] fw[feature] (each optional): its mean over B lon lat C, or the field itself.
//
//   crps_fwd_kernel<N, VEC>   one work item per target element e = b G C + r (G = lon lat): member i lies at pred[(b N + i) G C + r],
//                             so every member is one coalesced stream.  The N values stay in registers (N <= kCrpsRegMax) and are
//                             read once.  VEC: four elements per thread through 16-byte loads (G C a multiple of 4 and 16-byte
//                             aligned pointers); otherwise one element per thread.  fp32 on direct differences (__f*_rn), sum_i in
//                             member order, sum_{i<j} in (i, j) order: an element's value does not depend on the path or its place.
//   crps_fwd_any_kernel       any N up to 1024: x_i in a register, x_j re-read through the cache (N^2 / 2 loads per element), the two
//                             sums of up to 523 776 fp32 differences carried in fp64.  A coverage path, not a tuned one.
//   A workgroup owns a slab of kCrpsSlab elements of ONE sample (slabs do not cross samples: 32-bit index arithmetic only).
//   "mean": the slab's sum in fp64 goes to part[slab]; crps_final_kernel (one workgroup) adds the slabs as a fixed-shape tree.
//   "none": the same per-point code stores w v.
//   crps_bwd_kernel<N, VEC> / crps_bwd_any_kernel   recompute the signs from pred and target; the pairwise signs are counted as
//                             integers (exact), dpred_i = g w ((1/N) sign(x_i - y) - 2 c2 count_i) with g = dout[0] / n ("mean") or
//                             dout[e] ("none").  Plain stores.
// No atomics, no host reads: equal inputs give bitwise equal results, and both directions can be captured in a graph.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gw_amd.h"
#include "gw_internal.hpp"

using namespace gw;

namespace {

int failf(int code, const char* msg) { return set_error(code, msg); }

constexpr int kCrpsSlab = 4096;    // elements of one sample per workgroup (16 per thread)
constexpr int kCrpsRegMax = 16;    // ensemble sizes up to this keep the members in registers
constexpr int kCrpsMaxMembers = 1024;

struct CrpsArgs {
  int nlat, nvar;
  unsigned per_sample;       // G C
  unsigned slabs_per_sample;
  int members;               // read by the *_any kernels only
  float inv_n, two_c2;
  const float* pred;
  const float* target;
  const float* aw;           // [nlat] or NULL
  const float* fw;           // [nvar] or NULL
};

__device__ __forceinline__ float sign_of(float a, float b) { return (float)((a > b) - (a < b)); }

// v of one point from its N members in registers
template <int N>
__device__ __forceinline__ float crps_point(const float (&x)[N], float y, float inv_n, float two_c2) {
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) s1 = __fadd_rn(s1, fabsf(__fsub_rn(x[i], y)));
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = i + 1; j < N; ++j) s2 = __fadd_rn(s2, fabsf(__fsub_rn(x[i], x[j])));
  return __fsub_rn(__fmul_rn(inv_n, s1), __fmul_rn(two_c2, s2));
}

// x_i <- gw dv/dx_i, in place
template <int N>
__device__ __forceinline__ void crps_point_grad(float (&x)[N], float y, float inv_n, float two_c2, float gw) {
  int cnt[N];
#pragma unroll
  for (int i = 0; i < N; ++i) cnt[i] = 0;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = i + 1; j < N; ++j) {
      const int s = (x[i] > x[j]) - (x[i] < x[j]);
      cnt[i] += s;
      cnt[j] -= s;
    }
#pragma unroll
  for (int i = 0; i < N; ++i)
    x[i] = __fmul_rn(gw, __fsub_rn(__fmul_rn(inv_n, sign_of(x[i], y)), __fmul_rn(two_c2, (float)cnt[i])));
}

// (lat, feature) of element r of a sample, and the step to the next element
struct Where {
  int lat, var;
  __device__ __forceinline__ Where(unsigned r, int nlat, int nvar, bool wanted) : lat(0), var(0) {
    if (wanted) {
      const unsigned row = r / (unsigned)nvar;
      var = (int)(r - row * (unsigned)nvar);
      lat = (int)(row % (unsigned)nlat);
    }
  }
  __device__ __forceinline__ void next(int nlat, int nvar) {
    if (++var == nvar) {
      var = 0;
      if (++lat == nlat) lat = 0;
    }
  }
  __device__ __forceinline__ float weight(const float* __restrict__ aw, const float* __restrict__ fw) const {
    float w = 1.f;
    if (aw) w = aw[lat];
    if (fw) w = __fmul_rn(w, fw[var]);
    return w;
  }
};

__device__ __forceinline__ void slab_sum(double s, double* __restrict__ part) {
  __shared__ double red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// part != NULL: "mean" (the slab's sum), else out [B, G C] gets the field
template <int N, bool VEC>
__global__ __launch_bounds__(256) void crps_fwd_kernel(CrpsArgs a, double* __restrict__ part, float* __restrict__ out) {
  constexpr int W = VEC ? 4 : 1;
  const unsigned b = blockIdx.x / a.slabs_per_sample, slab = blockIdx.x - b * a.slabs_per_sample;
  const size_t gc = a.per_sample;
  const float* __restrict__ xp = a.pred + (size_t)b * N * gc;
  const float* __restrict__ tp = a.target + (size_t)b * gc;
  const bool weighted = a.aw != nullptr || a.fw != nullptr;
  double s = 0.0;
  for (int it = 0; it < kCrpsSlab / (256 * W); ++it) {
    const unsigned r = slab * (unsigned)kCrpsSlab + (unsigned)(it * 256 + threadIdx.x) * W;
    if (r >= a.per_sample) break;
    float x[W][N], y[W], v[W];
    if constexpr (VEC) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float4 t = *(const float4*)(xp + (size_t)i * gc + r);
        x[0][i] = t.x, x[1][i] = t.y, x[2][i] = t.z, x[3][i] = t.w;
      }
      const float4 t = *(const float4*)(tp + r);
      y[0] = t.x, y[1] = t.y, y[2] = t.z, y[3] = t.w;
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) x[0][i] = xp[(size_t)i * gc + r];
      y[0] = tp[r];
    }
    Where at(r, a.nlat, a.nvar, weighted);
#pragma unroll
    for (int c = 0; c < W; ++c) {
      v[c] = crps_point<N>(x[c], y[c], a.inv_n, a.two_c2);
      if (weighted) {
        v[c] = __fmul_rn(at.weight(a.aw, a.fw), v[c]);
        at.next(a.nlat, a.nvar);
      }
      s += (double)v[c];
    }
    if (part == nullptr) {
      float* o = out + (size_t)b * gc + r;
      if constexpr (VEC) {
        *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        *o = v[0];
      }
    }
  }
  if (part != nullptr) slab_sum(s, part);
}

__global__ __launch_bounds__(256) void crps_fwd_any_kernel(CrpsArgs a, double* __restrict__ part, float* __restrict__ out) {
  const unsigned b = blockIdx.x / a.slabs_per_sample, slab = blockIdx.x - b * a.slabs_per_sample;
  const size_t gc = a.per_sample;
  const int n = a.members;
  const float* __restrict__ xp = a.pred + (size_t)b * n * gc;
  const float* __restrict__ tp = a.target + (size_t)b * gc;
  const bool weighted = a.aw != nullptr || a.fw != nullptr;
  double s = 0.0;
  for (int it = 0; it < kCrpsSlab / 256; ++it) {
    const unsigned r = slab * (unsigned)kCrpsSlab + (unsigned)(it * 256 + threadIdx.x);
    if (r >= a.per_sample) break;
    const float y = tp[r];
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < n; ++i) {
      const float xi = xp[(size_t)i * gc + r];
      s1 += (double)fabsf(__fsub_rn(xi, y));
      for (int j = i + 1; j < n; ++j) s2 += (double)fabsf(__fsub_rn(xi, xp[(size_t)j * gc + r]));
    }
    float v = __fsub_rn(__fmul_rn(a.inv_n, (float)s1), __fmul_rn(a.two_c2, (float)s2));
    if (weighted) v = __fmul_rn(Where(r, a.nlat, a.nvar, true).weight(a.aw, a.fw), v);
    s += (double)v;
    if (part == nullptr) out[(size_t)b * gc + r] = v;
  }
  if (part != nullptr) slab_sum(s, part);
}

// one workgroup: loss = sum of the slabs' sums / n
__global__ __launch_bounds__(256) void crps_final_kernel(long long slabs, long long n, const double* __restrict__ part,
                                                         float* __restrict__ loss) {
  __shared__ double red[256];
  double s = 0.0;
  for (long long i = threadIdx.x; i < slabs; i += 256) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(red[0] / (double)n);
}

// field: dout is [B, G C] ("none"), else dout[0] is the gradient of the mean over n elements
template <int N, bool VEC>
__global__ __launch_bounds__(256) void crps_bwd_kernel(CrpsArgs a, const float* __restrict__ dout, int field, long long n_total,
                                                       float* __restrict__ dpred) {
  constexpr int W = VEC ? 4 : 1;
  const unsigned b = blockIdx.x / a.slabs_per_sample, slab = blockIdx.x - b * a.slabs_per_sample;
  const size_t gc = a.per_sample;
  const float* __restrict__ xp = a.pred + (size_t)b * N * gc;
  const float* __restrict__ tp = a.target + (size_t)b * gc;
  float* __restrict__ dp = dpred + (size_t)b * N * gc;
  const bool weighted = a.aw != nullptr || a.fw != nullptr;
  const float g_mean = field ? 0.f : (float)((double)dout[0] / (double)n_total);
  for (int it = 0; it < kCrpsSlab / (256 * W); ++it) {
    const unsigned r = slab * (unsigned)kCrpsSlab + (unsigned)(it * 256 + threadIdx.x) * W;
    if (r >= a.per_sample) break;
    float x[W][N], y[W], g[W];
#pragma unroll
    for (int c = 0; c < W; ++c) g[c] = g_mean;
    if constexpr (VEC) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float4 t = *(const float4*)(xp + (size_t)i * gc + r);
        x[0][i] = t.x, x[1][i] = t.y, x[2][i] = t.z, x[3][i] = t.w;
      }
      const float4 t = *(const float4*)(tp + r);
      y[0] = t.x, y[1] = t.y, y[2] = t.z, y[3] = t.w;
      if (field) {
        const float4 d = *(const float4*)(dout + (size_t)b * gc + r);
        g[0] = d.x, g[1] = d.y, g[2] = d.z, g[3] = d.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) x[0][i] = xp[(size_t)i * gc + r];
      y[0] = tp[r];
      if (field) g[0] = dout[(size_t)b * gc + r];
    }
    Where at(r, a.nlat, a.nvar, weighted);
#pragma unroll
    for (int c = 0; c < W; ++c) {
      float gw = g[c];
      if (weighted) {
        gw = __fmul_rn(gw, at.weight(a.aw, a.fw));
        at.next(a.nlat, a.nvar);
      }
      crps_point_grad<N>(x[c], y[c], a.inv_n, a.two_c2, gw);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float* o = dp + (size_t)i * gc + r;
      if constexpr (VEC) {
        *(float4*)o = make_float4(x[0][i], x[1][i], x[2][i], x[3][i]);
      } else {
        *o = x[0][i];
      }
    }
  }
}

__global__ __launch_bounds__(256) void crps_bwd_any_kernel(CrpsArgs a, const float* __restrict__ dout, int field, long long n_total,
                                                           float* __restrict__ dpred) {
  const unsigned b = blockIdx.x / a.slabs_per_sample, slab = blockIdx.x - b * a.slabs_per_sample;
  const size_t gc = a.per_sample;
  const int n = a.members;
  const float* __restrict__ xp = a.pred + (size_t)b * n * gc;
  const float* __restrict__ tp = a.target + (size_t)b * gc;
  float* __restrict__ dp = dpred + (size_t)b * n * gc;
  const bool weighted = a.aw != nullptr || a.fw != nullptr;
  const float g_mean = field ? 0.f : (float)((double)dout[0] / (double)n_total);
  for (int it = 0; it < kCrpsSlab / 256; ++it) {
    const unsigned r = slab * (unsigned)kCrpsSlab + (unsigned)(it * 256 + threadIdx.x);
    if (r >= a.per_sample) break;
    const float y = tp[r];
    float gw = field ? dout[(size_t)b * gc + r] : g_mean;
    if (weighted) gw = __fmul_rn(gw, Where(r, a.nlat, a.nvar, true).weight(a.aw, a.fw));
    for (int i = 0; i < n; ++i) {
      const float xi = xp[(size_t)i * gc + r];
      int cnt = 0;
      for (int j = 0; j < n; ++j) {
        const float xj = xp[(size_t)j * gc + r];
        cnt += (xi > xj) - (xi < xj);
      }
      dp[(size_t)i * gc + r] = __fmul_rn(gw, __fsub_rn(__fmul_rn(a.inv_n, sign_of(xi, y)), __fmul_rn(a.two_c2, (float)cnt)));
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
bool crps_shape_ok(int32_t batch, int32_t members, int32_t nlon, int32_t nlat, int32_t nvar) {
  return batch >= 1 && members >= 1 && members <= kCrpsMaxMembers && nlon >= 1 && nlat >= 1 && nvar >= 1;
}

// elements of one sample (G C); 0 when they or the slab count leave the 31-bit range of the kernels' index arithmetic
long long crps_per_sample(int32_t batch, int32_t nlon, int32_t nlat, int32_t nvar) {
  const long long g = (long long)nlon * nlat;
  if (g > INT32_MAX) return 0;
  const long long gc = g * nvar;  // < 2^62
  if (gc > INT32_MAX - kCrpsSlab) return 0;
  const long long sps = (gc + kCrpsSlab - 1) / kCrpsSlab;
  if (sps * batch > INT32_MAX) return 0;
  return gc;
}

bool crps_fill(CrpsArgs& a, int32_t batch, int32_t members, int32_t nlon, int32_t nlat, int32_t nvar, double alpha, const float* pred,
               const float* target, const float* aw, const float* fw) {
  const long long gc = crps_per_sample(batch, nlon, nlat, nvar);
  if (!gc) return false;
  const double n = (double)members;
  const double c2 = members > 1 ? alpha / (2.0 * n * (n - 1.0)) + (1.0 - alpha) / (2.0 * n * n) : 0.0;
  a.nlat = nlat, a.nvar = nvar;
  a.per_sample = (unsigned)gc;
  a.slabs_per_sample = (unsigned)((gc + kCrpsSlab - 1) / kCrpsSlab);
  a.members = members;
  a.inv_n = (float)(1.0 / n), a.two_c2 = (float)(2.0 * c2);
  a.pred = pred, a.target = target, a.aw = aw, a.fw = fw;
  return true;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define GW_CRPS_CASE(KERNEL, NN, ...)                                                                        \
  case NN:                                                                                                   \
    if (vec)                                                                                                 \
      hipLaunchKernelGGL((KERNEL<NN, true>), dim3(grid), dim3(256), 0, st, __VA_ARGS__);                     \
    else                                                                                                     \
      hipLaunchKernelGGL((KERNEL<NN, false>), dim3(grid), dim3(256), 0, st, __VA_ARGS__);                    \
    break;
#define GW_CRPS_DISPATCH(KERNEL, ...)                                                                        \
  switch (members) {                                                                                         \
    GW_CRPS_CASE(KERNEL, 1, __VA_ARGS__) GW_CRPS_CASE(KERNEL, 2, __VA_ARGS__) GW_CRPS_CASE(KERNEL, 3, __VA_ARGS__)    \
    GW_CRPS_CASE(KERNEL, 4, __VA_ARGS__) GW_CRPS_CASE(KERNEL, 5, __VA_ARGS__) GW_CRPS_CASE(KERNEL, 6, __VA_ARGS__)    \
    GW_CRPS_CASE(KERNEL, 7, __VA_ARGS__) GW_CRPS_CASE(KERNEL, 8, __VA_ARGS__) GW_CRPS_CASE(KERNEL, 9, __VA_ARGS__)    \
    GW_CRPS_CASE(KERNEL, 10, __VA_ARGS__) GW_CRPS_CASE(KERNEL, 11, __VA_ARGS__) GW_CRPS_CASE(KERNEL, 12, __VA_ARGS__) \
    GW_CRPS_CASE(KERNEL, 13, __VA_ARGS__) GW_CRPS_CASE(KERNEL, 14, __VA_ARGS__) GW_CRPS_CASE(KERNEL, 15, __VA_ARGS__) \
    GW_CRPS_CASE(KERNEL, 16, __VA_ARGS__)                                                                    \
  }

static_assert(kCrpsRegMax == 16, "GW_CRPS_DISPATCH lists the register-resident ensemble sizes");

}  // namespace

extern "C" {

size_t gw_ensemble_crps_workspace_bytes(int32_t batch, int32_t members, int32_t nlon, int32_t nlat, int32_t nvar) {
  const long long gc = crps_shape_ok(batch, members, nlon, nlat, nvar) ? crps_per_sample(batch, nlon, nlat, nvar) : 0;
  if (!gc) {
    failf(GW_E_BADARG, "gw_ensemble_crps_workspace_bytes: bad arguments");
    return 0;
  }
  return (size_t)(((gc + kCrpsSlab - 1) / kCrpsSlab) * batch) * sizeof(double);
}

int gw_ensemble_crps_forward(int32_t batch, int32_t members, int32_t nlon, int32_t nlat, int32_t nvar, double alpha, int32_t reduction,
                             const float* pred, const float* target, const float* area_weights, const float* features_weights,
                             void* workspace, size_t workspace_bytes, float* out, void* stream) {
  if (!crps_shape_ok(batch, members, nlon, nlat, nvar) || !pred || !target || !out || !(alpha >= 0.0 && alpha <= 1.0) ||
      (members == 1 && alpha > 0.0) || (reduction != GW_CRPS_MEAN && reduction != GW_CRPS_NONE))
    return failf(GW_E_BADARG, "gw_ensemble_crps_forward: bad arguments");
  CrpsArgs a;
  if (!crps_fill(a, batch, members, nlon, nlat, nvar, alpha, pred, target, area_weights, features_weights))
    return failf(GW_E_UNSUPPORTED, "gw_ensemble_crps_forward: shape too large");
  const long long slabs = (long long)a.slabs_per_sample * batch;
  const bool mean = reduction == GW_CRPS_MEAN;
  if (mean && (!workspace || workspace_bytes < (size_t)slabs * sizeof(double)))
    return failf(GW_E_BADARG, "gw_ensemble_crps_forward: bad arguments (workspace)");
  double* part = mean ? (double*)workspace : nullptr;
  float* field = mean ? nullptr : out;
  const bool vec = a.per_sample % 4 == 0 && aligned16(pred) && aligned16(target) && (mean || aligned16(out));
  const unsigned grid = (unsigned)slabs;
  hipStream_t st = (hipStream_t)stream;
  if (members <= kCrpsRegMax) {
    GW_CRPS_DISPATCH(crps_fwd_kernel, a, part, field)
  } else {
    hipLaunchKernelGGL(crps_fwd_any_kernel, dim3(grid), dim3(256), 0, st, a, part, field);
  }
  if (int rc = check_launch("crps_fwd_kernel launch")) return rc;
  if (!mean) return GW_OK;
  hipLaunchKernelGGL(crps_final_kernel, dim3(1), dim3(256), 0, st, slabs, (long long)a.per_sample * batch, (const double*)part, out);
  return check_launch("crps_final_kernel launch");
}

int gw_ensemble_crps_backward(int32_t batch, int32_t members, int32_t nlon, int32_t nlat, int32_t nvar, double alpha, int32_t reduction,
                              const float* pred, const float* target, const float* area_weights, const float* features_weights,
                              const float* dout, float* dpred, void* stream) {
  if (!crps_shape_ok(batch, members, nlon, nlat, nvar) || !pred || !target || !dout || !dpred || !(alpha >= 0.0 && alpha <= 1.0) ||
      (members == 1 && alpha > 0.0) || (reduction != GW_CRPS_MEAN && reduction != GW_CRPS_NONE))
    return failf(GW_E_BADARG, "gw_ensemble_crps_backward: bad arguments");
  CrpsArgs a;
  if (!crps_fill(a, batch, members, nlon, nlat, nvar, alpha, pred, target, area_weights, features_weights))
    return failf(GW_E_UNSUPPORTED, "gw_ensemble_crps_backward: shape too large");
  const int field = reduction == GW_CRPS_NONE;
  const bool vec = a.per_sample % 4 == 0 && aligned16(pred) && aligned16(target) && aligned16(dpred) && (!field || aligned16(dout));
  const unsigned grid = a.slabs_per_sample * (unsigned)batch;
  const long long n_total = (long long)a.per_sample * batch;
  hipStream_t st = (hipStream_t)stream;
  if (members <= kCrpsRegMax) {
    GW_CRPS_DISPATCH(crps_bwd_kernel, a, dout, field, n_total, dpred)
  } else {
    hipLaunchKernelGGL(crps_bwd_any_kernel, dim3(grid), dim3(256), 0, st, a, dout, field, n_total, dpred);
  }
  return check_launch("crps_bwd_kernel launch");
}

}  // extern "C"
