// gw_constraint.hip - PhysicalConstraintLayer (graph_weather/models/layers/constraint_layer.py) behind the decoder of the
// forecaster (forecast.py:234-246).  The reference reshapes the decoder output into a grid and round-trips it through the
// Python loops graph_to_grid / grid_to_graph; that whole chain reduces to gathers through a node -> grid-row map (`map`,
// see include/gw_amd.h) plus per-(sample, channel) statistics.  Everything here is HBM-bound: no matrix cores.
//
//   stats_partial_kernel   per (b, c) and slab of rows: sum_k cnt(k) hr[k] (and lr), or sum_k G(k) (and G(k) hr[k]) with
//                          G(k) = sum of the output gradient over the nodes reading row k (CSR walk); fp64 partials
//   stats_final_kernel     sums the slab partials in one fixed order (no atomics: bitwise reproducible) -> per-(b, c) scalars
//   apply_kernel           out[b, n, c] from row map[n] of hr / lr and the scalars (softmax f > 1: the block ratios)
//   block_ratio_kernel     softmax f > 1: S = f x f block sum of exp(a hr) (as mean * f^2, like AvgPool2d * f^2), lr / S
//   backward_kernel        dhr (and dlr) per grid row, reading the output gradient through the CSR of map's inverse
//   block_backward_kernel  softmax f > 1: the per-block part of the backward (kron / pool / reciprocal), then backward_kernel

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gw_amd.h"
#include "gw_internal.hpp"

using namespace gw;

namespace {

int failc(int code, const char* msg) { return set_error(code, msg); }

constexpr int kSlabRows = 64;   // grid rows per statistics partial
constexpr int kRowGroups = 4;   // waves per statistics workgroup, each on every 4th row of the slab

// scalar slots of the statistics table st[kSlots][batch * C]
enum { ST_MEAN_HR = 0, ST_MEAN_LR, ST_RATIO, ST_MEAN_G, ST_Q_HR, ST_Q_LR, kSlots };
// partial sums part[kParts][batch][n_slabs][C]
enum { P_HR = 0, P_LR, P_G, P_GH, kParts };

__device__ inline float cell_grad(const float* __restrict__ g, int64_t gbase, int ld_g, const int* __restrict__ inv_ptr,
                                  const int* __restrict__ inv_idx, int k, int c) {
  float s = 0.f;
  for (int i = inv_ptr[k]; i < inv_ptr[k + 1]; ++i) s += g[gbase + (int64_t)inv_idx[i] * ld_g + c];
  return s;
}

// grid (n_slabs, batch * ctiles), block 256: lane -> channel of a 64-channel tile, wave -> row group.  Rows that no node reads
// are skipped, never read: an inf / NaN there must not reach the statistics (the reference's means only see read rows).
// bwd 0: part[P_HR] += cnt hr, part[P_LR] += cnt lr (want_lr).   bwd 1: part[P_G] += G, part[P_GH] += G hr (want_gh).
__global__ __launch_bounds__(256) void stats_partial_kernel(int bwd, int want2, int batch, int nodes, int cells, int C,
                                                            const float* __restrict__ hr, int ld_hr, const float* __restrict__ lr,
                                                            int ld_lr, const float* __restrict__ g, int ld_g,
                                                            const int* __restrict__ inv_ptr, const int* __restrict__ inv_idx,
                                                            double* __restrict__ part, int n_slabs) {
  __shared__ double red[2][kRowGroups][64];
  const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int ctiles = (C + 63) / 64;
  const int b = blockIdx.y / ctiles;
  const int c = (blockIdx.y - b * ctiles) * 64 + lane;
  const int k0 = blockIdx.x * kSlabRows;
  const int k1 = min(cells, k0 + kSlabRows);
  double a0 = 0.0, a1 = 0.0;
  if (c < C) {
    const int64_t hb = (int64_t)b * cells * ld_hr;
    if (!bwd) {
      const int64_t lb = (int64_t)b * cells * ld_lr;
      for (int k = k0 + rg; k < k1; k += kRowGroups) {
        const int w = inv_ptr[k + 1] - inv_ptr[k];
        if (w == 0) continue;
        a0 += (double)w * (double)hr[hb + (int64_t)k * ld_hr + c];
        if (want2) a1 += (double)w * (double)lr[lb + (int64_t)k * ld_lr + c];
      }
    } else {
      const int64_t gb = (int64_t)b * nodes * ld_g;
      for (int k = k0 + rg; k < k1; k += kRowGroups) {
        if (inv_ptr[k + 1] == inv_ptr[k]) continue;
        const float G = cell_grad(g, gb, ld_g, inv_ptr, inv_idx, k, c);
        a0 += (double)G;
        if (want2) a1 += (double)G * (double)hr[hb + (int64_t)k * ld_hr + c];
      }
    }
  }
  red[0][rg][lane] = a0;
  red[1][rg][lane] = a1;
  __syncthreads();
  if (rg == 0 && c < C) {
    double s0 = 0.0, s1 = 0.0;
    for (int q = 0; q < kRowGroups; ++q) {  // fixed order
      s0 += red[0][q][lane];
      s1 += red[1][q][lane];
    }
    const int q0 = bwd ? P_G : P_HR, q1 = bwd ? P_GH : P_LR;
    const int64_t o = ((int64_t)b * n_slabs + blockIdx.x) * C + c;
    const int64_t plane = (int64_t)batch * n_slabs * C;
    part[q0 * plane + o] = s0;
    if (want2) part[q1 * plane + o] = s1;
  }
}

// one workgroup per (b, c): thread t sums slabs t, t + 256, ... in order, then a fixed-shape tree over the 256 threads
// (no atomics: bitwise reproducible); thread 0 writes the scalars of the type
__global__ __launch_bounds__(256) void stats_final_kernel(int type, int fwd, int bwd, int batch, int nodes, int C, int n_slabs,
                                                          const double* __restrict__ part, float* __restrict__ st) {
  __shared__ double red[kParts][256];
  const int t = blockIdx.x;  // b * C + c
  const int b = t / C, c = t - b * C;
  const int64_t plane = (int64_t)batch * n_slabs * C;
  const double* p = part + (int64_t)b * n_slabs * C + c;
  const int64_t plane_bc = (int64_t)batch * C;
  const bool mult = type == GW_CONSTRAINT_MULTIPLICATIVE;
  double acc[kParts] = {0.0, 0.0, 0.0, 0.0};
  for (int s = threadIdx.x; s < n_slabs; s += 256) {
    if (fwd) {
      acc[P_HR] += p[P_HR * plane + (int64_t)s * C];
      if (mult) acc[P_LR] += p[P_LR * plane + (int64_t)s * C];
    }
    if (bwd) {
      acc[P_G] += p[P_G * plane + (int64_t)s * C];
      if (mult) acc[P_GH] += p[P_GH * plane + (int64_t)s * C];
    }
  }
  for (int q = 0; q < kParts; ++q) red[q][threadIdx.x] = acc[q];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int q = 0; q < kParts; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (fwd) {
    const float mean_hr = (float)(red[P_HR][0] / nodes);
    st[ST_MEAN_HR * plane_bc + t] = mean_hr;
    if (mult) {
      const float mean_lr = (float)(red[P_LR][0] / nodes);
      st[ST_MEAN_LR * plane_bc + t] = mean_lr;
      st[ST_RATIO * plane_bc + t] = mean_lr / (mean_hr + 1e-8f);
    }
  }
  if (bwd) {
    const double s_g = red[P_G][0], s_gh = red[P_GH][0];
    st[ST_MEAN_G * plane_bc + t] = (float)(s_g / nodes);
    if (mult) {
      // ratio = m_lr / (m_hr + 1e-8):  d/dm_hr = -m_lr / den^2,  d/dm_lr = 1 / den;  d m / d row = cnt / N
      const double den = (double)st[ST_MEAN_HR * plane_bc + t] + 1e-8;
      const double m_lr = st[ST_MEAN_LR * plane_bc + t];
      st[ST_Q_HR * plane_bc + t] = (float)(-s_gh * m_lr / (den * den) / nodes);
      st[ST_Q_LR * plane_bc + t] = (float)(s_gh / den / nodes);
    }
  }
}

// softmax f > 1, one thread per (b, low-res cell kl, c): ratio[b, kl, c] = lr * (1 / (avgpool_f(E) * f^2))
__global__ __launch_bounds__(256) void block_ratio_kernel(int total, int C, int cells_lr, int grid_w, int f, float a,
                                                          const float* __restrict__ hr, int ld_hr, const float* __restrict__ lr,
                                                          int ld_lr, float* __restrict__ ratio) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int r = e / C, c = e - r * C;
  const int b = r / cells_lr, kl = r - b * cells_lr;
  const int wl = grid_w / f, bi = kl / wl, bj = kl - bi * wl;
  const int64_t hb = (int64_t)b * cells_lr * f * f * ld_hr;
  float s = 0.f;
  for (int di = 0; di < f; ++di)
    for (int dj = 0; dj < f; ++dj) s += expf(a * hr[hb + ((int64_t)(bi * f + di) * grid_w + bj * f + dj) * ld_hr + c]);
  const float area = (float)(f * f);
  const float S = (s / area) * area;
  ratio[e] = lr[(int64_t)r * ld_lr + c] * (1.0f / S);
}

// one thread per output element (b, n, c)
__global__ __launch_bounds__(256) void apply_kernel(int type, int total, int nodes, int cells, int C, int f, int grid_w, float a,
                                                    const float* __restrict__ hr, int ld_hr, const float* __restrict__ lr,
                                                    int ld_lr, const int* __restrict__ map, const float* __restrict__ st,
                                                    int batch, const float* __restrict__ ratio, float* __restrict__ out,
                                                    int ld_out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int r = e / C, c = e - r * C;
  const int b = r / nodes, n = r - b * nodes;
  const int k = map[n];
  const float h = hr[((int64_t)b * cells + k) * ld_hr + c];
  const int64_t bc = (int64_t)b * C + c, plane = (int64_t)batch * C;
  float y;
  if (type == GW_CONSTRAINT_ADDITIVE) {
    const float l = lr[((int64_t)b * cells + k) * ld_lr + c];
    y = h + (l - st[ST_MEAN_HR * plane + bc]);
  } else if (type == GW_CONSTRAINT_MULTIPLICATIVE) {
    y = h * st[ST_RATIO * plane + bc];
  } else if (f == 1) {
    const float l = lr[((int64_t)b * cells + k) * ld_lr + c];
    const float ex = expf(a * h);
    y = ex * (l * (1.0f / ex));  // the reference's order: overflows to inf / NaN exactly where it does
  } else {
    const int wl = grid_w / f, i = k / grid_w, j = k - i * grid_w;
    const int kl = (i / f) * wl + j / f;
    y = expf(a * h) * ratio[((int64_t)b * (cells / (f * f)) + kl) * C + c];
  }
  out[(int64_t)r * ld_out + c] = y;
}

// softmax f > 1 backward, one thread per (b, kl, c): with G the output gradient per grid cell and E = exp(a hr),
// d ratio = sum_block G E (kron backward), dlr = d ratio / S, d S = -(d ratio lr) / S^2, and the pool's share of dE,
// gpool = (d S * f^2) / f^2, goes to the workspace beside the ratio for backward_kernel
__global__ __launch_bounds__(256) void block_backward_kernel(int total, int nodes, int C, int cells_lr, int grid_w, int f, float a,
                                                             const float* __restrict__ hr, int ld_hr, const float* __restrict__ lr,
                                                             int ld_lr, const float* __restrict__ g, int ld_g,
                                                             const int* __restrict__ inv_ptr, const int* __restrict__ inv_idx,
                                                             float* __restrict__ ratio, float* __restrict__ gpool,
                                                             float* __restrict__ dlr, int ld_dlr) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int r = e / C, c = e - r * C;
  const int b = r / cells_lr, kl = r - b * cells_lr;
  const int wl = grid_w / f, bi = kl / wl, bj = kl - bi * wl;
  const int64_t hb = (int64_t)b * cells_lr * f * f * ld_hr, gb = (int64_t)b * nodes * ld_g;
  float s = 0.f, dr = 0.f;
  for (int di = 0; di < f; ++di)
    for (int dj = 0; dj < f; ++dj) {
      const int k = (bi * f + di) * grid_w + bj * f + dj;
      const float ex = expf(a * hr[hb + (int64_t)k * ld_hr + c]);
      s += ex;
      dr += cell_grad(g, gb, ld_g, inv_ptr, inv_idx, k, c) * ex;
    }
  const float area = (float)(f * f);
  const float S = (s / area) * area;
  const float inv = 1.0f / S;
  const float l = lr[(int64_t)r * ld_lr + c];
  ratio[e] = l * inv;
  if (dlr) dlr[(int64_t)r * ld_dlr + c] = dr * inv;
  const float dS = -(dr * l) * (inv * inv);
  gpool[e] = (dS * area) / area;
}

// one thread per grid row element (b, k, c): dhr (and dlr for f == 1)
__global__ __launch_bounds__(256) void backward_kernel(int type, int total, int nodes, int cells, int C, int f, int grid_w,
                                                       int graph_rows, float a, const float* __restrict__ hr, int ld_hr,
                                                       const float* __restrict__ lr, int ld_lr, const float* __restrict__ g,
                                                       int ld_g, const int* __restrict__ inv_ptr, const int* __restrict__ inv_idx,
                                                       const float* __restrict__ st, int batch, const float* __restrict__ ratio,
                                                       const float* __restrict__ gpool, float* __restrict__ dhr, int ld_dhr,
                                                       float* __restrict__ dlr, int ld_dlr) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int r = e / C, c = e - r * C;
  const int b = r / cells, k = r - b * cells;
  const int cnt = inv_ptr[k + 1] - inv_ptr[k];
  const int64_t row = (int64_t)b * cells + k;
  if (cnt == 0 && (type != GW_CONSTRAINT_SOFTMAX || graph_rows)) {  // a row no node reads: no gradient at all
    if (dhr) dhr[row * ld_dhr + c] = 0.f;
    if (dlr && f == 1) dlr[row * ld_dlr + c] = 0.f;
    return;
  }
  const float G = cnt ? cell_grad(g, (int64_t)b * nodes * ld_g, ld_g, inv_ptr, inv_idx, k, c) : 0.f;
  const int64_t bc = (int64_t)b * C + c, plane = (int64_t)batch * C;
  float dh, dl;
  if (type == GW_CONSTRAINT_ADDITIVE) {
    dh = G - (float)cnt * st[ST_MEAN_G * plane + bc];
    dl = G;
  } else if (type == GW_CONSTRAINT_MULTIPLICATIVE) {
    dh = st[ST_RATIO * plane + bc] * G + (float)cnt * st[ST_Q_HR * plane + bc];
    dl = (float)cnt * st[ST_Q_LR * plane + bc];
  } else if (f == 1) {  // autograd of e * (l * (1 / e)), e = exp(a h)
    const float h = hr[row * ld_hr + c], l = lr[row * ld_lr + c];
    const float ex = expf(a * h), q = 1.0f / ex, p = l * q;
    const float dp = G * ex;
    dl = dp * q;
    const float de = G * p + (-(dp * l) * (q * q));
    dh = (de * ex) * a;
  } else {
    const int wl = grid_w / f, i = k / grid_w, j = k - i * grid_w;
    const int64_t kl = (int64_t)b * (cells / (f * f)) + (i / f) * wl + j / f;
    const float ex = expf(a * hr[row * ld_hr + c]);
    dh = ((G * ratio[kl * C + c] + gpool[kl * C + c]) * ex) * a;
    dl = 0.f;
  }
  if (dhr) dhr[row * ld_dhr + c] = dh;
  if (dlr && f == 1) dlr[row * ld_dlr + c] = dl;
}

struct Layout {
  int n_slabs = 0;
  size_t part_off = 0, st_off = 0, ratio_off = 0, gpool_off = 0, bytes = 0;
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int cells_lr_of(const gw_constraint_args* a) { return a->f > 1 ? a->cells / (a->f * a->f) : a->cells; }

Layout layout_of(const gw_constraint_args* a) {
  Layout l;
  l.n_slabs = (a->cells + kSlabRows - 1) / kSlabRows;
  const size_t C = (size_t)a->channels, B = (size_t)a->batch;
  size_t off = 0;
  if (a->type != GW_CONSTRAINT_SOFTMAX) {
    l.part_off = off;
    off = align256(off + (size_t)kParts * B * l.n_slabs * C * sizeof(double));
    l.st_off = off;
    off = align256(off + (size_t)kSlots * B * C * sizeof(float));
  } else if (a->f > 1) {
    const size_t n = B * (size_t)cells_lr_of(a) * C * sizeof(float);
    l.ratio_off = off;
    off = align256(off + n);
    l.gpool_off = off;
    off = align256(off + n);
  }
  l.bytes = off;
  return l;
}

// argument checks shared by forward and backward; returns GW_OK or the failure code (message set)
int validate(const gw_constraint_args* a, const char* who) {
  static char msg[160];
  if (!a || !a->hr || !a->lr || !a->map || !a->inv_ptr || !a->inv_idx || a->batch <= 0 || a->nodes <= 0 || a->channels <= 0 ||
      a->cells <= 0 || a->ld_hr < a->channels || a->ld_lr < a->channels || a->f < 1 ||
      (a->type != GW_CONSTRAINT_ADDITIVE && a->type != GW_CONSTRAINT_MULTIPLICATIVE && a->type != GW_CONSTRAINT_SOFTMAX)) {
    snprintf(msg, sizeof(msg), "%s: bad arguments", who);
    return failc(GW_E_BADARG, msg);
  }
  if (a->f > 1 && (a->type != GW_CONSTRAINT_SOFTMAX || a->graph_rows || a->grid_h <= 0 || a->grid_w <= 0 ||
                   (int64_t)a->grid_h * a->grid_w != a->cells || a->grid_h % a->f || a->grid_w % a->f)) {
    snprintf(msg, sizeof(msg), "%s: bad arguments (f > 1: softmax on a grid_h x grid_w grid of whole f x f blocks)", who);
    return failc(GW_E_BADARG, msg);
  }
  const int64_t lim = INT32_MAX, B = a->batch;
  if (B * a->nodes * a->channels > lim || B * a->cells * a->ld_hr > lim || B * cells_lr_of(a) * a->ld_lr > lim ||
      B * a->cells * a->channels > lim) {
    snprintf(msg, sizeof(msg), "%s: more than 2^31-1 elements", who);
    return failc(GW_E_UNSUPPORTED, msg);
  }
  return GW_OK;
}

unsigned blocks_of(int64_t total) { return (unsigned)((total + 255) / 256); }

int run_stats(const gw_constraint_args* a, const Layout& l, char* ws, int bwd, int want2, const float* g, int ld_g,
              hipStream_t st) {
  const int ctiles = (a->channels + 63) / 64;
  hipLaunchKernelGGL(stats_partial_kernel, dim3(l.n_slabs, a->batch * ctiles), dim3(256), 0, st, bwd, want2, a->batch, a->nodes,
                     a->cells, a->channels, a->hr, a->ld_hr, a->lr, a->ld_lr, g, ld_g, a->inv_ptr, a->inv_idx,
                     (double*)(ws + l.part_off), l.n_slabs);
  return check_launch("stats_partial_kernel launch");
}

}  // namespace

extern "C" {

size_t gw_constraint_workspace_bytes(const gw_constraint_args* a) {
  if (validate(a, "gw_constraint_workspace_bytes") != GW_OK) return 0;
  return layout_of(a).bytes;
}

int gw_constraint_forward(const gw_constraint_args* a, void* workspace, size_t workspace_bytes, float* out, int32_t ld_out,
                          void* stream) {
  int rc = validate(a, "gw_constraint_forward");
  if (rc != GW_OK) return rc;
  if (!out || ld_out < a->channels) return failc(GW_E_BADARG, "gw_constraint_forward: bad arguments");
  if ((int64_t)a->batch * a->nodes * ld_out > INT32_MAX) return failc(GW_E_UNSUPPORTED, "gw_constraint_forward: more than 2^31-1 elements");
  const Layout l = layout_of(a);
  if (workspace_bytes < l.bytes || (l.bytes && !workspace))
    return failc(GW_E_BADARG, "gw_constraint_forward: workspace smaller than gw_constraint_workspace_bytes");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const int B = a->batch, C = a->channels;
  float* st = ws ? (float*)(ws + l.st_off) : nullptr;
  float* ratio = ws ? (float*)(ws + l.ratio_off) : nullptr;
  if (a->type != GW_CONSTRAINT_SOFTMAX) {
    if ((rc = run_stats(a, l, ws, 0, a->type == GW_CONSTRAINT_MULTIPLICATIVE, nullptr, 0, s)) != GW_OK) return rc;
    hipLaunchKernelGGL(stats_final_kernel, dim3(B * C), dim3(256), 0, s, a->type, 1, 0, B, a->nodes, C, l.n_slabs,
                       (const double*)(ws + l.part_off), st);
    if ((rc = check_launch("stats_final_kernel launch")) != GW_OK) return rc;
  } else if (a->f > 1) {
    const int total = B * cells_lr_of(a) * C;
    hipLaunchKernelGGL(block_ratio_kernel, dim3(blocks_of(total)), dim3(256), 0, s, total, C, cells_lr_of(a), a->grid_w, a->f,
                       a->exp_factor, a->hr, a->ld_hr, a->lr, a->ld_lr, ratio);
    if ((rc = check_launch("block_ratio_kernel launch")) != GW_OK) return rc;
  }
  const int total = B * a->nodes * C;
  hipLaunchKernelGGL(apply_kernel, dim3(blocks_of(total)), dim3(256), 0, s, a->type, total, a->nodes, a->cells, C, a->f, a->grid_w,
                     a->exp_factor, a->hr, a->ld_hr, a->lr, a->ld_lr, a->map, st, B, ratio, out, ld_out);
  return check_launch("apply_kernel launch");
}

int gw_constraint_backward(const gw_constraint_args* a, const float* dout, int32_t ld_dout, void* workspace, size_t workspace_bytes,
                           float* dhr, int32_t ld_dhr, float* dlr, int32_t ld_dlr, void* stream) {
  int rc = validate(a, "gw_constraint_backward");
  if (rc != GW_OK) return rc;
  const int B = a->batch, C = a->channels;
  if (!dout || ld_dout < C || (dhr && ld_dhr < C) || (dlr && ld_dlr < C))
    return failc(GW_E_BADARG, "gw_constraint_backward: bad arguments");
  if ((int64_t)B * a->nodes * ld_dout > INT32_MAX || (dhr && (int64_t)B * a->cells * ld_dhr > INT32_MAX) ||
      (dlr && (int64_t)B * cells_lr_of(a) * ld_dlr > INT32_MAX))
    return failc(GW_E_UNSUPPORTED, "gw_constraint_backward: more than 2^31-1 elements");
  const Layout l = layout_of(a);
  if (workspace_bytes < l.bytes || (l.bytes && !workspace))
    return failc(GW_E_BADARG, "gw_constraint_backward: workspace smaller than gw_constraint_workspace_bytes");
  if (!dhr && !dlr) return GW_OK;
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  float* st = ws ? (float*)(ws + l.st_off) : nullptr;
  float* ratio = ws ? (float*)(ws + l.ratio_off) : nullptr;
  float* gpool = ws ? (float*)(ws + l.gpool_off) : nullptr;
  const bool mult = a->type == GW_CONSTRAINT_MULTIPLICATIVE;
  if (a->type != GW_CONSTRAINT_SOFTMAX) {
    if (mult && (rc = run_stats(a, l, ws, 0, 1, nullptr, 0, s)) != GW_OK) return rc;
    if ((rc = run_stats(a, l, ws, 1, mult, dout, ld_dout, s)) != GW_OK) return rc;
    hipLaunchKernelGGL(stats_final_kernel, dim3(B * C), dim3(256), 0, s, a->type, mult ? 1 : 0, 1, B, a->nodes, C,
                       l.n_slabs, (const double*)(ws + l.part_off), st);
    if ((rc = check_launch("stats_final_kernel launch")) != GW_OK) return rc;
  } else if (a->f > 1) {
    const int total = B * cells_lr_of(a) * C;
    hipLaunchKernelGGL(block_backward_kernel, dim3(blocks_of(total)), dim3(256), 0, s, total, a->nodes, C, cells_lr_of(a), a->grid_w,
                       a->f, a->exp_factor, a->hr, a->ld_hr, a->lr, a->ld_lr, dout, ld_dout, a->inv_ptr, a->inv_idx, ratio, gpool,
                       dlr, ld_dlr);
    if ((rc = check_launch("block_backward_kernel launch")) != GW_OK) return rc;
  }
  if (!dhr && a->f > 1) return GW_OK;
  const int total = B * a->cells * C;
  hipLaunchKernelGGL(backward_kernel, dim3(blocks_of(total)), dim3(256), 0, s, a->type, total, a->nodes, a->cells, C, a->f, a->grid_w,
                     a->graph_rows, a->exp_factor, a->hr, a->ld_hr, a->lr, a->ld_lr, dout, ld_dout, a->inv_ptr, a->inv_idx, st, B,
                     ratio, gpool, dhr, ld_dhr, dlr, ld_dlr);
  return check_launch("backward_kernel launch");
}

}  // extern "C"
