// npfn_kmeans.hip -- K13: seeded k-means (k-means++ seeding + Lloyd) and nearest-centre
// assignment for TabPFN_Based_Uncond_Estimator (reference npe_pfn.py:793-794, 855: sklearn's
// KMeans.fit / KMeans.predict on the host).  Every distance and sum is fp64 on the fp32
// points; every reduction runs in a fixed order (no floating-point atomics), so the same
// inputs and seed give the same bits on every run.
//
//   k_km_colvar   population variance per column            -> tol_abs = tol * mean_j var_j
//   k_km_seed     k-means++ (one workgroup, k - 1 passes over the rows)
//   k_km_assign   nearest centre per row; per-wave partial sums / counts per cluster
//   k_km_update   partials added in wave order -> new centres, shift, done flag
//   k_km_store    centres rounded to fp32; the final labels / counts are one more
//                 k_km_assign against those stored centres
#include <hip/hip_runtime.h>

#include <string>

#include "npfn.h"
#include "npfn_common.h"
#include "npfn_kernels.h"

namespace {

constexpr int KM_MAX_CD = 4096;          // k * dim: the centres as fp64 in LDS, 32 KB
constexpr int KM_CHECK_EVERY = 8;        // Lloyd iterations between two looks at the done flag
constexpr int64_t KM_PART_CAP = 1 << 21; // doubles of per-wave partials (16 MB)

// column j: population variance in fp64 (two passes: mean, then squared deviations)
__global__ __launch_bounds__(256) void k_km_colvar(const float* __restrict__ x, int64_t n, int dim,
                                                   double* __restrict__ var) {
  __shared__ double red[4];
  const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double s = 0.0;
  for (int64_t i = tid; i < n; i += 256) s += (double)x[i * dim + j];
  s = wave_sum_d(s);
  if (lane == 0) red[w] = s;
  __syncthreads();
  const double mean = (red[0] + red[1] + red[2] + red[3]) / (double)n;
  __syncthreads();
  double q = 0.0;
  for (int64_t i = tid; i < n; i += 256) {
    const double dv = (double)x[i * dim + j] - mean;
    q += dv * dv;
  }
  q = wave_sum_d(q);
  if (lane == 0) red[w] = q;
  __syncthreads();
  if (tid == 0) var[j] = (red[0] + red[1] + red[2] + red[3]) / (double)n;
}

// k-means++ with one candidate per centre, u_c = philox_uniform(seed, 0, c).  One workgroup of
// 1024: per centre one pass that folds the newest centre into d2 (squared distance to the
// nearest chosen centre) and totals it, and one ordered prefix scan that stops at the first
// row whose inclusive sum exceeds u_c * total.  Thread t always owns rows t, t + 1024, ...,
// so d2 needs no fence between the passes.
__global__ __launch_bounds__(1024) void k_km_seed(const float* __restrict__ x, int64_t n, int dim, int k,
                                                  uint64_t seed, float tol, const double* __restrict__ var,
                                                  double* __restrict__ cen, double* __restrict__ d2,
                                                  double* __restrict__ tol_abs) {
  __shared__ double s_c[KM_MAX_CD];  // the newest centre (dim <= KM_MAX_CD)
  __shared__ double wred[16];
  __shared__ long long s_pick, s_last;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) {
    double s = 0.0;
    for (int j = 0; j < dim; ++j) s += var[j];
    *tol_abs = (double)tol * (s / (double)dim);
  }
  int64_t row = (int64_t)floor((double)philox_uniform(seed, 0, 0) * (double)n);
  if (row > n - 1) row = n - 1;
  for (int c = 0;; ++c) {
    __syncthreads();  // the previous round's readers of s_c are done
    for (int j = tid; j < dim; j += 1024) {
      const double v = (double)x[row * dim + j];
      s_c[j] = v;
      cen[(int64_t)c * dim + j] = v;
    }
    if (tid == 0) {
      s_pick = n;
      s_last = 0;
    }
    __syncthreads();
    if (c == k - 1) break;
    // pass A: d2_i = min(d2_i, |x_i - newest centre|^2), total in a fixed order
    double part = 0.0;
    for (int64_t i = tid; i < n; i += 1024) {
      double acc = 0.0;
      for (int j = 0; j < dim; ++j) {
        const double df = (double)x[i * dim + j] - s_c[j];
        acc += df * df;
      }
      if (c > 0) acc = fmin(acc, d2[i]);
      d2[i] = acc;
      part += acc;
    }
    part = wave_sum_d(part);
    if (lane == 0) wred[w] = part;
    __syncthreads();
    double tot = 0.0;
    for (int q = 0; q < 16; ++q) tot += wred[q];
    __syncthreads();
    const double u = (double)philox_uniform(seed, 0, (uint64_t)(c + 1));
    if (tot == 0.0) {  // every row sits on a chosen centre
      row = (int64_t)floor(u * (double)n);
      if (row > n - 1) row = n - 1;
      continue;
    }
    // pass B: first i whose inclusive prefix sum exceeds the target
    const double target = u * tot;
    double base = 0.0;
    for (int64_t c0 = 0; c0 < n; c0 += 1024) {
      const int64_t i = c0 + tid;
      const double e = i < n ? d2[i] : 0.0;
      double incl = e;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const double t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
      }
      if (lane == 63) wred[w] = incl;
      __syncthreads();
      double pre = 0.0, ctot = 0.0;
      for (int q = 0; q < 16; ++q) {
        if (q < w) pre += wred[q];
        ctot += wred[q];
      }
      if (i < n && base + pre + incl > target) atomicMin((unsigned long long*)&s_pick, (unsigned long long)i);
      if (e > 0.0) atomicMax((unsigned long long*)&s_last, (unsigned long long)i);
      __syncthreads();
      if (s_pick < n) break;  // block-uniform
      base += ctot;
    }
    // u * total rounded past the total: the last row with mass
    row = s_pick < n ? s_pick : s_last;
  }
}

// Nearest centre per row, ties to the lower index.  Lane l of a wave takes row c0 + l: a wave
// reads one contiguous 64 * dim * 4-byte span per chunk, each point once; the centres are staged
// in LDS as fp64 once per block (from the fp64 workspace during Lloyd, from the stored fp32
// centres for the final labels and for npfn_kmeans_assign).  With `part`, wave g adds its
// members' coordinates and counts per cluster, chunk after chunk, into its own column
// part[e * W + g] (e < k * dim: sum of coordinate e % dim of cluster e / dim; e >= k * dim:
// member count); element e is always touched by the same lane e % 64.  D > 0: the row is kept
// in registers; D == 0: any dim, the row is re-read through the cache.
template <int D>
__global__ __launch_bounds__(256) void k_km_assign(const float* __restrict__ x, int64_t n, int dim, int k,
                                                   const double* __restrict__ cen_d,
                                                   const float* __restrict__ cen_f, const int* __restrict__ done,
                                                   int64_t* __restrict__ labels,
                                                   unsigned long long* __restrict__ counts,
                                                   double* __restrict__ part) {
  extern __shared__ double s_cen[];
  if (done && *done) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int cd = k * dim;
  for (int e = tid; e < cd; e += 256) s_cen[e] = cen_d ? cen_d[e] : (double)cen_f[e];
  __syncthreads();
  const int64_t W = (int64_t)gridDim.x * 4;
  const int64_t g = (int64_t)blockIdx.x * 4 + (tid >> 6);
  if (part)
    for (int e = lane; e < cd + k; e += 64) part[(int64_t)e * W + g] = 0.0;
  for (int64_t c0 = g * 64; c0 < n; c0 += W * 64) {
    const int64_t i = c0 + lane;
    const bool valid = i < n;
    const float* xr = x + (valid ? i : c0) * dim;
    double xv[D > 0 ? D : 1];
    if (D > 0) {
#pragma unroll
      for (int j = 0; j < D; ++j) xv[j] = (double)xr[j];
    }
    double best = 0.0;
    int bl = 0;
    for (int c = 0; c < k; ++c) {
      const double* cc = s_cen + c * dim;
      double acc = 0.0;
      if (D > 0) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
          const double df = xv[j] - cc[j];
          acc += df * df;
        }
      } else {
        for (int j = 0; j < dim; ++j) {
          const double df = (double)xr[j] - cc[j];
          acc += df * df;
        }
      }
      if (c == 0 || acc < best) {
        best = acc;
        bl = c;
      }
    }
    if (labels && valid) labels[i] = bl;
    if (!part && !counts) continue;
    for (int c = 0; c < k; ++c) {
      const bool mine = valid && bl == c;
      const unsigned long long bal = __ballot(mine);
      if (!bal) continue;  // wave-uniform
      const int cnt = __popcll(bal);
      if (counts && lane == 0) atomicAdd(counts + c, (unsigned long long)cnt);
      if (!part) continue;
      if (D > 0) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
          const double v = wave_sum_d(mine ? xv[j] : 0.0);
          const int e = c * D + j;
          if (lane == (e & 63)) part[(int64_t)e * W + g] += v;
        }
      } else {
        for (int j = 0; j < dim; ++j) {
          const double v = wave_sum_d(mine ? (double)xr[j] : 0.0);
          const int e = c * dim + j;
          if (lane == (e & 63)) part[(int64_t)e * W + g] += v;
        }
      }
      const int e = cd + c;
      if (lane == (e & 63)) part[(int64_t)e * W + g] += (double)cnt;
    }
  }
}

// One workgroup: wave q takes elements e = q, q + 16, ... of the k * dim centre coordinates.
// Lane l adds the partials of waves l, l + 64, ... in that order, the 64 lane sums meet in
// wave_sum_d's butterfly: a fixed order.  new centre = sum / count (an empty cluster keeps its
// centre); shift = sum_e (new - old)^2, per wave in element order, then over the 16 waves in
// order.  Sets *done when shift <= tol_abs; a launch after that returns at once.
__global__ __launch_bounds__(1024) void k_km_update(const double* __restrict__ part, int64_t W, int k, int dim,
                                                    double* __restrict__ cen, const double* __restrict__ tol_abs,
                                                    int* __restrict__ done, int64_t* __restrict__ n_iter) {
  __shared__ double wred[16];
  if (*done) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int cd = k * dim;
  double shift = 0.0;
  for (int e = w; e < cd; e += 16) {
    const double* ps = part + (int64_t)e * W;
    const double* pc = part + (int64_t)(cd + e / dim) * W;
    double s = 0.0, cnt = 0.0;
    for (int64_t g = lane; g < W; g += 64) {
      s += ps[g];
      cnt += pc[g];
    }
    s = wave_sum_d(s);
    cnt = wave_sum_d(cnt);
    const double old = cen[e];
    const double nw = cnt > 0.0 ? s / cnt : old;
    const double df = nw - old;
    shift += df * df;
    if (lane == 0) cen[e] = nw;
  }
  if (lane == 0) wred[w] = shift;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int q = 0; q < 16; ++q) tot += wred[q];
    *n_iter += 1;
    if (tot <= *tol_abs) *done = 1;
  }
}

__global__ void k_km_store(const double* __restrict__ cen, int cd, float* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < cd) out[e] = (float)cen[e];
}

int fail(int code, const std::string& msg) { return npfn::set_error(code, msg.c_str()); }

int launch_status(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return NPFN_OK;
  return fail(NPFN_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// waves of the assignment grid: one per 64 rows up to 2048, fewer when their partials
// ((k * dim + k) doubles each) would pass KM_PART_CAP
unsigned assign_blocks(int64_t n, int k, int dim) {
  int64_t blocks = (n + 255) / 256;
  int64_t cap = KM_PART_CAP / ((int64_t)k * dim + k) / 4;
  if (cap > 512) cap = 512;
  if (cap < 16) cap = 16;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

void launch_assign(hipStream_t s, unsigned blocks, const float* x, int64_t n, int dim, int k, const double* cen_d,
                   const float* cen_f, const int* done, int64_t* labels, unsigned long long* counts,
                   double* part) {
  const size_t lds = sizeof(double) * (size_t)k * dim;
#define NPFN_KM_CASE(DD)                                                                                       \
  case DD:                                                                                                     \
    hipLaunchKernelGGL(k_km_assign<DD>, dim3(blocks), dim3(256), lds, s, x, n, dim, k, cen_d, cen_f, done,    \
                       labels, counts, part);                                                                  \
    break;
  switch (dim) {
    NPFN_KM_CASE(1)
    NPFN_KM_CASE(2)
    NPFN_KM_CASE(3)
    NPFN_KM_CASE(4)
    NPFN_KM_CASE(5)
    NPFN_KM_CASE(6)
    NPFN_KM_CASE(7)
    NPFN_KM_CASE(8)
    default:
      hipLaunchKernelGGL(k_km_assign<0>, dim3(blocks), dim3(256), lds, s, x, n, dim, k, cen_d, cen_f, done,
                         labels, counts, part);
  }
#undef NPFN_KM_CASE
}

int check_shape(const char* fn, int64_t n_rows, int32_t dim, int32_t k) {
  const std::string f(fn);
  if (k < 1 || dim < 1) return fail(NPFN_EINVAL, f + ": need k >= 1 and dim >= 1");
  if ((int64_t)k * dim > KM_MAX_CD)
    return fail(NPFN_EINVAL, f + ": k * dim = " + std::to_string((int64_t)k * dim) + " exceeds the cap of " +
                                 std::to_string(KM_MAX_CD) + " (the centres are held in LDS as fp64)");
  if (n_rows >= (1ll << 31))
    return fail(NPFN_EINVAL, f + ": n_rows = " + std::to_string(n_rows) + " is not below the cap of 2^31 rows");
  return NPFN_OK;
}

}  // namespace

extern "C" {

int npfn_kmeans_fit(const float* pts, int64_t n_rows, int32_t dim, int32_t k, uint64_t seed, int32_t max_iter,
                    float tol, float* centers, int64_t* labels, int64_t* counts, int64_t* n_iter, void* stream) {
  if (const int rc = check_shape("kmeans_fit", n_rows, dim, k)) return rc;
  if (k > n_rows)
    return fail(NPFN_EINVAL, "kmeans_fit: k = " + std::to_string(k) + " exceeds n_rows = " + std::to_string(n_rows) +
                                 " (at most one cluster per row)");
  if (!pts || !centers || !labels || !counts || !n_iter) return fail(NPFN_EINVAL, "kmeans_fit: null pointer");
  if (max_iter < 0 || !(tol >= 0.f)) return fail(NPFN_EINVAL, "kmeans_fit: need max_iter >= 0 and tol >= 0");
  hipStream_t s = (hipStream_t)stream;
  const int cd = k * dim;
  const unsigned blocks = assign_blocks(n_rows, k, dim);
  const int64_t W = (int64_t)blocks * 4;
  // workspace (doubles): centres | column variances | tol_abs | d2 | partials ; then the done flag
  const int64_t o_var = cd, o_tol = o_var + dim, o_d2 = o_tol + 1, o_part = o_d2 + n_rows;
  const int64_t n_dbl = o_part + (int64_t)(cd + k) * W;
  double* ws = nullptr;
  if (hipMallocAsync((void**)&ws, sizeof(double) * (n_dbl + 1), s) != hipSuccess) {
    (void)hipGetLastError();
    return fail(NPFN_ENOMEM, "kmeans_fit: hipMallocAsync of the " + std::to_string(sizeof(double) * (n_dbl + 1)) +
                                 "-byte workspace failed");
  }
  double *cen = ws, *var = ws + o_var, *tol_abs = ws + o_tol, *d2 = ws + o_d2, *part = ws + o_part;
  int* done = (int*)(ws + n_dbl);
  (void)hipMemsetAsync(done, 0, sizeof(double), s);
  (void)hipMemsetAsync(n_iter, 0, sizeof(int64_t), s);
  (void)hipMemsetAsync(counts, 0, sizeof(int64_t) * k, s);
  hipLaunchKernelGGL(k_km_colvar, dim3(dim), dim3(256), 0, s, pts, n_rows, (int)dim, var);
  hipLaunchKernelGGL(k_km_seed, dim3(1), dim3(1024), 0, s, pts, n_rows, (int)dim, (int)k, seed, tol, var, cen, d2,
                     tol_abs);
  int rc = launch_status("kmeans_fit: seeding launch");
  for (int it = 0; rc == NPFN_OK && it < max_iter; ++it) {
    launch_assign(s, blocks, pts, n_rows, dim, k, cen, nullptr, done, nullptr, nullptr, part);
    hipLaunchKernelGGL(k_km_update, dim3(1), dim3(1024), 0, s, part, W, (int)k, (int)dim, cen, tol_abs, done, n_iter);
    rc = launch_status("kmeans_fit: Lloyd iteration launch");
    if (rc != NPFN_OK || (it + 1) % KM_CHECK_EVERY != 0 || it + 1 >= max_iter) continue;
    int h_done = 0;
    if (hipMemcpyAsync(&h_done, done, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      rc = launch_status("kmeans_fit: reading the convergence flag");
      if (rc == NPFN_OK) rc = fail(NPFN_EHIP, "kmeans_fit: reading the convergence flag failed");
      break;
    }
    if (h_done) break;
  }
  if (rc == NPFN_OK) {
    hipLaunchKernelGGL(k_km_store, dim3((unsigned)((cd + 255) / 256)), dim3(256), 0, s, cen, cd, centers);
    launch_assign(s, blocks, pts, n_rows, dim, k, nullptr, centers, nullptr, labels, (unsigned long long*)counts,
                  nullptr);
    rc = launch_status("kmeans_fit: final assignment launch");
  }
  (void)hipFreeAsync(ws, s);
  return rc;
}

int npfn_kmeans_assign(const float* pts, int64_t n_rows, int32_t dim, const float* centers, int32_t k,
                       int64_t* labels, void* stream) {
  if (const int rc = check_shape("kmeans_assign", n_rows, dim, k)) return rc;
  if (n_rows < 0) return fail(NPFN_EINVAL, "kmeans_assign: need n_rows >= 0");
  if (!centers) return fail(NPFN_EINVAL, "kmeans_assign: null pointer");
  if (n_rows == 0) return NPFN_OK;  // empty pts / labels may come as null pointers: no launch
  if (!pts || !labels) return fail(NPFN_EINVAL, "kmeans_assign: null pointer");
  launch_assign((hipStream_t)stream, assign_blocks(n_rows, k, dim), pts, n_rows, dim, k, nullptr, centers, nullptr,
                labels, nullptr, nullptr);
  return launch_status("kmeans_assign: k_km_assign launch");
}

}  // extern "C"
