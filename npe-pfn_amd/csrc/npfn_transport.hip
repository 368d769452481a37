// npfn_transport.hip -- exact 2-Wasserstein distance between two equally sized, uniformly weighted
// sets of draws (npe_pfn.diagnostics.wasserstein_batched): the linear assignment problem on
// integer costs, solved by the shortest-augmenting-path Hungarian method from zero duals, one
// workgroup per observation.  The statement of every number is in include/npfn.h (npfn_w2_assign);
// npe_pfn.diagnostics.transport_costs_host / assignment_solve_host restate it on the host.
//
// Block size: the smallest power of two in 64..1024 that is >= ceil(n / 2), so a thread owns at
// most kCols = 2 columns (j = tid and tid + blockDim): 64 threads up to n = 128, 128 up to 256,
// 256 up to 512, 512 up to 1024, 1024 up to the cap of 2048.  Every wave pays a step's fixed part
// (the wave reduction, the fold of the waves' slots, the barrier) whatever its share of the
// columns, so a small n runs on few waves.
#include <hip/hip_runtime.h>

#include <string>

#include "npfn.h"
#include "npfn_common.h"
#include "npfn_kernels.h"

namespace {

constexpr int kCols = 2;              // columns per thread
constexpr int kMaxThreads = 1024;
constexpr int kMaxN = kCols * kMaxThreads;
constexpr int kMaxDim = 64;
constexpr int kMaxImage = 32768;      // n * dim floats of b's LDS image (128 KiB)
constexpr size_t kLdsBudget = 160 * 1024 - 1024;   // the CU's LDS less the static arrays' share
constexpr int kVirt = -1;             // the virtual column that holds the row being inserted
constexpr long long kInf = 0x7fffffffffffffffLL;
constexpr int kNone = 0x7fffffff;
constexpr double kMaxCost = 0x1p41;

__device__ __forceinline__ bool not_finite(float v) { return !(fabsf(v) <= 3.4028234663852886e38f); }

// dynamic LDS, in this order: u [n] int64, bT [dim][n] fp32, (A_LDS: aS [n][dim] fp32,) rowOf [n]
// int16, wayS [n] int16
size_t lds_bytes(int n, int dim, bool a_lds) {
  return (size_t)n * 8 + (size_t)n * dim * 4 * (a_lds ? 2 : 1) + (size_t)n * 2 * 2;
}

// One workgroup solves observation obs0 + blockIdx.x.  Thread tid owns columns tid and tid +
// blockDim and keeps their v, minv, way, used flag and (once used) row in registers; u, the
// column -> row map and, for the path flip, way are in LDS.  Each step recomputes the cost row of
// i0 from b's transposed LDS image (lane j reads word k * n + j: conflict-free) and a's row i0 (an
// LDS broadcast when a fits beside b, a scalar load from global memory otherwise), k ascending,
// every operation rounded on its own (plain operators with the contraction into FMAs switched
// off, as in k_mmd_sums).  The step's (minimum, lowest column) goes through wave_argmin_i64, one
// LDS slot per wave and one barrier; every thread then folds the slots itself.  One barrier per
// step is enough: the slots alternate between two sets by the step's parity; u[i0] is read
// before the barrier and the only thread that writes it (the owner of column j0, after the
// barrier) waits there for every reader; the rows written after a step's barrier belong to used
// columns, the row read before the next one to a column that was not used yet.  u of the row
// being inserted is read in its first step only, so its deltas are summed in a register and added
// once.  A cost above 2^41 (or not a number: a d2 that overflowed) enters the reduction as -1,
// below every true value (the reduced costs are >= 0), so the whole workgroup sees it in the same
// step and leaves.  Every loop is bounded before it starts: n insertions, at most i + 1 steps in
// insertion i, at most n + 1 hops in the flip.
template <bool A_LDS>
__global__ __launch_bounds__(kMaxThreads) void k_w2_assign(const float* __restrict__ a, const float* __restrict__ b,
                                                            int n, int dim, int64_t obs0,
                                                            const double* __restrict__ scale, int* __restrict__ assign,
                                                            long long* __restrict__ duals,
                                                            unsigned long long* __restrict__ cost_sum,
                                                            long long* __restrict__ steps, int* __restrict__ bad) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ long long red_v[2][kMaxThreads / 64];
  __shared__ int red_j[2][kMaxThreads / 64];
  const int tid = threadIdx.x, B = blockDim.x, lane = tid & 63, w = tid >> 6, nW = B >> 6;
  const int64_t ob = obs0 + blockIdx.x;
  long long* uS = reinterpret_cast<long long*>(smem);
  float* bT = reinterpret_cast<float*>(uS + n);
  float* aS = bT + (size_t)n * dim;
  short* rowOf = reinterpret_cast<short*>(aS + (A_LDS ? (size_t)n * dim : 0));
  short* wayS = rowOf + n;
  const float* __restrict__ ag = a + ob * n * dim;
  const float* __restrict__ bg = b + ob * n * dim;

  bool nonfinite = false;
  for (int idx = tid; idx < n * dim; idx += B) {
    const int r = idx / dim, k = idx - r * dim;
    const float vb = bg[idx], va = ag[idx];
    nonfinite |= not_finite(vb) || not_finite(va);
    bT[k * n + r] = vb;
    if (A_LDS) aS[idx] = va;
  }
  for (int j = tid; j < n; j += B) {
    uS[j] = 0;
    rowOf[j] = -1;
  }
  if (__syncthreads_or(nonfinite)) {   // uniform; also the barrier behind the staging
    if (tid == 0) bad[ob] = 1;
    return;
  }

  const double sc = scale[ob];
  int col[kCols], colc[kCols];   // the owned columns; clamped into the image for the reads
  long long v[kCols], minv[kCols];
  int way[kCols], myrow[kCols];
  bool used[kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c) {
    col[c] = tid + c * B;
    colc[c] = min(col[c], n - 1);
    v[c] = 0;
    myrow[c] = 0;
  }

  // d2 of (row r, owned column c) as the definition has it, then q = llrint(d2 * scale); over is
  // raised for a product above 2^41 or not a number
  auto cost = [&](int r, int c, bool& over) -> long long {
    float acc = 0.f;
    for (int k = 0; k < dim; ++k) {
      const float ak = A_LDS ? aS[r * dim + k] : ag[(size_t)r * dim + k];
      const float t = ak - bT[k * n + colc[c]];
      const float tt = t * t;
      acc = acc + tt;
    }
    const double p = (double)acc * sc;
    const bool o = !(p <= kMaxCost);
    over |= o;
    return o ? 0 : llrint(p);
  };

  const long long cap = (long long)n * (n + 1) / 2;
  long long nsteps = 0;
  int err = 0;
  for (int i = 0; i < n; ++i) {
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
      minv[c] = kInf;
      way[c] = kVirt;
      used[c] = false;
    }
    int j0 = kVirt, i0 = i;
    long long dsum = 0;
    for (int s = 0; s <= i; ++s) {
      if (++nsteps > cap) {
        err = 3;
        break;
      }
      const int r0 = __builtin_amdgcn_readfirstlane(i0);
      const long long ui = uS[r0];
      bool over = false;
      long long bv = kInf;
      int bj = kNone;
#pragma unroll
      for (int c = 0; c < kCols; ++c) {
        if (col[c] < n && !used[c]) {
          const long long cur = cost(r0, c, over) - ui - v[c];
          if (cur < minv[c]) {
            minv[c] = cur;
            way[c] = j0;
          }
          if (minv[c] < bv) {   // c ascending is column ascending: the lowest column of a tie stays
            bv = minv[c];
            bj = col[c];
          }
        }
      }
      if (over) {
        bv = -1;
        bj = 0;
      }
      wave_argmin_i64(bv, bj);
      const int par = s & 1;
      if (lane == 0) {
        red_v[par][w] = bv;
        red_j[par][w] = bj;
      }
      __syncthreads();
      long long delta = red_v[par][0];
      int j1 = red_j[par][0];
      for (int x = 1; x < nW; ++x) argmin_take(delta, j1, red_v[par][x], red_j[par][x]);
      if (delta < 0) {
        err = 2;
        break;
      }
      if (j1 >= n) {   // no unused column left: cannot happen inside the step bound
        err = 3;
        break;
      }
#pragma unroll
      for (int c = 0; c < kCols; ++c) {
        if (col[c] < n) {
          if (used[c]) {
            uS[myrow[c]] += delta;
            v[c] -= delta;
          } else {
            minv[c] -= delta;
          }
        }
      }
      dsum += delta;
      i0 = rowOf[j1];
#pragma unroll
      for (int c = 0; c < kCols; ++c) {
        if (col[c] == j1) {
          used[c] = true;
          myrow[c] = i0;
        }
      }
      j0 = j1;
      if (i0 < 0) break;
    }
    if (err) break;
    if (i0 >= 0) {   // the step bound of this insertion ran out before a free column
      err = 3;
      break;
    }
#pragma unroll
    for (int c = 0; c < kCols; ++c)
      if (col[c] < n) wayS[col[c]] = (short)way[c];
    __syncthreads();
    if (tid == 0) {
      uS[i] += dsum;
      int jj = j0;
      for (int t = 0; t <= n && jj != kVirt; ++t) {
        const int jp = wayS[jj];
        rowOf[jj] = jp == kVirt ? (short)i : rowOf[jp];
        jj = jp;
      }
    }
    __syncthreads();
  }
  if (err) {   // uniform over the workgroup
    if (tid == 0) bad[ob] = err;
    return;
  }

  long long mine = 0;
#pragma unroll
  for (int c = 0; c < kCols; ++c) {
    if (col[c] < n) {
      const int r = rowOf[col[c]];   // >= 0: n insertions matched every column
      bool over = false;
      if (r >= 0) {
        mine += cost(r, c, over);
        assign[ob * n + r] = col[c];
      }
      if (duals) duals[(ob * 2 + 1) * n + col[c]] = v[c];
    }
  }
  if (duals)
    for (int j = tid; j < n; j += B) duals[ob * 2 * n + j] = uS[j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if (lane == 0 && mine) atomicAdd(cost_sum + ob, (unsigned long long)mine);
  if (tid == 0 && steps) steps[ob] = nsteps;
}

int fail(int code, const std::string& msg) { return npfn::set_error(code, msg.c_str()); }

}  // namespace

extern "C" {

int npfn_w2_assign(const float* a, const float* b, int64_t n_obs, int32_t n, int32_t dim, const double* scale,
                   int32_t* assign, int64_t* duals, int64_t* cost_sum, int64_t* steps, int32_t* bad, void* stream) {
  if (n_obs < 0) return fail(NPFN_EINVAL, "w2_assign: need n_obs >= 0");
  if (n < 1 || n > kMaxN)
    return fail(NPFN_EINVAL, "w2_assign: n must lie in 1.." + std::to_string(kMaxN) +
                                 " (two columns per thread of a 1024-thread workgroup)");
  if (dim < 1 || dim > kMaxDim) return fail(NPFN_EINVAL, "w2_assign: dim must lie in 1.." + std::to_string(kMaxDim));
  if ((int64_t)n * dim > kMaxImage)
    return fail(NPFN_EINVAL, "w2_assign: n * dim must not exceed " + std::to_string(kMaxImage) +
                                 " (b's coordinates stay in LDS)");
  if (!a || !b || !scale || !assign || !cost_sum || !bad)
    return fail(NPFN_EINVAL, "w2_assign: null a, b, scale, assign, cost_sum or bad");
  if (n_obs == 0) return NPFN_OK;

  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(assign, 0, (size_t)n_obs * n * sizeof(int32_t), s);
  if (e == hipSuccess && duals) e = hipMemsetAsync(duals, 0, (size_t)n_obs * 2 * n * sizeof(int64_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(cost_sum, 0, (size_t)n_obs * sizeof(int64_t), s);
  if (e == hipSuccess && steps) e = hipMemsetAsync(steps, 0, (size_t)n_obs * sizeof(int64_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(bad, 0, (size_t)n_obs * sizeof(int32_t), s);
  if (e != hipSuccess) return fail(NPFN_EHIP, std::string("w2_assign: hipMemsetAsync: ") + hipGetErrorString(e));

  int threads = 64;
  while (threads * kCols < n) threads *= 2;   // <= 1024: n <= kMaxN
  const bool a_lds = lds_bytes(n, dim, true) <= kLdsBudget;
  const size_t lds = lds_bytes(n, dim, a_lds);   // <= 152 KiB at the caps
  auto kern = a_lds ? k_w2_assign<true> : k_w2_assign<false>;
  e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget);
  if (e != hipSuccess) return fail(NPFN_EHIP, std::string("w2_assign: hipFuncSetAttribute: ") + hipGetErrorString(e));
  const int64_t per_launch = 1 << 30;
  for (int64_t m0 = 0; m0 < n_obs; m0 += per_launch) {
    const int64_t nb = n_obs - m0 < per_launch ? n_obs - m0 : per_launch;
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(threads), lds, s, a, b, (int)n, (int)dim, m0, scale, (int*)assign,
                       (long long*)duals, (unsigned long long*)cost_sum, (long long*)steps, (int*)bad);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(NPFN_EHIP, std::string("w2_assign: k_w2_assign launch: ") + hipGetErrorString(e));
  }
  return NPFN_OK;
}

}  // extern "C"
