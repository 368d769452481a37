// npfn_ranks.hip -- coverage ranks (NPE_PFN_Core.coverage_batched): one sampler round folded into
// per-observation integer counts of "draw < truth" / "draw == truth" per parameter
// (simulation-based calibration), of "draw denser than the truth" (HPD) and of "draw closer to
// the reference point than the truth" (TARP).  The statement of every count is in include/npfn.h
// (npfn_rank_accumulate); npe_pfn.diagnostics.rank_accumulate_host restates it in torch.
#include <hip/hip_runtime.h>

#include <string>

#include "npfn.h"
#include "npfn_common.h"
#include "npfn_kernels.h"

namespace {

constexpr int kStrip = 256;  // rows of one observation per workgroup = threads per workgroup
constexpr int kCols = 32;    // columns staged per pass (wider tables take several passes)

// Grid (strips of an observation) x (observations).  Thread t owns row t of the strip.  Per pass of
// up to kCols columns: the strip's [rows, cw] block goes to LDS with flat coalesced loads (dim <=
// kCols: one contiguous run of rows * dim floats) at an odd row stride, so that the column reads
// that follow -- lane t reads word t * stride + c -- hit 64 different banks.  A column's count is a
// ballot per wave; lane 0 parks it in LDS, 2 * cw threads add the four waves and issue one integer
// add each.  Nothing per column lives in registers: the only per-row state carried across the
// columns is the fp64 distance of the TARP column.
// The contraction into an FMA is switched off for the body by the pragma (as in k_box_propose):
// d2 is a chain of separately rounded fp64 multiplies and adds that the host restates bit for bit.
__global__ __launch_bounds__(kStrip) void k_rank_accumulate(
    const float* __restrict__ theta, const float* __restrict__ logp, const uint8_t* __restrict__ take, int64_t per,
    int dim, int stride, const float* __restrict__ theta_true, const float* __restrict__ logp_true,
    const float* __restrict__ ref, const float* __restrict__ inv_scale, unsigned long long* __restrict__ counts,
    int64_t obs0) {
#pragma clang fp contract(off)
  extern __shared__ float tile[];  // [kStrip][stride]
  __shared__ int wcnt[kStrip / 64][kCols][2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t m = obs0 + blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * kStrip;
  const int nrows = (int)(per - r0 < kStrip ? per - r0 : kStrip);
  const int64_t row = m * per + r0 + tid;
  const bool on = tid < nrows && (!take || take[row] != 0);
  const float* __restrict__ src = theta + (m * per + r0) * dim;
  const float* __restrict__ tt = theta_true + m * dim;
  const float* __restrict__ rf = ref ? ref + m * dim : nullptr;
  unsigned long long* __restrict__ out = counts + m * (int64_t)(dim + 2) * 2;
  double d2 = 0.0, d2t = 0.0;

  for (int c0 = 0; c0 < dim; c0 += kCols) {
    const int cw = dim - c0 < kCols ? dim - c0 : kCols;
    {
      // element idx of the [nrows, cw] block = (r, c); idx advances by kStrip per step
      int r = tid / cw, c = tid - r * cw;
      const int dq = kStrip / cw, dr = kStrip - dq * cw;
      for (int idx = tid; idx < nrows * cw; idx += kStrip) {
        tile[r * stride + c] = src[(int64_t)r * dim + c0 + c];
        r += dq;
        c += dr;
        if (c >= cw) {
          c -= cw;
          ++r;
        }
      }
    }
    __syncthreads();
    for (int c = 0; c < cw; ++c) {
      const float v = tile[tid * stride + c];  // rows past nrows: stale words, masked by `on`
      const float t = tt[c0 + c];
      const unsigned long long lt = __ballot(on && v < t);
      const unsigned long long eq = __ballot(on && v == t);
      if (lane == 0) {
        wcnt[w][c][0] = __popcll(lt);
        wcnt[w][c][1] = __popcll(eq);
      }
      if (rf) {
        const double o = (double)rf[c0 + c], sc = (double)inv_scale[c0 + c];
        const double a = ((double)v - o) * sc;
        const double b = ((double)t - o) * sc;
        d2 = d2 + a * a;
        d2t = d2t + b * b;
      }
    }
    __syncthreads();
    if (tid < cw * 2) {
      const int c = tid >> 1, j = tid & 1;
      int s = 0;
      for (int q = 0; q < kStrip / 64; ++q) s += wcnt[q][c][j];
      if (s) atomicAdd(out + (int64_t)(c0 + c) * 2 + j, (unsigned long long)s);
    }
    __syncthreads();
  }

  // columns dim (HPD: draws denser than the truth) and dim + 1 (TARP: draws closer to ref)
  if (logp) {
    const float l = tid < nrows ? logp[row] : 0.f;
    const float lt = logp_true[m];
    const unsigned long long gt = __ballot(on && l > lt);
    const unsigned long long eq = __ballot(on && l == lt);
    if (lane == 0) {
      wcnt[w][0][0] = __popcll(gt);
      wcnt[w][0][1] = __popcll(eq);
    }
  }
  if (rf) {
    const unsigned long long lt = __ballot(on && d2 < d2t);
    const unsigned long long eq = __ballot(on && d2 == d2t);
    if (lane == 0) {
      wcnt[w][1][0] = __popcll(lt);
      wcnt[w][1][1] = __popcll(eq);
    }
  }
  __syncthreads();
  if (tid < 4) {
    const int c = tid >> 1, j = tid & 1;
    if (c == 0 ? logp != nullptr : rf != nullptr) {
      int s = 0;
      for (int q = 0; q < kStrip / 64; ++q) s += wcnt[q][c][j];
      if (s) atomicAdd(out + (int64_t)(dim + c) * 2 + j, (unsigned long long)s);
    }
  }
}

int fail(int code, const std::string& msg) { return npfn::set_error(code, msg.c_str()); }

}  // namespace

extern "C" {

int npfn_rank_accumulate(const float* theta, const float* logp, const uint8_t* take, int64_t n_obs, int64_t per,
                         int32_t dim, const float* theta_true, const float* logp_true, const float* ref,
                         const float* inv_scale, int64_t* counts, void* stream) {
  if (n_obs < 0 || per < 0 || dim < 1)
    return fail(NPFN_EINVAL, "rank_accumulate: need n_obs >= 0, per >= 0 and dim >= 1");
  if ((logp == nullptr) != (logp_true == nullptr))
    return fail(NPFN_EINVAL, "rank_accumulate: logp and logp_true go together (both or neither)");
  if ((ref == nullptr) != (inv_scale == nullptr))
    return fail(NPFN_EINVAL, "rank_accumulate: ref and inv_scale go together (both or neither)");
  if (n_obs == 0 || per == 0) return NPFN_OK;
  if (!theta || !theta_true || !counts) return fail(NPFN_EINVAL, "rank_accumulate: null theta, theta_true or counts");
  const int64_t strips = (per + kStrip - 1) / kStrip;
  if (strips > 0x7fffffffll) return fail(NPFN_EINVAL, "rank_accumulate: too many rows per observation for one launch");
  const int cw = dim < kCols ? dim : kCols;
  const int stride = cw | 1;
  const size_t lds = (size_t)kStrip * stride * sizeof(float);
  for (int64_t m0 = 0; m0 < n_obs; m0 += 65535) {  // the grid's y extent ends at 65535
    const int64_t ny = n_obs - m0 < 65535 ? n_obs - m0 : 65535;
    hipLaunchKernelGGL(k_rank_accumulate, dim3((unsigned)strips, (unsigned)ny), dim3(kStrip), lds,
                       (hipStream_t)stream, theta, logp, take, per, (int)dim, stride, theta_true, logp_true, ref,
                       inv_scale, (unsigned long long*)counts, m0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
      return fail(NPFN_EHIP, std::string("rank_accumulate: k_rank_accumulate launch: ") + hipGetErrorString(e));
  }
  return NPFN_OK;
}

}  // extern "C"
