// npfn_restricted.hip -- the rejection round of NPE_PFN_RestrictedPrior (reference
// restricted_prior.py:8-97 around sbi's rejection loop): box proposals from the Philox row
// stream, the threshold on the classifier's last class, and the ordered append of the accepted
// rows behind the rows of earlier rounds.  The classifier forward between them is
// npfn_predict_proba's own (npfn_engine.hip: npfn_predict_accept, npfn_restricted_box_round).
#include <hip/hip_runtime.h>

#include <string>

#include "npfn.h"
#include "npfn_common.h"
#include "npfn_kernels.h"

namespace {

// out[i][j] = min(low[j] + u * (high[j] - low[j]), high[j]), u = philox_uniform(seed, counter + j,
// row_base + i).  One thread per element.  Subtract, multiply and add are rounded one by one, so
// a float32 restatement gives the same bits.  The contraction into an FMA is switched off for the
// function body by the pragma: __fmul_rn / __fadd_rn do not do it here -- without
// OCML_BASIC_ROUNDED_OPERATIONS the HIP headers define them as the plain operators, which inline
// with the headers' own contraction flags (the ISA of that variant had a v_fmac_f32).  The min
// keeps the point in the closed box when fl(high - low) rounded up.
__global__ __launch_bounds__(256) void k_box_propose(const float* __restrict__ low, const float* __restrict__ high,
                                                     int dim, int64_t n, uint64_t seed, uint64_t counter,
                                                     uint64_t row_base, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * dim) return;
  const int64_t i = idx / dim;
  const int j = (int)(idx - i * dim);
  const float u = philox_uniform(seed, counter + (uint64_t)j, row_base + (uint64_t)i);
  const float lo = low[j], hi = high[j];
  const float span = hi - lo;
  const float t = u * span;
  out[idx] = fminf(lo + t, hi);
}

// mask[i] = probs[i][K - 1] > thr (strict); prob_out[i] (nullable) = that probability
__global__ __launch_bounds__(256) void k_accept_last(const float* __restrict__ probs, int64_t n, int K, float thr,
                                                     uint8_t* __restrict__ mask, float* __restrict__ prob_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float p = probs[i * K + (K - 1)];
  mask[i] = p > thr ? 1 : 0;
  if (prob_out) prob_out[i] = p;
}

// Ordered append with a capacity: the rows of src [n][dim] with mask != 0 go, in input order, to
// dst rows counts[0], counts[0] + 1, ... while those stay below `capacity`; the rest are counted
// only.  counts[0] = min(capacity, counts[0] + accepted), counts[1] += accepted.  One workgroup
// takes the rows in 1024-row passes in order, as k_compact does (a round has about 10^4 rows: ten
// passes), so the order is the input order by construction and no block waits on another.
__global__ __launch_bounds__(1024) void k_append_rows(const float* __restrict__ src, const uint8_t* __restrict__ mask,
                                                      int64_t n, int dim, float* __restrict__ dst, int64_t capacity,
                                                      int64_t* __restrict__ counts) {
  __shared__ int wsum[16];
  __shared__ long long base;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long start = counts[0];
  if (tid == 0) base = start;
  __syncthreads();
  for (int64_t c0 = 0; c0 < n; c0 += 1024) {
    const int64_t i = c0 + tid;
    const bool flag = (i < n) && mask[i] != 0;
    const unsigned long long bal = __ballot(flag);
    const int rank = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int pre = 0, tot = 0;
    for (int q = 0; q < 16; ++q) {
      if (q < w) pre += wsum[q];
      tot += wsum[q];
    }
    const int64_t o = base + pre + rank;
    if (flag && o >= 0 && o < capacity)
      for (int j = 0; j < dim; ++j) dst[o * dim + j] = src[i * dim + j];
    __syncthreads();
    if (tid == 0) base += tot;
    __syncthreads();
  }
  if (tid == 0) {
    counts[0] = base < capacity ? base : (start < capacity ? capacity : start);
    counts[1] += base - start;
  }
}

int fail(int code, const std::string& msg) { return npfn::set_error(code, msg.c_str()); }

}  // namespace

namespace npfn {

void launch_box_propose(const float* low, const float* high, int dim, int64_t n, uint64_t seed, uint64_t counter,
                        uint64_t row_base, float* out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_box_propose, dim3((unsigned)((n * dim + 255) / 256)), dim3(256), 0, s, low, high, dim, n, seed,
                     counter, row_base, out);
}

void launch_accept_last(const float* probs, int64_t n, int K, float thr, uint8_t* mask, float* prob_out,
                        hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_accept_last, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, probs, n, K, thr, mask,
                     prob_out);
}

void launch_append_rows(const float* src, const uint8_t* mask, int64_t n, int dim, float* dst, int64_t capacity,
                        int64_t* counts, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_append_rows, dim3(1), dim3(1024), 0, s, src, mask, n, dim, dst, capacity, counts);
}

}  // namespace npfn

extern "C" {

int npfn_box_propose(const float* low, const float* high, int32_t dim, int64_t n_rows, uint64_t seed,
                     uint64_t counter, int64_t row_base, float* out, void* stream) {
  if (dim < 1 || n_rows < 0 || row_base < 0)
    return fail(NPFN_EINVAL, "box_propose: need dim >= 1, n_rows >= 0 and row_base >= 0");
  if (!low || !high) return fail(NPFN_EINVAL, "box_propose: null bounds");
  if (n_rows == 0) return NPFN_OK;
  if (!out) return fail(NPFN_EINVAL, "box_propose: null output");
  if (n_rows > (0x7fffffffll * 256) / dim) return fail(NPFN_EINVAL, "box_propose: too many values for one launch");
  npfn::launch_box_propose(low, high, dim, n_rows, seed, counter, (uint64_t)row_base, out, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NPFN_EHIP, std::string("box_propose: k_box_propose launch: ") + hipGetErrorString(e));
  return NPFN_OK;
}

}  // extern "C"
