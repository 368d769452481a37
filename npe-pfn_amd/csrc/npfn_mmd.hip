// npfn_mmd.hip -- MMD two-sample test (npe_pfn.diagnostics.mmd_batched): the kernel values of every
// ordered pair of an observation's pooled sample, quantised to integers and folded into the
// within-group sums of many labellings (the observed split and its permutations) without the
// N x N kernel matrix or an N x P product ever reaching global memory.  The statement of every
// number is in include/npfn.h (npfn_mmd_sums); npe_pfn.diagnostics.mmd_sums_host restates it in
// torch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "npfn.h"
#include "npfn_common.h"
#include "npfn_kernels.h"

namespace {

constexpr int kTile = 64;        // points per tile edge = lanes of a wave
constexpr int kThreads = 256;    // four waves; wave w computes rows 16 w .. 16 w + 15 of a q tile
constexpr int kSlab = 256;       // labellings per workgroup: thread t owns labelling slab * 256 + t
constexpr int kStrip = 8;        // tiles J of one workgroup (its sums stay in registers across them)
constexpr int kRowBytes = 4 * kTile;  // a row of the q tile: four byte planes of 64 points
constexpr int kJStride = kTile + 1;   // row stride of the transposed J tile: conflict-free both ways
constexpr int kMaxBw = 8;
constexpr int kMaxDim = 64;
constexpr int kMaxLabel = 4096;
constexpr int64_t kMaxPool = 32768;   // N^2 pairs x 2^31 per pair <= 2^61
constexpr double kScale = 0x1p28;     // q = sum_b llrint(k_b * 2^28)

struct MmdParams {
  float c[kMaxBw];   // rbf: fl(-0.5 / a_b); multiscale: fl(a_b * a_b)
  int n_bw;
  int kernel;
};

__device__ __forceinline__ bool not_finite(float v) { return !(fabsf(v) <= 3.4028234663852886e38f); }

// The labels of labellings p0 .. p0 + 63 (p0 wave-uniform) at the npts points from pt0, as one
// 64-bit mask per labelling: the wave reads 64 consecutive bytes of a labelling, a ballot packs
// them, and lane r keeps the mask of labelling p0 + r.  Points past npts and labellings past
// n_label read nothing and get 0.
__device__ __forceinline__ unsigned long long label_masks(const uint8_t* __restrict__ labels, int n_label, int64_t N,
                                                          int p0, int64_t pt0, int npts, int lane) {
  unsigned long long mine = 0ull;
  const bool pt = lane < npts;
#pragma unroll 8
  for (int r = 0; r < 64; ++r) {
    const int p = p0 + r;
    const bool on = pt && p < n_label && labels[(int64_t)p * N + pt0 + lane] != 0;
    const unsigned long long b = __ballot(on);
    if (lane == r) mine = b;
  }
  return mine;
}

// Grid (tile I, strip of tiles J >= I, observation x slab of labellings).  The workgroup keeps tile
// I's coordinates in LDS as [point][k] (read by broadcast) and, per tile J of its strip, tile J's
// as [k][point] (lane j reads word k * 65 + j).  Thread (w, lane) forms d2 of the 16 pairs (16 w +
// r, lane) in registers, k ascending, every subtract, multiply and add rounded on its own (plain
// operators under the pragma that switches the contraction into FMAs off for this body, as in
// k_rank_accumulate; the __f*_rn intrinsics are inline functions of a header the pragma does not
// reach, and were contracted), and writes their q (0 for points past the end of the pool) into an LDS tile
// cut into byte planes: row i holds byte 0 of its 64 q, then byte 1, 2 and 3.  One wave sums the
// tile's rows (rotated reads: 64 banks).  Then thread t folds the tile into labelling slab * 256 +
// t: with mi / mj its labels of the two tiles as bit masks and mj spread to one byte per point,
// row i gives a_i = sum of q(i, j) over the j in mj as four byte-plane sums, each a chain of 16
// v_dot4_u32_u8 (at most 64 * 255 per plane: exact in 32 bits) on 16-byte LDS reads that every
// thread makes at the same address (a broadcast), recombined with shifts in 64 bits; a_i goes to
// group 1 when i is in mi and rowsum_i - a_i to group 0 otherwise.  An off-diagonal tile stands
// for (I, J) and (J, I): q is bitwise symmetric, so it counts twice.  Last, one 64-bit integer
// add per non-zero counter: the result does not depend on which workgroup arrives first.
__global__ __launch_bounds__(kThreads) void k_mmd_sums(const float* __restrict__ z, int N, int dim, MmdParams prm,
                                                       const uint8_t* __restrict__ labels, int n_label, int slabs,
                                                       int64_t obs0, unsigned long long* __restrict__ sums,
                                                       unsigned long long* __restrict__ total,
                                                       int* __restrict__ bad) {
#pragma clang fp contract(off)
  extern __shared__ float zs[];   // zI [kTile][dim], zJ [dim][kJStride]
  __shared__ __attribute__((aligned(16))) uint8_t qb[kTile * kRowBytes];   // [row][byte plane][point]
  __shared__ unsigned long long rowsum[kTile];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nT = (N + kTile - 1) / kTile;
  const int I = blockIdx.x;
  const int J0 = I + (int)blockIdx.y * kStrip;
  if (J0 >= nT) return;   // uniform over the workgroup
  const int J1 = min(J0 + kStrip, nT);
  const int uz = blockIdx.z / slabs, slab = blockIdx.z - uz * slabs;
  const int64_t u = obs0 + uz;
  const float* __restrict__ zu = z + u * N * dim;
  float* zI = zs;
  float* zJ = zs + kTile * dim;
  const int nI = min(kTile, N - I * kTile);
  const int p = slab * kSlab + tid;
  const bool active = p < n_label;
  bool nonfinite = false;

  for (int idx = tid; idx < kTile * dim; idx += kThreads) {
    const float v = idx < nI * dim ? zu[(int64_t)I * kTile * dim + idx] : 0.f;
    nonfinite |= not_finite(v);
    zI[idx] = v;
  }
  const unsigned long long mi = label_masks(labels, n_label, N, slab * kSlab + w * 64, (int64_t)I * kTile, nI, lane);

  unsigned long long s0 = 0ull, s1 = 0ull, tot = 0ull;
  for (int J = J0; J < J1; ++J) {
    const int nJ = min(kTile, N - J * kTile);
    for (int idx = tid; idx < kTile * dim; idx += kThreads) {
      const int r = idx / dim, k = idx - r * dim;
      const float v = r < nJ ? zu[(int64_t)J * kTile * dim + idx] : 0.f;
      nonfinite |= not_finite(v);
      zJ[k * kJStride + r] = v;
    }
    const unsigned long long mj =
        J == I ? mi : label_masks(labels, n_label, N, slab * kSlab + w * 64, (int64_t)J * kTile, nJ, lane);
    __syncthreads();

    {
      float acc[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      for (int k = 0; k < dim; ++k) {
        const float zj = zJ[k * kJStride + lane];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float t = zI[(w * 16 + r) * dim + k] - zj;
          const float tt = t * t;
          acc[r] = acc[r] + tt;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = w * 16 + r;
        uint32_t qq = 0u;
        if (i < nI && lane < nJ) {
          for (int b = 0; b < prm.n_bw; ++b) {
            const float cb = prm.c[b];
            const float arg = acc[r] * cb, den = cb + acc[r];
            const float kb = prm.kernel == 0 ? expf(arg) : cb / den;
            qq += (uint32_t)llrint((double)kb * kScale);
          }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) qb[i * kRowBytes + b * kTile + lane] = (uint8_t)(qq >> (8 * b));
      }
    }
    __syncthreads();
    if (tid < kTile) {
      const uint32_t* __restrict__ mine = reinterpret_cast<const uint32_t*>(qb + tid * kRowBytes);
      unsigned long long rs = 0ull;
      for (int jj = 0; jj < kTile; ++jj) {
        const int wd = (jj + tid) & (kTile - 1);   // word wd: points 4 (wd & 15) .. + 3 of plane wd >> 4
        rs += (unsigned long long)__builtin_amdgcn_udot4(mine[wd], 0x01010101u, 0u, false) << (8 * (wd >> 4));
      }
      rowsum[tid] = rs;
    }
    __syncthreads();

    if (active) {
      uint32_t lb[kTile / 4];   // mj, one byte (0 / 1) per point
#pragma unroll
      for (int j4 = 0; j4 < kTile / 4; ++j4) {
        const uint32_t nib = (uint32_t)(mj >> (4 * j4)) & 0xfu;
        lb[j4] = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
      }
      unsigned long long t0 = 0ull, t1 = 0ull, rt = 0ull;
      for (int i = 0; i < kTile; ++i) {
        const uint4* __restrict__ row = reinterpret_cast<const uint4*>(qb + i * kRowBytes);
        uint32_t ab[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          uint32_t acc = 0u;
#pragma unroll
          for (int j16 = 0; j16 < 4; ++j16) {
            const uint4 v = row[4 * b + j16];
            acc = __builtin_amdgcn_udot4(v.x, lb[4 * j16 + 0], acc, false);
            acc = __builtin_amdgcn_udot4(v.y, lb[4 * j16 + 1], acc, false);
            acc = __builtin_amdgcn_udot4(v.z, lb[4 * j16 + 2], acc, false);
            acc = __builtin_amdgcn_udot4(v.w, lb[4 * j16 + 3], acc, false);
          }
          ab[b] = acc;
        }
        // ab[b] <= 64 * 255 < 2^14: the lower three planes fit 32 bits together
        const unsigned long long a =
            (unsigned long long)(ab[0] + (ab[1] << 8) + (ab[2] << 16)) + ((unsigned long long)ab[3] << 24);
        const unsigned long long rs = rowsum[i];
        rt += rs;
        if ((mi >> i) & 1ull) t0 += a; else t1 += rs - a;
      }
      const unsigned long long wgt = J == I ? 1ull : 2ull;
      s0 += wgt * t0;
      s1 += wgt * t1;
      tot += wgt * rt;
    }
    __syncthreads();   // the next tile J overwrites zJ, qb and rowsum
  }

  if (active) {
    unsigned long long* __restrict__ dst = sums + (u * n_label + p) * 2;
    if (s0) atomicAdd(dst, s0);
    if (s1) atomicAdd(dst + 1, s1);
  }
  if (slab == 0 && tid == 0 && tot) atomicAdd(total + u, tot);
  if (nonfinite) bad[u] = 1;
}

int fail(int code, const std::string& msg) { return npfn::set_error(code, msg.c_str()); }

}  // namespace

extern "C" {

int npfn_mmd_sums(const float* z, int64_t n_obs, int64_t n_pool, int32_t dim, int32_t kernel,
                  const float* bandwidths, int32_t n_bw, const uint8_t* labels, int32_t n_label, int64_t* sums,
                  int64_t* total, int32_t* bad, void* stream) {
  if (n_obs < 0) return fail(NPFN_EINVAL, "mmd_sums: need n_obs >= 0");
  if (n_pool < 1 || n_pool > kMaxPool)
    return fail(NPFN_EINVAL, "mmd_sums: n_pool must lie in 1.." + std::to_string(kMaxPool) +
                                 " (the int64 headroom of N^2 sums of at most 2^31)");
  if (dim < 1 || dim > kMaxDim) return fail(NPFN_EINVAL, "mmd_sums: dim must lie in 1.." + std::to_string(kMaxDim));
  if (kernel != 0 && kernel != 1) return fail(NPFN_EINVAL, "mmd_sums: kernel must be 0 (rbf) or 1 (multiscale)");
  if (n_bw < 1 || n_bw > kMaxBw) return fail(NPFN_EINVAL, "mmd_sums: n_bw must lie in 1.." + std::to_string(kMaxBw));
  if (n_label < 1 || n_label > kMaxLabel)
    return fail(NPFN_EINVAL, "mmd_sums: n_label must lie in 1.." + std::to_string(kMaxLabel));
  if (!z || !bandwidths || !labels || !sums || !total || !bad)
    return fail(NPFN_EINVAL, "mmd_sums: null z, bandwidths, labels, sums, total or bad");
  MmdParams prm{};
  prm.n_bw = n_bw;
  prm.kernel = kernel;
  for (int b = 0; b < n_bw; ++b) {
    const float a = bandwidths[b];
    if (!std::isfinite(a) || !(a > 0.f))
      return fail(NPFN_EINVAL, "mmd_sums: bandwidth " + std::to_string(b) + " is not finite and > 0");
    prm.c[b] = kernel == 0 ? -0.5f / a : a * a;
  }
  if (n_obs == 0) return NPFN_OK;

  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(sums, 0, (size_t)n_obs * n_label * 2 * sizeof(int64_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(total, 0, (size_t)n_obs * sizeof(int64_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(bad, 0, (size_t)n_obs * sizeof(int32_t), s);
  if (e != hipSuccess) return fail(NPFN_EHIP, std::string("mmd_sums: hipMemsetAsync: ") + hipGetErrorString(e));

  const int N = (int)n_pool;
  const int nT = (N + kTile - 1) / kTile;
  const int slabs = (n_label + kSlab - 1) / kSlab;
  const int64_t obs_per_launch = 65535 / slabs;   // the grid's z extent ends at 65535
  const size_t lds = (size_t)(kTile * dim + dim * kJStride) * sizeof(float);
  for (int64_t m0 = 0; m0 < n_obs; m0 += obs_per_launch) {
    const int64_t nz = n_obs - m0 < obs_per_launch ? n_obs - m0 : obs_per_launch;
    hipLaunchKernelGGL(k_mmd_sums, dim3((unsigned)nT, (unsigned)((nT + kStrip - 1) / kStrip), (unsigned)(nz * slabs)),
                       dim3(kThreads), lds, s, z, N, (int)dim, prm, labels, (int)n_label, slabs, m0,
                       (unsigned long long*)sums, (unsigned long long*)total, (int*)bad);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(NPFN_EHIP, std::string("mmd_sums: k_mmd_sums launch: ") + hipGetErrorString(e));
  }
  return NPFN_OK;
}

}  // extern "C"
