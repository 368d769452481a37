// npfn_pairs.hip -- 2-D posterior marginals (NPE_PFN_Core.pair_marginals): the sampler's row
// mixtures re-binned onto a coarse grid of G cells (k_bar_cell_mass) and folded, keyed by the cells
// of the rows' earlier draws, into per-observation integer tables (k_pair_accumulate) that
// k_pair_final turns into fp32 masses.  The statement of every number is in include/npfn.h
// (npfn_bar_cell_mass, npfn_pair_accumulate); npe_pfn.pair_marginals.pair_accumulate_host restates
// the accumulation in torch.
#include <hip/hip_runtime.h>

#include <string>

#include "npfn.h"
#include "npfn_common.h"
#include "npfn_kernels.h"

namespace {

constexpr int kMaxCells = 128;            // G <= 128: the G + 1 CDF values of a row live in LDS
constexpr int kPairRows = 256;            // rows of one observation per workgroup (a strip)
constexpr int kPairTabCells = 4096;       // int64 cells of a workgroup's table: 32 KB of LDS
constexpr double kPairScale = 0x1p40;     // q = llrint(w * 2^40)

// The NLL's bucket rule on plain borders b[0..nb] (bar_cdf_bucket of npfn_kernels.hip with scale 1
// and shift 0): searchsorted left - 1, the two end-border fix-ups, clamped.
__device__ __forceinline__ int cell_bucket(const float* __restrict__ b, int nb, float e) {
  int lo = 0, hi = nb + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (b[mid] < e) lo = mid + 1; else hi = mid;
  }
  int j = lo - 1;
  if (e == b[0]) j = 0;
  if (e == b[nb]) j = nb - 1;
  return min(max(j, 0), nb - 1);
}

// One workgroup per row.  The row's nb masses go to LDS with coalesced loads; thread t owns the
// `chunk` consecutive bars from t * chunk (chunk odd, so that the 32 lanes of an LDS lane group
// read 32 different banks) and sums them in bar order in fp64; a Hillis-Steele scan over the 256
// thread sums (double-buffered in LDS, the same additions whatever the launch) gives every
// thread's exclusive prefix and the total.  Thread t <= G then answers edge t: L(j) = its owner's
// prefix + the owner's bars before j, F = (L + p[j] * frac) / tot, always from the left; threads
// t < G write the differences.
__global__ __launch_bounds__(256) void k_bar_cell_mass(const float* __restrict__ probs,
                                                       const float* __restrict__ borders, int nb, int chunk,
                                                       const float* __restrict__ edges, int G,
                                                       double* __restrict__ w) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* scan = reinterpret_cast<double*>(smem);   // [2][256]
  double* F = scan + 512;                           // [kMaxCells + 1], padded to 132
  float* p = reinterpret_cast<float*>(F + 132);     // [nb]
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* __restrict__ src = probs + row * nb;
  for (int b = tid; b < nb; b += 256) p[b] = src[b];
  __syncthreads();
  {
    const int b0 = min(tid * chunk, nb), b1 = min(b0 + chunk, nb);
    double acc = 0.0;
    for (int b = b0; b < b1; ++b) acc += (double)p[b];
    scan[tid] = acc;
  }
  __syncthreads();
  int cur = 0;
  for (int off = 1; off < 256; off <<= 1) {
    const double v = scan[cur * 256 + tid] + (tid >= off ? scan[cur * 256 + tid - off] : 0.0);
    scan[(cur ^ 1) * 256 + tid] = v;
    cur ^= 1;
    __syncthreads();
  }
  const double* incl = scan + cur * 256;
  const double tot = incl[255];
  const bool ok = tot > 0.0 && tot < (double)INFINITY;
  if (tid <= G && ok) {
    const float e = edges[tid];
    const int j = cell_bucket(borders, nb, e);
    const int owner = j / chunk;
    double L = owner > 0 ? incl[owner - 1] : 0.0;
    for (int b = owner * chunk; b < j; ++b) L += (double)p[b];
    const double left = (double)borders[j], right = (double)borders[j + 1];
    const double wd = right - left;
    double frac = 1.0;   // the share of bar j left of e (bar_cdf_finish's rules)
    if (wd > 0.0) {
      if (j == 0) {                  // half-normal hanging left from b[1]
        frac = erfc(fmax(right - (double)e, 0.0) / (wd / NPFN_HALFNORMAL_MEDIAN * M_SQRT2));
      } else if (j == nb - 1) {      // half-normal hanging right from b[nb - 1]
        frac = erf(fmax((double)e - left, 0.0) / (wd / NPFN_HALFNORMAL_MEDIAN * M_SQRT2));
      } else {
        frac = fmin(fmax(((double)e - left) / wd, 0.0), 1.0);
      }
    }
    F[tid] = (L + (double)p[j] * frac) / tot;
  }
  __syncthreads();
  if (tid < G) w[row * G + tid] = ok ? fmax(F[tid + 1] - F[tid], 0.0) : (double)NAN;
}

// Grid (strips touched by the window) x (earlier dimension j, slab of the a-axis).  A strip is
// kPairRows consecutive rows of one observation, counted from the observation's first row, clipped
// to the window; strip sid0 + blockIdx.x belongs to observation sid / S.  The workgroup keeps the
// slab [na][G] of pairQ[u][j] in LDS as int64, followed by G cell sums (used by blockIdx.y == 0,
// which also raises bad[u]).  Row i's cell in dimension j is found once (thread i, binary search);
// then the strip's [n][G] block of w is swept flat -- coalesced 8-byte loads -- and every element
// is quantised and added with a 64-bit LDS integer add; last, one 64-bit global integer add per
// non-zero cell.  Integer sums: the result does not depend on which workgroup or wave arrives
// first, and no workgroup waits on another.
__global__ __launch_bounds__(kPairRows) void k_pair_accumulate(
    const double* __restrict__ w, const float* __restrict__ theta, int64_t ldt, int n_prev,
    const float* __restrict__ edges, int G, int SA, int slabs, int64_t r0, int64_t n_rows, int64_t per, int64_t S,
    int64_t sid0, unsigned long long* __restrict__ pairQ, unsigned long long* __restrict__ cellQ,
    int* __restrict__ bad) {
  extern __shared__ unsigned long long tab[];  // [na][G] pair cells, then [G] cell sums
  __shared__ int acell[kPairRows];
  __shared__ int rowbad[kPairRows];
  const int tid = threadIdx.x;
  const int64_t sid = sid0 + blockIdx.x, u = sid / S, st = sid - u * S;
  const int64_t g0 = u * per + st * kPairRows;
  const int64_t e1 = (st + 1) * kPairRows, g1 = u * per + (e1 < per ? e1 : per);
  const int64_t lo = g0 > r0 ? g0 : r0, hi = g1 < r0 + n_rows ? g1 : r0 + n_rows;
  if (hi <= lo) return;   // uniform over the workgroup
  const int n = (int)(hi - lo);
  const int j = blockIdx.y / slabs, a0 = (blockIdx.y - j * slabs) * SA;
  const int na = n_prev > 0 ? min(SA, G - a0) : 0;
  const bool first = blockIdx.y == 0;
  unsigned long long* cells = tab + na * G;
  for (int i = tid; i < na * G + G; i += kPairRows) tab[i] = 0ull;
  if (tid < n) {
    rowbad[tid] = 0;
    int a = -1;
    if (n_prev > 0) {
      const float th = theta[(lo - r0 + tid) * ldt + j];
      const float* __restrict__ ed = edges + (int64_t)j * (G + 1);
      int l = 0, h = G + 1;   // the number of edges <= th
      while (l < h) {
        const int mid = (l + h) >> 1;
        if (ed[mid] <= th) l = mid + 1; else h = mid;
      }
      a = (th == th && l >= 1 && l <= G) ? l - 1 : -1;   // below e[0], at or above e[G], NaN: no cell
    }
    acell[tid] = a;
  }
  __syncthreads();
  const double* __restrict__ wr = w + (lo - r0) * G;
  for (int idx = tid; idx < n * G; idx += kPairRows) {
    const double v = wr[idx];
    if (v != v) rowbad[idx / G] = 1;
  }
  __syncthreads();
  for (int idx = tid; idx < n * G; idx += kPairRows) {
    const int i = idx / G, c = idx - i * G;
    if (rowbad[i]) continue;
    const unsigned long long q = (unsigned long long)llrint(wr[idx] * kPairScale);
    if (q == 0ull) continue;
    if (first) atomicAdd(&cells[c], q);
    const int a = acell[i] - a0;
    if (a >= 0 && a < na) atomicAdd(&tab[a * G + c], q);
  }
  __syncthreads();
  unsigned long long* __restrict__ dst = pairQ + ((u * n_prev + j) * G + a0) * (int64_t)G;
  for (int i = tid; i < na * G; i += kPairRows) {
    const unsigned long long v = tab[i];
    if (v) atomicAdd(dst + i, v);
  }
  if (first) {
    for (int c = tid; c < G; c += kPairRows) {
      const unsigned long long v = cells[c];
      if (v) atomicAdd(cellQ + u * G + c, v);
    }
    if (tid < n && rowbad[tid]) bad[u] = 1;
  }
}

// grid (observations, tiles of the observation's `inner` sums)
__global__ __launch_bounds__(256) void k_pair_final(const long long* __restrict__ Q, const int* __restrict__ bad,
                                                    int64_t inner, int64_t per, float* __restrict__ out,
                                                    int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x, u = blockIdx.x;
  if (i >= inner) return;
  out[u * ldo + i] = bad[u] ? NAN : (float)((double)Q[u * inner + i] / (kPairScale * (double)per));
}

int fail(int code, const std::string& msg) { return npfn::set_error(code, msg.c_str()); }

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NPFN_EHIP, std::string(what) + " launch: " + hipGetErrorString(e));
  return NPFN_OK;
}

}  // namespace

namespace npfn {

int cell_mass_max_bars() { return (65536 - (512 + 132) * (int)sizeof(double)) / (int)sizeof(float); }

void launch_bar_cell_mass(const float* probs, const float* borders, int64_t rows, int nb, const float* edges, int G,
                          double* w, hipStream_t s) {
  if (rows <= 0) return;
  const int chunk = ((nb + 255) / 256) | 1;
  const size_t lds = (512 + 132) * sizeof(double) + (size_t)nb * sizeof(float);
  hipLaunchKernelGGL(k_bar_cell_mass, dim3((unsigned)rows), dim3(256), lds, s, probs, borders, nb, chunk, edges, G, w);
}

void launch_pair_accumulate(const double* w, const float* theta, int64_t ldt, int n_prev, const float* edges, int G,
                            int64_t r0, int64_t rows, int64_t per, int64_t* pairQ, int64_t* cellQ, int32_t* bad,
                            hipStream_t s) {
  if (rows <= 0) return;
  const int64_t S = (per + kPairRows - 1) / kPairRows;
  auto strip_of = [&](int64_t g) { return (g / per) * S + (g % per) / kPairRows; };
  const int64_t sid0 = strip_of(r0), n_strips = strip_of(r0 + rows - 1) - sid0 + 1;
  const int SA = std::min(G, kPairTabCells / G), slabs = (G + SA - 1) / SA;
  const size_t lds = ((size_t)(n_prev > 0 ? SA : 0) * G + G) * sizeof(unsigned long long);
  hipLaunchKernelGGL(k_pair_accumulate, dim3((unsigned)n_strips, (unsigned)(std::max(n_prev, 1) * slabs)),
                     dim3(kPairRows), lds, s, w, theta, ldt, n_prev, edges, G, SA, slabs, r0, rows, per, S, sid0,
                     (unsigned long long*)pairQ, (unsigned long long*)cellQ, (int*)bad);
}

void launch_pair_final(const int64_t* Q, const int32_t* bad, int64_t n_unique, int64_t inner, int64_t per, float* out,
                       int64_t ldo, hipStream_t s) {
  if (n_unique <= 0 || inner <= 0) return;
  hipLaunchKernelGGL(k_pair_final, dim3((unsigned)n_unique, (unsigned)((inner + 255) / 256)), dim3(256), 0, s,
                     (const long long*)Q, (const int*)bad, inner, per, out, ldo);
}

int pair_check_cells(int32_t n_cells, int64_t per, const char* who) {
  if (n_cells < 2 || n_cells > kMaxCells)
    return fail(NPFN_EINVAL, std::string(who) + ": n_cells must lie in 2.." + std::to_string(kMaxCells));
  if (per > kPairMaxPer)
    return fail(NPFN_EINVAL, std::string(who) + ": more than 2^22 rows per observation (the int64 headroom of the "
                                                "2^40-scaled sums)");
  return NPFN_OK;
}

}  // namespace npfn

using namespace npfn;

extern "C" {

int npfn_bar_cell_mass(const float* probs, const float* borders, int64_t n_rows, int32_t n_bars, const float* edges,
                       int32_t n_cells, double* w_out, void* stream) {
  if (n_rows < 0 || n_bars < 2 || n_bars > cell_mass_max_bars())
    return fail(NPFN_EINVAL, "bar_cell_mass: need n_rows >= 0 and 2 <= n_bars <= " +
                                 std::to_string(cell_mass_max_bars()));
  if (int rc = pair_check_cells(n_cells, 1, "bar_cell_mass")) return rc;
  if (n_rows > 0x7fffffffll) return fail(NPFN_EINVAL, "bar_cell_mass: too many rows for one launch");
  if (!probs || !borders || !edges || !w_out)
    return fail(NPFN_EINVAL, "bar_cell_mass: null probs, borders, edges or w_out");
  if (n_rows == 0) return NPFN_OK;
  launch_bar_cell_mass(probs, borders, n_rows, n_bars, edges, n_cells, w_out, (hipStream_t)stream);
  return launched("bar_cell_mass: k_bar_cell_mass");
}

int npfn_pair_accumulate(const double* w, const float* theta, int64_t ldt, int32_t n_prev, const float* edges,
                         int32_t n_cells, int64_t r0, int64_t n_rows, int64_t per, int64_t* pairQ, int64_t* cellQ,
                         int32_t* bad, void* stream) {
  if (r0 < 0 || n_rows < 0 || per < 1 || n_prev < 0 || ldt < n_prev)
    return fail(NPFN_EINVAL, "pair_accumulate: need r0 >= 0, n_rows >= 0, per >= 1 and 0 <= n_prev <= ldt");
  if (int rc = pair_check_cells(n_cells, per, "pair_accumulate")) return rc;
  if ((int64_t)n_prev * 4 > 65535) return fail(NPFN_EINVAL, "pair_accumulate: n_prev too large for one launch");
  if (!w || !cellQ || !bad || (n_prev > 0 && (!theta || !edges || !pairQ)))
    return fail(NPFN_EINVAL, "pair_accumulate: null w, theta, edges, pairQ, cellQ or bad");
  if (n_rows == 0) return NPFN_OK;
  if (n_rows / kPairRows + (r0 + n_rows) / per + 2 > 0x7fffffffll)
    return fail(NPFN_EINVAL, "pair_accumulate: too many rows for one launch");
  launch_pair_accumulate(w, theta, ldt, n_prev, edges, n_cells, r0, n_rows, per, pairQ, cellQ, bad,
                         (hipStream_t)stream);
  return launched("pair_accumulate: k_pair_accumulate");
}

}  // extern "C"
