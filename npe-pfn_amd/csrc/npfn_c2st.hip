// npfn_c2st.hip -- classifier two-sample test (npe_pfn.diagnostics.c2st_batched): one workgroup
// trains and scores the small ReLU MLP of one (observation, fold) in a single launch -- weights,
// activations and back-propagated errors in LDS, gradients and Adam state in registers.  The
// statement of every number is in include/npfn.h (npfn_c2st_fit); npe_pfn.diagnostics.c2st_fit_host
// restates it in torch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "npfn.h"
#include "npfn_common.h"
#include "npfn_kernels.h"

namespace {

constexpr int kThreads = 512;     // eight waves: two per SIMD, 256 registers each
constexpr int kRows = 16;         // rows of a tile: thread (unit, row group) computes 4 of them
constexpr int kMaxLayers = 5;
constexpr int kMaxWidth = 128;    // units per layer: one pass of 128 units x 4 row groups
constexpr int kMaxDim = 64;
constexpr int kMaxParams = 16384;
constexpr int kSlots = 3;         // 4 x 4 tiles of dW per thread (<= 1232 tiles at the caps)
constexpr int kMaxPool = 32768;
constexpr int kMaxFolds = 16;
constexpr int kMaxBatch = 4096;
constexpr size_t kLdsLimit = 160 * 1024;

// The padded network.  Layer l maps width[l] inputs to width[l + 1] units.  Its LDS image is
// rows[l] = roundup(width[l + 1], 4) rows of a_stride[l] = roundup(width[l] + 1, 4) floats: W[o][.],
// then the bias in column width[l], then zeros.  Activations of layer l are kRows rows of
// a_stride[l] floats with a constant 1 in column width[l] and zeros behind it (the logits: 4
// floats); the errors of layer l >= 1 are kRows rows of d_stride[l] = roundup(width[l], 4).  Padding
// entries are parameters that start at 0 and whose gradient is exactly 0, so they stay 0.
struct Net {
  int n_layers, n_params, n_tiles;
  int width[kMaxLayers + 1];
  int a_stride[kMaxLayers + 1], a_off[kMaxLayers + 1];
  int d_stride[kMaxLayers + 1], d_off[kMaxLayers + 1];
  int w_off[kMaxLayers], p_off[kMaxLayers + 1], tile_off[kMaxLayers + 1];
  int w_floats, a_floats, d_floats;
};

struct FoldSizes {
  int n_train[kMaxFolds];
};

__device__ __forceinline__ bool not_finite(float v) { return !(fabsf(v) <= 3.4028234663852886e38f); }

// LDS index of parameter p of the flat vector (layer by layer W [out, in] row-major, then b [out])
__device__ __forceinline__ int param_slot(const Net& sn, int p) {
  int l = 0;
  while (l + 1 < sn.n_layers && p >= sn.p_off[l + 1]) ++l;
  const int q = p - sn.p_off[l], in = sn.width[l], out = sn.width[l + 1];
  int o, i;
  if (q < out * in) {
    o = q / in;
    i = q - o * in;
  } else {
    o = q - out * in;
    i = in;
  }
  return sn.w_off[l] + o * sn.a_stride[l] + i;
}

// act_{l + 1} = relu(W_l act_l + b_l) for every layer (no relu on the logits), on the kRows rows
// whose inputs are in act_0.  Thread (o = tid & 127, rg = tid >> 7) forms unit o of rows 4 rg .. 4
// rg + 3: i ascending in chains of fmaf, the bias last (the 1 column).  Ends on a barrier.
__device__ __forceinline__ void forward_tile(const Net& sn, const float* __restrict__ Ws, float* __restrict__ As,
                                             int tid) {
  const int o = tid & (kMaxWidth - 1), rg = tid >> 7;
  for (int l = 0; l < sn.n_layers; ++l) {
    const int S = sn.a_stride[l], S1 = sn.a_stride[l + 1], s4 = S >> 2;
    if (o < sn.width[l + 1]) {
      const float4* __restrict__ w = reinterpret_cast<const float4*>(Ws + sn.w_off[l] + o * S);
      const float4* __restrict__ a = reinterpret_cast<const float4*>(As + sn.a_off[l] + rg * 4 * S);
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2   // two iterations' LDS reads in flight (-9 %, same bits); 4 spills
      for (int i4 = 0; i4 < s4; ++i4) {
        const float4 wv = w[i4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 av = a[j * s4 + i4];
          acc[j] = fmaf(wv.x, av.x, acc[j]);
          acc[j] = fmaf(wv.y, av.y, acc[j]);
          acc[j] = fmaf(wv.z, av.z, acc[j]);
          acc[j] = fmaf(wv.w, av.w, acc[j]);
        }
      }
      const bool relu = l + 1 < sn.n_layers;
      float* __restrict__ dst = As + sn.a_off[l + 1] + rg * 4 * S1 + o;
#pragma unroll
      for (int j = 0; j < 4; ++j) dst[j * S1] = relu && acc[j] < 0.f ? 0.f : acc[j];   // a NaN stays
    }
    __syncthreads();
  }
}

// Rows r < n_rows of act_0 <- pooled points idx(r) of the observation; the other rows <- 0.
template <class Idx>
__device__ __forceinline__ void load_rows(const Net& sn, float* __restrict__ As, const float* __restrict__ zu, int dim,
                                          int n_pool, int n_rows, int tid, Idx idx) {
  const int S = sn.a_stride[0];
  for (int e = tid; e < kRows * dim; e += kThreads) {
    const int r = e / dim, k = e - r * dim;
    float v = 0.f;
    if (r < n_rows) {
      const int p = min(max(idx(r), 0), n_pool - 1);
      v = zu[(int64_t)p * dim + k];
    }
    As[sn.a_off[0] + r * S + k] = v;
  }
}

__device__ __forceinline__ float sigmoidf(float d) {   // 1 / (1 + exp(-d)) without overflow
  const float e = expf(-fabsf(d));
  return d >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// Grid: one workgroup per (observation, fold).  See include/npfn.h for the definition; the layout:
//  - forward: forward_tile on a tile of kRows batch rows read from global memory;
//  - loss and the logits' errors: threads 0..15, one row each; thread 0 adds the rows' losses in
//    row order;
//  - backward: thread (i, rg) forms the error of unit i of layer l on its 4 rows from the errors of
//    layer l + 1 (o ascending) and gates it by the unit's activation;
//  - gradient: the 4 x 4 tiles of every layer's padded [W | b] are dealt to the threads, tile t to
//    thread t % 512, slot t / 512; a thread adds error x activation over the rows of the tile, then
//    over the tiles of the batch, in registers, where the same entries' Adam moments live for the
//    whole training; after the last tile of a batch it updates its entries in LDS.
__global__ __launch_bounds__(kThreads) void k_c2st_fit(const float* __restrict__ z, int n_pool, int n_first, int dim,
                                                       Net net, const float* __restrict__ init,
                                                       const uint8_t* __restrict__ fold, int n_folds,
                                                       const int* __restrict__ order, FoldSizes fs, int order_ld,
                                                       int epochs, int batch, const float* __restrict__ adam,
                                                       float beta1, float beta2, float eps, float weight_decay,
                                                       int64_t obs0, int* __restrict__ correct,
                                                       float* __restrict__ loss, float* __restrict__ prob,
                                                       float* __restrict__ params_out, int* __restrict__ bad) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ Net sn;
  __shared__ float row_loss[kRows];
  __shared__ int row_label[kRows];
  const int tid = threadIdx.x;
  const int f = (int)(blockIdx.x % (unsigned)n_folds);
  const int64_t u = obs0 + blockIdx.x / (unsigned)n_folds;
  const float* __restrict__ zu = z + u * n_pool * dim;
  const int n_train = fs.n_train[f];

  bool nonfinite = false;
  for (int e = tid; e < n_pool * dim; e += kThreads) nonfinite |= not_finite(zu[e]);
  if (tid == 0) sn = net;
  if (__syncthreads_or(nonfinite)) {   // uniform: every fold of the observation leaves here
    if (tid == 0) bad[u] = 1;
    return;
  }

  float* __restrict__ Ws = smem;
  float* __restrict__ As = Ws + sn.w_floats;
  float* __restrict__ Ds = As + sn.a_floats;
  const int L = sn.n_layers, P = sn.n_params;
  for (int e = tid; e < sn.w_floats + sn.a_floats + sn.d_floats; e += kThreads) smem[e] = 0.f;
  __syncthreads();
  for (int p = tid; p < P; p += kThreads) Ws[param_slot(sn, p)] = init[p];
  for (int e = tid; e < L * kRows; e += kThreads) {   // the constant 1 behind every layer's inputs
    const int l = e / kRows, r = e - l * kRows;
    As[sn.a_off[l] + r * sn.a_stride[l] + sn.width[l]] = 1.f;
  }

  // this thread's tiles of dW
  int t_w[kSlots], t_a[kSlots], t_d[kSlots], t_S[kSlots], t_ds[kSlots];
  bool t_on[kSlots];
#pragma unroll
  for (int k = 0; k < kSlots; ++k) {
    const int gid = tid + k * kThreads;
    t_on[k] = gid < sn.n_tiles;
    int l = 0;
    while (l + 1 < L && gid >= sn.tile_off[l + 1]) ++l;
    const int t = t_on[k] ? gid - sn.tile_off[l] : 0;
    const int S = sn.a_stride[l], n_it = S >> 2, ot = t / n_it, it = t - ot * n_it;
    t_S[k] = S;
    t_ds[k] = sn.d_stride[l + 1];
    t_w[k] = sn.w_off[l] + ot * 4 * S + it * 4;
    t_a[k] = sn.a_off[l] + it * 4;
    t_d[k] = sn.d_off[l + 1] + ot * 4;
  }
  float g[kSlots][16], am[kSlots][16], av[kSlots][16];
#pragma unroll
  for (int k = 0; k < kSlots; ++k)
#pragma unroll
    for (int q = 0; q < 16; ++q) am[k][q] = av[k][q] = 0.f;
  __syncthreads();

  const int* __restrict__ ord_f = order + (int64_t)f * epochs * order_ld;
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
  const int un = tid & (kMaxWidth - 1), rg = tid >> 7;
  int step = 0;
  bool diverged = false;   // thread 0's
  for (int ep = 0; ep < epochs; ++ep) {
    const int* __restrict__ ord = ord_f + (int64_t)ep * order_ld;
    float eloss = 0.f;   // thread 0's
    for (int b0 = 0; b0 < n_train; b0 += batch, ++step) {
      const int B = min(batch, n_train - b0);
      float bsum = 0.f;   // thread 0's
#pragma unroll
      for (int k = 0; k < kSlots; ++k)
#pragma unroll
        for (int q = 0; q < 16; ++q) g[k][q] = 0.f;

      for (int r0 = 0; r0 < B; r0 += kRows) {
        const int nr = min(kRows, B - r0);
        load_rows(sn, As, zu, dim, n_pool, nr, tid, [&](int r) { return ord[b0 + r0 + r]; });
        if (tid < kRows)
          row_label[tid] = tid < nr ? (min(max(ord[b0 + r0 + tid], 0), n_pool - 1) >= n_first ? 1 : 0) : -1;
        __syncthreads();
        forward_tile(sn, Ws, As, tid);

        if (tid < kRows) {
          const float* __restrict__ lg = As + sn.a_off[L] + tid * sn.a_stride[L];
          float* __restrict__ dl = Ds + sn.d_off[L] + tid * sn.d_stride[L];
          const int y = row_label[tid];
          float ls = 0.f, d1 = 0.f;
          if (y >= 0) {
            const float d = lg[1] - lg[0], s = y ? -d : d;   // the wrong logit minus the right one
            ls = (s > 0.f ? s : 0.f) + log1pf(expf(-fabsf(s)));   // NaN for a NaN logit
            d1 = (sigmoidf(d) - (float)y) / (float)B;
          }
          row_loss[tid] = ls;
          dl[0] = -d1;
          dl[1] = d1;
        }
        __syncthreads();
        if (tid == 0)
          for (int r = 0; r < nr; ++r) bsum += row_loss[r];

        for (int l = L - 1; l >= 1; --l) {
          const int S = sn.a_stride[l], DS = sn.d_stride[l], DS1 = sn.d_stride[l + 1], o4n = DS1 >> 2;
          if (un < sn.width[l]) {
            const float* __restrict__ w = Ws + sn.w_off[l] + un;
            const float4* __restrict__ d = reinterpret_cast<const float4*>(Ds + sn.d_off[l + 1] + rg * 4 * DS1);
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
            for (int o4 = 0; o4 < o4n; ++o4) {
              const float w0 = w[(o4 * 4 + 0) * S], w1 = w[(o4 * 4 + 1) * S], w2 = w[(o4 * 4 + 2) * S],
                          w3 = w[(o4 * 4 + 3) * S];
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const float4 dv = d[j * o4n + o4];
                acc[j] = fmaf(dv.x, w0, acc[j]);
                acc[j] = fmaf(dv.y, w1, acc[j]);
                acc[j] = fmaf(dv.z, w2, acc[j]);
                acc[j] = fmaf(dv.w, w3, acc[j]);
              }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int r = rg * 4 + j;
              Ds[sn.d_off[l] + r * DS + un] = As[sn.a_off[l] + r * S + un] > 0.f ? acc[j] : 0.f;
            }
          }
          __syncthreads();
        }

#pragma unroll
        for (int k = 0; k < kSlots; ++k) {
          if (t_on[k]) {
            const float* __restrict__ ap = As + t_a[k];
            const float* __restrict__ dp = Ds + t_d[k];
#pragma unroll 4
            for (int r = 0; r < kRows; ++r) {
              const float4 a4 = *reinterpret_cast<const float4*>(ap + r * t_S[k]);
              const float4 d4 = *reinterpret_cast<const float4*>(dp + r * t_ds[k]);
              const float dd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
              for (int a = 0; a < 4; ++a) {
                g[k][a * 4 + 0] = fmaf(dd[a], a4.x, g[k][a * 4 + 0]);
                g[k][a * 4 + 1] = fmaf(dd[a], a4.y, g[k][a * 4 + 1]);
                g[k][a * 4 + 2] = fmaf(dd[a], a4.z, g[k][a * 4 + 2]);
                g[k][a * 4 + 3] = fmaf(dd[a], a4.w, g[k][a * 4 + 3]);
              }
            }
          }
        }
        __syncthreads();   // the next tile overwrites the activations and errors
      }

      // Adam, as torch.optim.Adam: the step's two factors come from the caller's table
      const float lr_t = adam[2 * step], c2 = adam[2 * step + 1];
#pragma unroll
      for (int k = 0; k < kSlots; ++k) {
        if (t_on[k]) {
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            float4* __restrict__ wp = reinterpret_cast<float4*>(Ws + t_w[k] + a * t_S[k]);
            const float4 w4 = *wp;
            float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              const int q = a * 4 + b;
              const float gg = fmaf(weight_decay, wv[b], g[k][q]);
              am[k][q] = fmaf(beta1, am[k][q], omb1 * gg);
              av[k][q] = fmaf(beta2, av[k][q], omb2 * gg * gg);
              const float den = fmaf(sqrtf(av[k][q]), c2, eps);
              wv[b] = wv[b] - lr_t * (am[k][q] / den);
            }
            *wp = make_float4(wv[0], wv[1], wv[2], wv[3]);
          }
        }
      }
      if (tid == 0) eloss += (bsum / (float)B) * (float)B;
      __syncthreads();
    }
    if (tid == 0) {
      const float el = eloss / (float)n_train;
      loss[(u * n_folds + f) * epochs + ep] = el;
      diverged |= not_finite(el);
    }
  }

  // held-out points: every tile of the pool that has one
  int n_correct = 0;   // thread 0's
  for (int i0 = 0; i0 < n_pool; i0 += kRows) {
    const int nr = min(kRows, n_pool - i0);
    bool any = false;
    for (int r = 0; r < nr; ++r) any |= fold[i0 + r] == f;   // uniform
    if (!any) continue;
    load_rows(sn, As, zu, dim, n_pool, nr, tid, [&](int r) { return i0 + r; });
    __syncthreads();
    forward_tile(sn, Ws, As, tid);
    if (tid == 0) {
      for (int r = 0; r < nr; ++r) {
        const int i = i0 + r;
        if (fold[i] != f) continue;
        const float* __restrict__ lg = As + sn.a_off[L] + r * sn.a_stride[L];
        const bool pred = lg[1] > lg[0];
        n_correct += pred == (i >= n_first) ? 1 : 0;
        if (prob) prob[u * n_pool + i] = sigmoidf(lg[1] - lg[0]);
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    correct[u * n_folds + f] = n_correct;
    if (diverged) bad[u] = 2;
  }
  if (params_out) {
    float* __restrict__ po = params_out + (u * n_folds + f) * P;
    for (int p = tid; p < P; p += kThreads) po[p] = Ws[param_slot(sn, p)];
  }
}

int fail(int code, const std::string& msg) { return npfn::set_error(code, msg.c_str()); }

int roundup4(int v) { return (v + 3) & ~3; }

}  // namespace

extern "C" {

int npfn_c2st_fit(const float* z, int64_t n_obs, int32_t n_pool, int32_t n_first, int32_t dim, const int32_t* widths,
                  int32_t n_layers, const float* init, const uint8_t* fold, int32_t n_folds, const int32_t* order,
                  const int32_t* n_train, int32_t order_ld, int32_t epochs, int32_t batch, const float* adam,
                  float beta1, float beta2, float eps, float weight_decay, int32_t* correct, float* loss, float* prob,
                  float* params_out, int32_t* bad, void* stream) {
  if (n_obs < 0) return fail(NPFN_EINVAL, "c2st_fit: need n_obs >= 0");
  if (dim < 1 || dim > kMaxDim) return fail(NPFN_EINVAL, "c2st_fit: dim must lie in 1.." + std::to_string(kMaxDim));
  if (n_pool < 2 || n_pool > kMaxPool)
    return fail(NPFN_EINVAL, "c2st_fit: n_pool must lie in 2.." + std::to_string(kMaxPool));
  if (n_first < 1 || n_first > n_pool - 1) return fail(NPFN_EINVAL, "c2st_fit: n_first must lie in 1..n_pool - 1");
  if (n_layers < 1 || n_layers > kMaxLayers)
    return fail(NPFN_EINVAL, "c2st_fit: n_layers must lie in 1.." + std::to_string(kMaxLayers));
  if (n_folds < 2 || n_folds > kMaxFolds)
    return fail(NPFN_EINVAL, "c2st_fit: n_folds must lie in 2.." + std::to_string(kMaxFolds));
  if (epochs < 1) return fail(NPFN_EINVAL, "c2st_fit: need epochs >= 1");
  if (batch < 1 || batch > kMaxBatch)
    return fail(NPFN_EINVAL, "c2st_fit: batch must lie in 1.." + std::to_string(kMaxBatch));
  if (!z || !widths || !init || !fold || !order || !n_train || !adam || !correct || !loss || !bad)
    return fail(NPFN_EINVAL, "c2st_fit: null z, widths, init, fold, order, n_train, adam, correct, loss or bad");
  if (widths[0] != dim) return fail(NPFN_EINVAL, "c2st_fit: widths[0] must equal dim");
  if (widths[n_layers] != 2) return fail(NPFN_EINVAL, "c2st_fit: the last width must be 2 (the two logits)");
  Net net{};
  net.n_layers = n_layers;
  int64_t P = 0;
  for (int l = 0; l <= n_layers; ++l) {
    if (widths[l] < 1 || widths[l] > kMaxWidth)
      return fail(NPFN_EINVAL, "c2st_fit: every width must lie in 1.." + std::to_string(kMaxWidth));
    net.width[l] = widths[l];
    if (l < n_layers) {
      net.p_off[l] = (int)P;
      P += (int64_t)widths[l + 1] * (widths[l] + 1);
    }
  }
  if (P > kMaxParams)
    return fail(NPFN_EINVAL, "c2st_fit: the network has " + std::to_string(P) + " parameters, above the " +
                                 std::to_string(kMaxParams) + " that a workgroup holds");
  net.p_off[n_layers] = (int)P;
  net.n_params = (int)P;
  FoldSizes fs{};
  for (int f = 0; f < n_folds; ++f) {
    if (n_train[f] < 1 || n_train[f] > order_ld || n_train[f] > n_pool)
      return fail(NPFN_EINVAL, "c2st_fit: every n_train must lie in 1..min(order_ld, n_pool)");
    fs.n_train[f] = n_train[f];
  }
  for (int l = 0; l <= n_layers; ++l) {
    net.a_stride[l] = l < n_layers ? roundup4(widths[l] + 1) : 4;
    net.a_off[l] = net.a_floats;
    net.a_floats += kRows * net.a_stride[l];
    net.d_stride[l] = l >= 1 ? roundup4(widths[l]) : 0;
    net.d_off[l] = net.d_floats;
    net.d_floats += kRows * net.d_stride[l];
  }
  for (int l = 0; l < n_layers; ++l) {
    const int rows = roundup4(widths[l + 1]);
    net.w_off[l] = net.w_floats;
    net.w_floats += rows * net.a_stride[l];
    net.tile_off[l] = net.n_tiles;
    net.n_tiles += (rows / 4) * (net.a_stride[l] / 4);
  }
  net.tile_off[n_layers] = net.n_tiles;
  const size_t lds = (size_t)(net.w_floats + net.a_floats + net.d_floats) * sizeof(float);
  // both hold whenever P <= 16384 and every width <= 128 (padding adds at most 3 rows and 4 columns
  // per layer: <= 1232 tiles, <= 151 KiB); checked all the same, since the kernel rests on them
  if (net.n_tiles > kSlots * kThreads || lds + 1024 > kLdsLimit)
    return fail(NPFN_EINVAL, "c2st_fit: the padded network does not fit one workgroup");
  if (n_obs == 0) return NPFN_OK;
  if (n_obs * n_folds > (int64_t)1 << 40) return fail(NPFN_EINVAL, "c2st_fit: n_obs * n_folds is too large");

  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(correct, 0, (size_t)n_obs * n_folds * sizeof(int32_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(loss, 0, (size_t)n_obs * n_folds * epochs * sizeof(float), s);
  if (e == hipSuccess && prob) e = hipMemsetAsync(prob, 0, (size_t)n_obs * n_pool * sizeof(float), s);
  if (e == hipSuccess && params_out)
    e = hipMemsetAsync(params_out, 0, (size_t)n_obs * n_folds * (size_t)P * sizeof(float), s);
  if (e == hipSuccess) e = hipMemsetAsync(bad, 0, (size_t)n_obs * sizeof(int32_t), s);
  if (e != hipSuccess) return fail(NPFN_EHIP, std::string("c2st_fit: hipMemsetAsync: ") + hipGetErrorString(e));

  e = hipFuncSetAttribute((const void*)k_c2st_fit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsLimit - 1024));
  if (e != hipSuccess) return fail(NPFN_EHIP, std::string("c2st_fit: hipFuncSetAttribute: ") + hipGetErrorString(e));
  const int64_t obs_per_launch = ((int64_t)1 << 30) / n_folds;
  for (int64_t m0 = 0; m0 < n_obs; m0 += obs_per_launch) {
    const int64_t nb = n_obs - m0 < obs_per_launch ? n_obs - m0 : obs_per_launch;
    hipLaunchKernelGGL(k_c2st_fit, dim3((unsigned)(nb * n_folds)), dim3(kThreads), lds, s, z, (int)n_pool,
                       (int)n_first, (int)dim, net, init, fold, (int)n_folds, (const int*)order, fs, (int)order_ld,
                       (int)epochs, (int)batch, adam, beta1, beta2, eps, weight_decay, m0, (int*)correct, loss, prob,
                       params_out, (int*)bad);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(NPFN_EHIP, std::string("c2st_fit: k_c2st_fit launch: ") + hipGetErrorString(e));
  }
  return NPFN_OK;
}

}  // extern "C"
