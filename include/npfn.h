/*
 * npfn.h -- C-ABI of the MI355X NPE-PFN engine (libnpfn.so).
 *
 * Drop-in boundary: the reference reaches this arithmetic through the
 * tabpfn estimator object held by NPE_PFN_Core (npe_pfn/npe_pfn.py:48,69;
 * tabpfn==2.2.1, poetry.lock:4455-4464).  Each entry point below replaces one
 * call the reference makes on it; the Python host package
 * (npe-pfn_amd/npe_pfn/tabpfn.py) binds them with ctypes, and INTEGRATION.md
 * shows the binding a maintainer would add to the reference.
 *
 * Conventions
 *  - every function returns 0 on success, a negative NPFN_E* code on failure;
 *    npfn_last_error() returns the thread-local message of the last failure;
 *  - all float/int buffers are DEVICE pointers owned by the caller (e.g.
 *    torch tensors' data_ptr()), row-major, float32 unless stated;
 *  - `stream` is a hipStream_t (NULL = legacy default stream); work is
 *    stream-ordered and asynchronous unless stated;
 *  - one engine handle per (device, thread); concurrent use of a handle is
 *    undefined (the reference is single-threaded).
 */
#ifndef NPFN_H
#define NPFN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPFN_OK 0
#define NPFN_EINVAL (-1)   /* bad argument or shape */
#define NPFN_EHIP (-2)     /* HIP runtime error */
#define NPFN_ESTATE (-3)   /* call out of order (e.g. predict before fit) */
#define NPFN_ENOMEM (-4)   /* device allocation failed */

typedef struct npfn_engine npfn_engine; /* opaque */

typedef struct npfn_config {
  int32_t d_model;            /* 192  [ext: tabpfn v2 regressor emsize] */
  int32_t n_heads;            /* 6    (head_dim must be 32) */
  int32_t n_layers;           /* 12 */
  int32_t d_ff;               /* 768 */
  int32_t n_bars;             /* 5000 Riemann bars */
  int32_t features_per_group; /* 2 */
  int32_t max_groups;         /* rows of the positional-embedding table */
  int32_t n_estimators;       /* 8  (TabPFNRegressor(n_estimators=...)) */
  float softmax_temperature;  /* 0.9 (TabPFNRegressor(softmax_temperature=...)) */
  int32_t device;             /* HIP device ordinal */
  uint64_t random_state;      /* TabPFNRegressor(random_state=...): feature
                                 permutations and the Philox key of sampling */
} npfn_config;

/* Library identity. */
int npfn_version(void);
const char* npfn_last_error(void);

/* Number of float32 values in the weight blob for `cfg` (layout: named tensors
 * in the order of npe_pfn/weights.py::weight_names, each [out, in] row-major). */
size_t npfn_weights_size(const npfn_config* cfg);

/* Create / destroy an engine.  `weights` is a HOST pointer to the blob; it is
 * converted (bf16 for GEMM weights) and uploaded once.  Replaces
 * `TabPFNRegressor(**regressor_init_kwargs)` (npe_pfn.py:48, :69). */
int npfn_engine_create(const npfn_config* cfg, const float* weights, size_t n_weights,
                       npfn_engine** out);
int npfn_engine_destroy(npfn_engine* h);

/* Per-estimator preprocessing of the feature columns, applied from the next fit on.
 * mode 3 (the DEFAULT of a new engine): tabpfn's default preprocessing ensemble [ext:
 * tabpfn 2.2.1, reached from TabPFNRegressor(**regressor_init_kwargs), npe_pfn.py:48;
 * restated in oracle/preprocess_oracle.py, parity pinned to that restatement and to
 * sklearn / hashlib only]: estimators 0-3 quantile-uniform features appended to the
 * original ones plus a TruncatedSVD of both, estimators 4-7 Yeo-Johnson features, every
 * estimator a SHA-256 fingerprint feature, every second estimator of each pipeline a
 * Yeo-Johnson transform of the target.  Table caps (npfn_fit returns NPFN_EINVAL past
 * them, npfn_last_error() naming the cap; npe_pfn/limits.py checks the same in Python):
 * at most max_groups feature groups per estimator row (2 features each; the default table has
 * 640 rows: tabpfn's 500 features under the ensemble need 626) and 1024 tokens; rows of up to
 * 256 tokens run the fused row kernel, wider estimator groups the per-sublayer kernels with the
 * long-row feature attention (memory: a wide group's train forward holds ~4.2 KB of per-sublayer
 * workspace per token -- E * n * C * 4.2 KB, ~26 GB per estimator group at 10 000 rows x 627
 * tokens -- plus its K/V cache; tested on the GPU up to 1 000 context rows x 298 features and
 * 100 rows x 500 features; past the device's memory npfn_fit returns NPFN_ENOMEM naming the
 * failed allocation); the SVD on at most 1024 features (a one-block Jacobi up to 256,
 * the n x n dual up to 512 context rows, else rocSOLVER dsyevd); for the quantile pipelines
 * sklearn's n_quantiles (n/5, the classifier's n/10) <= its 10000-row subsample, the
 * subsample itself from at most 65536 rows.  Above
 * 10000 context rows the quantile fit uses sklearn's 10000-row subsample and the train
 * fingerprints are made distinct among the 10000 hash buckets within blocks of 10000 rows
 * (tabpfn itself refuses more than 10000 rows unless ignore_pretraining_limits=True).
 * For npfn_fit_classes mode 3 is the
 * classifier's ensemble (quantile-uniform + original + SVD on every estimator, with the
 * fingerprint; the class shuffle is always on).
 * mode 0: standardization only -- NOT tabpfn's default; kept for the reference-anchored
 * golden fixtures.  mode 1: sklearn QuantileTransformer (uniform, n_quantiles =
 * max(n/5, 2)) on even estimators (`PreprocessorConfig("quantile_uni")`).  mode 2: mode 1
 * plus the Yeo-Johnson power transform (sklearn PowerTransformer, lambda by maximum
 * likelihood) on odd estimators ("safepower"); the quantile caps as for mode 3.
 * Invalidates the fit. */
int npfn_set_preprocessing(npfn_engine* h, int32_t mode);

/* TabPFNRegressor / TabPFNClassifier(average_before_softmax=...) [ext: tabpfn 2.2.1, reached
 * through regressor_init_kwargs / classifier_init_kwargs, npe_pfn.py:45-48, 610]: 0 (default)
 * mixes the ensemble as the mean of the estimators' probabilities; 1 as softmax(mean_e log q_e)
 * -- the estimators' (border-translated) log probabilities averaged, then renormalized; for the
 * classifier the estimators' class logits averaged, then softmax.  Applies from the next
 * predict / predict_proba / AR call on; the fit is kept. */
int npfn_set_average_before_softmax(npfn_engine* h, int32_t enable);

/* Fit: X [n_ctx, n_features] (row stride ldx), y [n_ctx] (element stride ldy).
 * Computes target standardization, per-estimator preprocessing and the
 * train-side forward (item-attention K/V cache of every layer).
 * Errors: NPFN_EINVAL past a table cap (npfn_set_preprocessing); NPFN_ENOMEM when a workspace
 * does not fit; NPFN_EHIP for a HIP error, or when the wide-table SVD's rocSOLVER dsyevd reports
 * no convergence (its info flag is checked before its vectors are used; that path alone waits on
 * the stream).
 * Replaces `self._model.fit(joint[:, :F], joint[:, F])` (npe_pfn.py:140,215,502). */
int npfn_fit(npfn_engine* h, const float* X, int64_t ldx, const float* y, int64_t ldy,
             int64_t n_ctx, int32_t n_features, void* stream);

/* Predict: Xq [n_rows, n_features of the last fit] (row stride ldq) ->
 * logits [n_rows, n_bars] = log of the ensemble-mean bar probabilities.
 * Replaces `predict(X, output_type="full", quantiles=[])["logits"]`
 * (npe_pfn.py:143-145, 217-219, 505-507). */
int npfn_predict(npfn_engine* h, const float* Xq, int64_t ldq, int64_t n_rows, float* logits,
                 void* stream);

/* Classifier fit (TabPFNClassifier.fit, npe_pfn.py:661): X [n_ctx, n_features],
 * y [n_ctx] = label INDICES 0..n_classes-1 as float (the host label-encodes, as
 * sklearn's LabelEncoder does in tabpfn).  The engine must have been created
 * with a classifier weight blob (decoder width cfg.n_bars >= n_classes; the
 * v2 classifier has 10).  Per estimator the labels are permuted; the train-side
 * forward fills the item-attention K/V cache exactly as npfn_fit does. */
int npfn_fit_classes(npfn_engine* h, const float* X, int64_t ldx, const float* y, int64_t ldy,
                     int64_t n_ctx, int32_t n_features, int32_t n_classes, void* stream);

/* Classifier probabilities: probs [n_rows, n_classes] = estimator mean of
 * softmax(class logits / T), in label-index order.  Replaces
 * `self._classifier.predict_proba(theta[mask])` (npe_pfn.py:697). */
int npfn_predict_proba(npfn_engine* h, const float* Xq, int64_t ldq, int64_t n_rows, float* probs,
                       void* stream);

/* Borders [n_bars + 1] of the last fit's criterion (standardized borders *
 * y_std + y_mean): the `criterion` half of predict(...)["criterion"]. */
int npfn_get_borders(npfn_engine* h, float* borders, void* stream);

/* criterion.sample(logits) (npe_pfn.py:146, 220): inverse-CDF sample of each
 * row with u = Philox4x32-10(counter=(row, counter), key=seed).  A row with no finite logit
 * (no mass) draws NaN, as npfn_bar_stats answers such a row. */
int npfn_bar_sample(const float* logits, const float* borders, int64_t n_rows, int32_t n_bars,
                    uint64_t seed, uint64_t counter, float* out, void* stream);

/* criterion(logits, y) (npe_pfn.py:149, 226, 510): full-support bar NLL. */
int npfn_bar_nll(const float* logits, const float* borders, const float* y, int64_t n_rows,
                 int32_t n_bars, float* out, void* stream);

/* criterion.cdf(logits, y): the CDF of the full-support bar distribution, the integral of exactly
 * the density whose negative log npfn_bar_nll returns (half-normal tail bars included):
 * out[i] = F(y_i) under row i of logits [n_rows, n_bars].  With p = softmax(logits row), borders
 * b[0..n_bars], w_j = b[j+1] - b[j], HM = 0.6744897501960817 and j the bucket of y by the NLL's
 * rule (searchsorted(b, y, left) - 1, the two end-border fix-ups, clamped to [0, n_bars-1]):
 *   F = sum_{i<j} p_i + p_j frac,
 *  - inner bars: frac = clamp((y - b[j]) / w_j, 0, 1);
 *  - left tail bar (j = 0), a half-normal hanging left from b[1] with scale s0 = w_0 / HM:
 *    frac = erfc(max(b[1] - y, 0) / (s0 sqrt 2)), so F(b[0]) = p_0 / 2 and F(-inf) = 0;
 *  - right tail bar (j = n_bars-1), s1 = w_last / HM: frac = erf(max(y - b[n_bars-1], 0) / (s1 sqrt 2));
 *  - w_j == 0: frac = 1.
 * The mass left and right of bar j are both summed (fp32 block sums) and the result is formed in
 * fp64 from the smaller side -- (S_left + p_j frac) / total if S_left <= S_right, else
 * 1 - (S_right + p_j (1 - frac)) / total with 1 - frac from the complementary error function in
 * the tails -- so the upper tail keeps its relative precision (as npfn_bar_stats' high quantiles).
 * y = NaN or a row without a finite logit gives NaN; y = -inf gives 0, y = +inf gives 1.
 * Note: tabpfn's sampler interpolates LINEARLY inside the two tail bars while its density there is
 * half-normal; npfn_bar_sample and the icdf of npfn_bar_stats keep that, so icdf(cdf(y)) == y
 * holds on the inner bars only.
 * Asynchronous; n_rows == 0 launches nothing.
 * Errors: NPFN_EINVAL for n_bars < 2, n_rows < 0 or a missing pointer. */
int npfn_bar_cdf(const float* logits, const float* borders, const float* y, int64_t n_rows, int32_t n_bars,
                 float* out, void* stream);

/* criterion.mean(logits), .median(logits), .mode(logits) and .icdf(logits, q) [ext: tabpfn 2.2.1
 * FullSupportBarDistribution] of each row of logits [n_rows, n_bars] in one pass.  With borders
 * b[0..n_bars], widths w_j = b[j+1] - b[j], p = softmax(logits row), HM = the half-normal median
 * 0.6744897501960817:
 *  - mean_out [n_rows] = sum_j p_j m_j, m_j = b[j] + w_j / 2 for the inner bars and the
 *    half-normal means m_0 = b[1] - (w_0 / HM) sqrt(2 / pi), m_last = b[n_bars-1] +
 *    (w_last / HM) sqrt(2 / pi) for the two tail bars (the scales of the NLL); summed in fp64;
 *  - quant_out [n_q][n_rows] (quantile i contiguous) = icdf(quantiles[i]): the arithmetic of
 *    npfn_bar_sample with u = q -- the first bar with mass whose cumulative sum reaches q * total,
 *    linear interpolation inside it (tail bars included) with the fraction clamped to [0, 1], the
 *    last bar with mass if q lies beyond the rounded total; above q = 1 - 2^-8, where fp32 sums
 *    from the left no longer resolve the tail, the same search on the complement summed from the
 *    right (the first bar with mass that leaves at most 1 - q to its right); q = 0 / 1 give the
 *    left / right border of the first / last bar with mass, never a point inside a zero-mass
 *    bar; q outside [0, 1] is clamped; the median is q = 0.5;
 *  - mode_out [n_rows] = the centre b[j] + w_j / 2 of the bar with the largest p_j / w_j (the
 *    lowest j on ties, tail bars with the plain centre, bars with w_j == 0 skipped).
 * quantiles is a DEVICE array of n_q <= 64 levels.  Any output may be NULL (that statistic is
 * skipped); n_q == 0 allows quantiles and quant_out to be NULL.  A row without a finite logit
 * gives NaN.  Asynchronous; n_rows == 0 launches nothing.
 * Errors: NPFN_EINVAL for n_bars < 2, n_q < 0, n_q > 64 or a missing pointer. */
int npfn_bar_stats(const float* logits, const float* borders, int64_t n_rows, int32_t n_bars,
                   const float* quantiles, int32_t n_q, float* mean_out, float* mode_out,
                   float* quant_out, void* stream);

/* predict(X, output_type="mean" | "median" | "mode" | "quantiles" | "main", quantiles=...) [ext:
 * tabpfn 2.2.1 TabPFNRegressor.predict]: npfn_predict's forward and ensemble mix, then the
 * summaries of npfn_bar_stats on the last fit's borders -- 8192 query rows at a time through an
 * engine-owned window of mixture logits (164 MB at 5000 bars);
 * the [n_rows, n_bars] fp32 logits of npfn_predict are never allocated.
 * Outputs, NULL outputs, the quantile list and n_q as for npfn_bar_stats.  Asynchronous;
 * honours npfn_set_average_before_softmax.
 * Errors: NPFN_EINVAL as for npfn_bar_stats and for ldq < n_features; NPFN_ESTATE before a fit,
 * after a classifier fit, or on a partial estimator range. */
int npfn_predict_stats(npfn_engine* h, const float* Xq, int64_t ldq, int64_t n_rows,
                       const float* quantiles, int32_t n_q, float* mean_out, float* mode_out,
                       float* quant_out, void* stream);

/* Fused autoregressive sampler: the whole `for param_idx in range(dim_theta)`
 * loop of NPE_PFN_Core._sample / _sample_batched (npe_pfn.py:135-169,
 * 211-241) on the device.  x_ctx [n_ctx, dim_x], theta_ctx [n_ctx, dim_theta]
 * (context), x_query [n_rows, dim_x] (already repeated / interleaved).
 * Step k uses Philox counter `counter + k`; query row i draws its uniform at
 * Philox row `row_base + i`, so a batch split into shards (rows [a, b) with
 * row_base = a, e.g. one observation shard per GPU) draws exactly the numbers
 * of the unsplit batch.  Writes theta_out [n_rows,
 * dim_theta] and, if log_prob_out != NULL, the summed per-step log densities
 * with -inf replaced by log(eps) (npe_pfn.py:148-159). */
int npfn_ar_sample(npfn_engine* h, const float* x_ctx, const float* theta_ctx, int64_t n_ctx,
                   int32_t dim_x, int32_t dim_theta, const float* x_query, int64_t n_rows,
                   uint64_t counter, int64_t row_base, float* theta_out, float* log_prob_out,
                   float eps, void* stream);

/* npfn_ar_sample over repeated query rows: x_unique [n_unique, dim_x] holds the distinct rows
 * and query row i is x_unique[i / (n_rows / n_unique)] (n_unique divides n_rows) -- the
 * `x.repeat(batch, 1)` of one observation (npe_pfn.py:122, n_unique = 1) and the obs-major
 * `x.repeat_interleave(n, 0)` of sample_batched (npe_pfn.py:199).  AR step 0, whose features
 * are the query rows alone, runs the forward, decoder and ensemble mix once per distinct row;
 * every row then draws from its row's mixture with its own uniform.  Same results as
 * npfn_ar_sample on the repeated rows, bit for bit: the forward is batch-invariant (a row's
 * result does not depend on its slot in the row kernel's token tile). */
int npfn_ar_sample_repeated(npfn_engine* h, const float* x_ctx, const float* theta_ctx, int64_t n_ctx,
                            int32_t dim_x, int32_t dim_theta, const float* x_unique, int64_t n_unique,
                            int64_t n_rows, uint64_t counter, int64_t row_base, float* theta_out,
                            float* log_prob_out, float eps, void* stream);

/* npfn_ar_sample_repeated that also returns the posterior marginals averaged over the sampler's
 * own conditionals ("Rao-Blackwellised" marginals).  Same arguments, fits, fit reuse
 * (npfn_set_fit_token), side-stream prefit, chunking (npfn_set_chunk_rows) and step 0 once per
 * distinct row; theta_out / log_prob_out (either may be NULL) are bit for bit those of
 * npfn_ar_sample_repeated.  With per = n_rows / n_unique and p_i the ensemble mixture row i
 * draws theta_k from at step k (given x and the row's own theta_<k):
 *  - marg_out [n_unique, dim_theta, n_bars]: [u, k, b] = (1 / per) * sum over the per rows i of
 *    observation u of p_i[b] / sum_b p_i[b] -- the estimate of the marginal bar masses of
 *    q(theta_k | x_u) that integrates each conditional instead of sampling it.  Every [u, k]
 *    row sums to 1 (to fp32 rounding).  At step 0 all rows of an observation share one mixture,
 *    so [u, 0] is that mixture normalised, with no averaging;
 *  - borders_out [dim_theta, n_bars + 1]: [k] = step k's bar borders, what npfn_get_borders
 *    returns after that step's fit, bit for bit.  All rows of a step share them, which is why
 *    the average over draws is a plain column sum with no re-binning.
 * Row k of marg_out with row k of borders_out is a bar distribution like any other:
 * npfn_bar_stats / npfn_bar_cdf / npfn_bar_nll on log(marg_out[u, k]) summarise it.
 * Reduction: per row 1 / sum_b p in fp64; rows added in row order in fp64 within strips of 64
 * consecutive rows of an observation, the strips added in order, one division by per, one
 * rounding to fp32.  No atomics; the summation order does not depend on the chunking, so the
 * result is bitwise reproducible and independent of npfn_set_chunk_rows, and an observation's
 * marginals do not depend on which other observations share the call (given the same row_base
 * for its rows).  A row whose mixture has no mass makes its observation's marginal NaN.
 * Device memory: a [min(chunk rows, n_rows), n_bars] fp32 window (328 MB at 16384 x 5000) and
 * [n_unique * ceil(per / 64), n_bars] fp64 partials.  Asynchronous.
 * Errors: NPFN_EINVAL for n_unique < 1, n_rows < n_unique, n_unique not dividing n_rows, NULL
 * marg_out or borders_out (these four are checked first, on the host, before the engine is
 * touched), and whatever npfn_ar_sample_repeated rejects; NPFN_ESTATE on a partial estimator
 * range. */
int npfn_ar_marginals(npfn_engine* h, const float* x_ctx, const float* theta_ctx, int64_t n_ctx,
                      int32_t dim_x, int32_t dim_theta, const float* x_unique, int64_t n_unique,
                      int64_t n_rows, uint64_t counter, int64_t row_base, float* theta_out,
                      float* log_prob_out, float eps, float* marg_out, float* borders_out, void* stream);

/* npfn_ar_sample_repeated that also returns the 2-D posterior marginals of every pair of
 * parameters on a grid of n_cells x n_cells cells ("half Rao-Blackwellised": the earlier
 * coordinate of a pair is the draw's cell, the later one is integrated out of the row's
 * conditional instead of being sampled).  Arguments, fits, fit reuse, side-stream prefit, chunking
 * and step 0 once per distinct row as npfn_ar_marginals up to eps; theta_out / log_prob_out (either
 * may be NULL) are bit for bit those of npfn_ar_sample_repeated.  With G = n_cells, per = n_rows /
 * n_unique, edges [dim_theta, G + 1] (DEVICE, row k strictly increasing: the cell borders of
 * parameter k; not checked here) and w_i[k][c] = npfn_bar_cell_mass of the mixture row i draws
 * theta_k from, on step k's borders and edges[k]:
 *  - cell_out [n_unique, dim_theta, G]: [u, k, c] = (1 / per) * sum over the rows i of
 *    observation u of w_i[k][c] -- the 1-D marginal's cell masses (at step 0 the distinct row's
 *    own cell masses);
 *  - pair_out [n_unique, n_pairs, G, G], n_pairs = dim_theta (dim_theta - 1) / 2, pair (j, k),
 *    j < k, at index k (k - 1) / 2 + j: [u, (j, k), a, c] = (1 / per) * sum over the rows i of
 *    observation u whose draw theta_j lies in cell a of edges[j] (edges[j][a] <= theta_j <
 *    edges[j][a + 1]) of w_i[k][c].  Mass outside the limits of either parameter is left out, so
 *    a table sums to the share of the joint inside its limits.  May be NULL when dim_theta == 1.
 * Route: every window of rows goes k_mix_prob -> window -> k_group_sample(per = 1) as in
 * npfn_ar_marginals, then npfn_bar_cell_mass and npfn_pair_accumulate on the window; each step's
 * sums are divided by 2^40 per and rounded to fp32 once.  The sums are integers, so the result
 * is bitwise reproducible and independent of npfn_set_chunk_rows, and an observation's tables do
 * not depend on which other observations share the call (given the same row_base for its rows).
 * An observation with a row whose mixture has no mass gets NaN tables for that step.
 * Device memory owned by the engine: npfn_ar_marginals' fp32 window, a [max(chunk rows,
 * n_unique), G] fp64 window of cell masses and [n_unique, (dim_theta - 1) G G + G] int64 sums,
 * zeroed by every call.  Asynchronous.
 * Errors, on the host before the engine is touched: NPFN_EINVAL for n_unique < 1, n_rows <
 * n_unique, n_unique not dividing n_rows, n_cells outside 2..128, per > 2^22 (the int64 headroom
 * of the 2^40-scaled sums), NULL edges or cell_out, NULL pair_out with dim_theta > 1; then
 * whatever npfn_ar_sample_repeated rejects; NPFN_ESTATE on a partial estimator range. */
int npfn_ar_pair_marginals(npfn_engine* h, const float* x_ctx, const float* theta_ctx, int64_t n_ctx,
                           int32_t dim_x, int32_t dim_theta, const float* x_unique, int64_t n_unique,
                           int64_t n_rows, uint64_t counter, int64_t row_base, float* theta_out,
                           float* log_prob_out, float eps, const float* edges, int32_t n_cells,
                           float* pair_out, float* cell_out, void* stream);

/* Teacher-forced autoregressive log density (npe_pfn.py:462-524):
 * log_prob_out [n_rows] = sum_k -NLL_k(theta[:, k] | x, theta[:, :k]). */
int npfn_ar_log_prob(npfn_engine* h, const float* x_ctx, const float* theta_ctx, int64_t n_ctx,
                     int32_t dim_x, int32_t dim_theta, const float* x_query, const float* theta,
                     int64_t n_rows, float* log_prob_out, float eps, void* stream);

/* npfn_ar_log_prob over repeated query rows (the `x.repeat(num_samples, 1)` of npe_pfn.py:480):
 * x_unique [n_unique, dim_x], query row i = x_unique[i / (n_rows / n_unique)]; step 0 runs once
 * per distinct row and every row's theta is scored under its row's mixture, which is the
 * repeated rows' own (the forward is batch-invariant). */
int npfn_ar_log_prob_repeated(npfn_engine* h, const float* x_ctx, const float* theta_ctx, int64_t n_ctx,
                              int32_t dim_x, int32_t dim_theta, const float* x_unique, int64_t n_unique,
                              const float* theta, int64_t n_rows, float* log_prob_out, float eps,
                              void* stream);

/* The teacher-forced pass of npfn_ar_log_prob / npfn_ar_log_prob_repeated with its per-step
 * results kept (NPE_PFN_Core.log_prob_batched / pit_batched; the reference declares
 * log_prob_batched and leaves it unimplemented, npe_pfn.py:457-460).  x_unique [n_unique, dim_x],
 * query row i = x_unique[i / (n_rows / n_unique)], n_unique dividing n_rows: n_unique == n_rows is
 * the plain case (npfn_ar_log_prob's path), otherwise step 0 runs its forward once per distinct
 * row (npfn_ar_log_prob_repeated's path).  theta [n_rows, dim_theta].
 *  - logp_steps [n_rows, dim_theta]: [i, k] = step k's log density of theta[i, k] given x and
 *    theta[i, :k], -inf replaced by log(eps) -- the same arithmetic on the same mixture as
 *    npfn_ar_log_prob, so summing the columns in order in fp32 gives its result bit for bit;
 *  - cdf_steps [n_rows, dim_theta]: [i, k] = npfn_bar_cdf's F(theta[i, k]) of that step's mixture
 *    on that step's borders -- the probability integral transform u_k = F_k(theta_k | x,
 *    theta_<k), uniform exactly when conditional k is calibrated.
 * Either output may be NULL (it is skipped), not both.  Fit reuse (npfn_set_fit_token), chunking
 * (npfn_set_chunk_rows) and npfn_set_average_before_softmax as for npfn_ar_log_prob.  Asynchronous.
 * Errors: NPFN_ESTATE on a partial estimator range; NPFN_EINVAL for bad dimensions, a missing
 * input, n_unique < 1 or not dividing n_rows, or both outputs NULL. */
int npfn_ar_score(npfn_engine* h, const float* x_ctx, const float* theta_ctx, int64_t n_ctx, int32_t dim_x,
                  int32_t dim_theta, const float* x_unique, int64_t n_unique, const float* theta, int64_t n_rows,
                  float* logp_steps, float* cdf_steps, float eps, void* stream);

/* K9: prior-support check of a box prior (npe_pfn.py:581-600 with
 * BoxUniform): mask[i] = all_j(low_j <= theta[i,j] <= high_j), 1 or 0.
 * The bounds are closed: theta == low_j and theta == high_j are inside, the next float past
 * either is outside; -0.0 equals +0.0.  Both comparisons are false for NaN, so a row with a
 * NaN cell, or a column with a NaN bound, is outside.  Infinite bounds are allowed (+-inf
 * cells are inside a bound of the same infinity); low_j > high_j accepts no row.
 * n_rows == 0 launches nothing (theta and mask may then be NULL).
 * Errors: NPFN_EINVAL for dim < 1, n_rows < 0 or a missing pointer with n_rows > 0. */
int npfn_box_support(const float* theta, int64_t n_rows, int32_t dim, const float* low,
                     const float* high, uint8_t* mask, void* stream);

/* K9/K10 stream compaction: rows of src [n_rows, dim] with mask != 0 are
 * written in order to dst; *count_out (device int64) receives the count.
 * Any non-zero mask byte selects its row (not only 1).  dst [n_rows, dim] is written in rows
 * [0, count) only: rows from count on keep what they held.  n_rows == 0 launches no kernel and
 * sets *count_out = 0 (src, mask and dst may then be NULL, as the pointers of empty arrays are).
 * Errors: NPFN_EINVAL for dim < 1, n_rows < 0, a missing count_out, or a missing src, mask or
 * dst with n_rows > 0. */
int npfn_compact_rows(const float* src, const uint8_t* mask, int64_t n_rows, int32_t dim,
                      float* dst, int64_t* count_out, void* stream);

/* Box proposals of the restricted prior's rejection sampler (NPE_PFN_RestrictedPrior, reference
 * restricted_prior.py:8-97; there prior.sample of a BoxUniform inside sbi's rejection loop):
 * with u = Philox4x32-10 uniform(key = seed, counter = counter + j, row = row_base + i) -- the
 * u of npfn_bar_sample, the 64-bit row's high word included -- and span_j = fl(high[j] - low[j]),
 *   out[i, j] = min(fl(low[j] + fl(u * span_j)), high[j]),
 * every operation rounded to fp32 on its own (no fused multiply-add), so a float32 restatement
 * is bit-exact (tests/restricted_ref.py).  The min keeps the point inside the closed box that
 * npfn_box_support accepts when span_j rounded up.  low, high [dim] and out [n_rows, dim] are
 * DEVICE arrays.  Rows [a, b) with row_base = a are rows a..b-1 of the unsplit call.
 * Asynchronous; n_rows == 0 launches nothing.
 * Errors: NPFN_EINVAL for dim < 1, n_rows < 0, row_base < 0, a missing pointer or more than
 * 2^39 - 256 values in one call. */
int npfn_box_propose(const float* low, const float* high, int32_t dim, int64_t n_rows, uint64_t seed,
                     uint64_t counter, int64_t row_base, float* out, void* stream);

/* The restricted prior's accept decision (reference restricted_prior.py:25-28,
 * `classifier.predict_proba(theta)[:, -1] > acceptance_threshold`): mask_out[i] (uint8, 0 / 1) =
 * p_i > threshold, strictly, with p_i the LAST class's probability of row i exactly as
 * npfn_predict_proba returns it -- the same forward, chunking (npfn_set_chunk_rows) and ensemble
 * mix (npfn_set_average_before_softmax honoured) into an engine-owned window of [chunk rows,
 * n_classes] probabilities, then one kernel over its last column; bit-equal to column
 * n_classes - 1 of npfn_predict_proba.  prob_out [n_rows] (may be NULL) receives p_i.
 * Asynchronous; n_rows == 0 launches nothing.
 * Errors: NPFN_ESTATE before npfn_fit_classes (or after a regressor fit) or on a partial
 * estimator range; NPFN_EINVAL for n_rows < 0, ldq < n_features or a missing Xq / mask_out. */
int npfn_predict_accept(npfn_engine* h, const float* Xq, int64_t ldq, int64_t n_rows, float threshold,
                        uint8_t* mask_out, float* prob_out, void* stream);

/* One rejection round of the restricted prior over a box (the body of sbi's rejection loop
 * around restricted_prior.py:25-28, without its two host round trips):
 *  1. npfn_box_propose(low, high, dim, n_rows, seed, counter, row_base) into engine scratch;
 *  2. npfn_predict_accept's decision on those rows at `threshold` (dim must be the classifier
 *     fit's feature count);
 *  3. the accepted rows, in row order, are appended to theta_out [capacity, dim] from row
 *     counts[0] on; accepted rows that would land at or past `capacity` are dropped;
 *  4. counts[0] = min(capacity, counts[0] + accepted); counts[1] += accepted.
 * counts is a DEVICE int64[2] = {rows stored in theta_out, rows accepted in total}, set to 0 by
 * the caller before the first round and read by it when it wants to (0 <= counts[0] <= capacity
 * is the caller's promise).  Rounds with row_base = the rows proposed so far make theta_out the
 * first `capacity` accepted rows of the Philox row stream, whatever the sizes of the rounds (the
 * forward is batch-invariant).  The append is one workgroup taking 1024 rows per pass in order:
 * deterministic, no floating-point atomics, no workgroup waiting on another.
 * n_rows == 0 launches nothing; counts[0] == capacity leaves theta_out untouched (the round
 * still counts its accepted rows into counts[1]).  Asynchronous; the scratch for proposals,
 * flags and probabilities is engine-owned and grows on demand (growing waits on the stream).
 * Errors: NPFN_ESTATE as for npfn_predict_accept; NPFN_EINVAL for dim != n_features, n_rows < 0,
 * capacity < 0, row_base < 0, a missing low / high / counts, or a missing theta_out with
 * capacity > 0; NPFN_ENOMEM when the scratch does not fit. */
int npfn_restricted_box_round(npfn_engine* h, const float* low, const float* high, int32_t dim, float threshold,
                              int64_t n_rows, uint64_t seed, uint64_t counter, int64_t row_base, float* theta_out,
                              int64_t capacity, int64_t* counts, void* stream);

/* Coverage ranks (NPE_PFN_Core.coverage_batched): folds one sampler round into per-observation
 * integer counts, so that simulation-based-calibration, HPD and TARP ranks need no stored draws.
 * theta [n_obs * per, dim] is obs-major (row i belongs to observation i / per: the layout of
 * npfn_ar_sample_repeated's theta_out), logp [n_obs * per] the rows' log densities, take
 * [n_obs * per] (may be NULL: every row) selects the rows that take part (take[i] != 0);
 * theta_true [n_obs, dim], logp_true [n_obs], ref [n_obs, dim], inv_scale [dim].
 * counts [n_obs, dim + 2, 2] int64 is ADDED to (the caller zeroes it before the first round);
 * for observation m and each of its rows s that takes part, slot 0 counts "<" and slot 1 "==":
 *  - column k < dim:  theta[s, k] < theta_true[m, k]   /  theta[s, k] == theta_true[m, k];
 *  - column dim (HPD):  logp[s] > logp_true[m]          /  logp[s] == logp_true[m];
 *  - column dim + 1 (TARP):  d2(theta[s]) < d2(theta_true[m])  /  ==, where
 *    d2(a) = sum over k ascending of t_k * t_k, t_k = ((double)a_k - (double)ref[m, k]) *
 *    (double)inv_scale[k], in fp64 with every multiply and add rounded on its own (no fused
 *    multiply-add), so a host restatement gives the same bits
 *    (npe_pfn.diagnostics.rank_accumulate_host).
 * The comparisons are IEEE: a NaN on either side counts in neither slot.  logp / logp_true may
 * both be NULL (the HPD column is left untouched), ref / inv_scale may both be NULL (the TARP
 * column is left untouched).  Every observation is cut into strips of 256 rows, one workgroup
 * each; a workgroup stages its rows through LDS (the table is read once, coalesced), counts per
 * wave with a ballot, sums its waves in LDS and issues one 64-bit integer add per non-zero
 * counter.  Integer sums do not depend on the order of arrival: the result is bitwise
 * reproducible.  Any dim >= 1.  Asynchronous; n_obs * per == 0 launches nothing.
 * Errors: NPFN_EINVAL (message starting "rank_accumulate") for n_obs < 0, per < 0, dim < 1, half
 * of a nullable pair, or a missing theta / theta_true / counts -- all on the host before any
 * launch. */
int npfn_rank_accumulate(const float* theta, const float* logp, const uint8_t* take, int64_t n_obs, int64_t per,
                         int32_t dim, const float* theta_true, const float* logp_true, const float* ref,
                         const float* inv_scale, int64_t* counts, void* stream);

/* Cell masses of bar distributions on a coarse grid (the row kernel of npfn_ar_pair_marginals;
 * needs no engine).  probs [n_rows, n_bars]: UNNORMALISED fp32 bar masses (a k_mix_prob row, or
 * exp of logits); borders [n_bars + 1], shared by all rows; edges [n_cells + 1] fp32, strictly
 * increasing (not checked).  w_out [n_rows, n_cells] in FP64: with tot = sum_b p[b] and L(j) =
 * sum_{b<j} p[b] (both fp64; per thread in bar order, then an LDS block scan in a fixed order),
 *   F(e) = (L(j) + p[j] * frac) / tot,   w[c] = max(F(edges[c + 1]) - F(edges[c]), 0),
 * j = the bucket of e by npfn_bar_nll's rule and frac the share of bar j left of e by
 * npfn_bar_cdf's rules: linear in an inner bar, erfc / erf of the half-normal tails in the two
 * end bars, 1 in a bar of width 0.  F is always formed from the left (the sums are fp64).  A
 * row whose tot is not a positive finite number gets NaN in its whole w row.  One 256-thread
 * workgroup per row.  Asynchronous.
 * Errors (host, before any launch): NPFN_EINVAL (message starting "bar_cell_mass") for n_rows <
 * 0 or >= 2^31, n_bars < 2 or beyond what a workgroup's LDS holds (15 000), n_cells outside
 * 2..128, or a NULL pointer. */
int npfn_bar_cell_mass(const float* probs, const float* borders, int64_t n_rows, int32_t n_bars,
                       const float* edges, int32_t n_cells, double* w_out, void* stream);

/* Folds one window of cell masses into the integer sums behind npfn_ar_pair_marginals (needs no
 * engine).  With G = n_cells: w [n_rows, G] fp64 (npfn_bar_cell_mass), theta [n_rows, ldt] whose
 * first n_prev columns are the rows' earlier draws, edges [n_prev, G + 1] (row j strictly
 * increasing); window row r is row r0 + r of the call and belongs to observation u = (r0 + r) /
 * per.  Every w is quantised once, q = llrint(w * 2^40) (round half to even), and for row r:
 *  - cellQ [U, G]: cellQ[u][c] += q[c] for every c;
 *  - pairQ [U, n_prev, G, G]: for every j < n_prev whose draw has a cell a (edges[j][a] <=
 *    theta[r][j] < edges[j][a + 1]): pairQ[u][j][a][c] += q[c] for every c.  A draw below
 *    edges[j][0], at or above edges[j][G], or NaN has no cell;
 *  - a row with a NaN in w sets bad[u] = 1 (bad [U] int32) and adds nothing.
 * Both tables are ADDED to (int64; the caller zeroes them and bad before the first window).
 * npe_pfn.pair_marginals.pair_accumulate_host is the same statement in torch; the two are equal
 * exactly.  Kernel: one workgroup per (strip of 256 consecutive rows of an observation, j, slab
 * of at most 4096 / G values of a); it finds the rows' cells by binary search, adds into an
 * int64 LDS table with 64-bit LDS integer adds and issues one 64-bit global integer add per
 * non-zero cell.  Integer sums do not depend on the order of arrival: the result is bitwise
 * reproducible whatever the windows, the launch geometry or the other observations of the call.
 * n_prev = 0 (theta, edges and pairQ may be NULL) adds to cellQ only.  Asynchronous.
 * Errors (host, before any launch): NPFN_EINVAL (message starting "pair_accumulate") for r0 < 0,
 * n_rows < 0, per < 1, per > 2^22 (the int64 headroom: 2^22 rows x 2^40 < 2^63), n_prev < 0 or
 * > ldt, n_cells outside 2..128, or a missing pointer. */
int npfn_pair_accumulate(const double* w, const float* theta, int64_t ldt, int32_t n_prev, const float* edges,
                         int32_t n_cells, int64_t r0, int64_t n_rows, int64_t per, int64_t* pairQ,
                         int64_t* cellQ, int32_t* bad, void* stream);

/* MMD two-sample sums (npe_pfn.diagnostics.mmd_batched; the reference's MMD, scripts/
 * evaluate_ropefm.py:283-320, with a permutation null; needs no engine).  z [n_obs, N = n_pool,
 * dim] (device): observation u's pooled sample, both sets stacked.  bandwidths [n_bw] is a HOST
 * array of the a_b (the one host pointer among this header's device pointers; read before the
 * call returns).  labels [n_label, N] uint8 (device), shared by all observations: row p marks
 * (non-zero) the points of group X under labelling p -- row 0 the observed split, the others
 * permutations of it.  Outputs (device), ZEROED BY THE CALL itself on `stream`: sums [n_obs,
 * n_label, 2] int64, total [n_obs] int64, bad [n_obs] int32.
 *  - d2(i, j), fp32: acc = 0; for k ascending t = fl(z_i[k] - z_j[k]), acc = fl(acc + fl(t * t)),
 *    every operation rounded on its own (no fused multiply-add, as in npfn_box_propose), so d2 is
 *    bitwise symmetric and d2(i, i) = 0;
 *  - kernel = 0 (rbf, the reference's exp(-0.5 d2 / a)): c_b = fl(-0.5f / a_b) on the host, k_b =
 *    expf(fl(d2 * c_b)) with the accurate expf;
 *  - kernel = 1 (multiscale, the reference's a^2 / (a^2 + d2)): s_b = fl(a_b * a_b) on the host,
 *    k_b = fl(s_b / fl(s_b + d2)), the division correctly rounded;
 *  - q(i, j) = sum over b of llrint((double)k_b * 2^28) (round half to even); k_b <= 1 and n_bw <=
 *    8, so q <= 2^31 and q(i, i) = n_bw * 2^28 exactly;
 *  - over ORDERED pairs, the diagonal included: sums[u][p][0] = sum of q(i, j) over the i, j with
 *    labels[p][i] and labels[p][j] both set, sums[u][p][1] the same with both clear, total[u] the
 *    sum over all N^2 pairs (the cross sum of a labelling is total - sums[0] - sums[1]).
 * Fixed point makes the sums integers: they do not depend on the order of arrival, so the result
 * is bitwise reproducible whatever the launch geometry or the other observations of the call, and
 * multiscale equals the torch restatement npe_pfn.diagnostics.mmd_sums_host exactly (rbf to
 * expf's last bit: 2^-23 of k_b, 32 units, per pair and bandwidth).  An observation with a
 * non-finite coordinate gets bad[u] = 1; its sums are then unspecified.
 * Kernel: one workgroup per (tile I of 64 points, strip of 8 tiles J >= I, observation, slab of 256
 * labellings).  Both tiles' coordinates are staged in LDS, every q of the tile pair is computed
 * once into an LDS tile cut into byte planes, and thread t folds it into labelling slab * 256 + t:
 * its labels are two 64-bit masks built with a ballot, the bytes of q are read by LDS broadcast
 * and summed per plane with v_dot4_u32_u8 (exact in 32 bits), the planes recombined in int64.  An
 * off-diagonal tile pair counts twice.  One 64-bit integer add per workgroup and non-zero
 * counter.  Neither an N x N nor an N x n_label array reaches global memory.  Asynchronous;
 * n_obs == 0 launches nothing.
 * Errors (host, before any launch): NPFN_EINVAL (message starting "mmd_sums") for n_obs < 0,
 * n_pool outside 1..32768 (N^2 * 2^31 <= 2^61 keeps the int64 sums exact), dim outside 1..64,
 * kernel not 0 or 1, n_bw outside 1..8, a bandwidth that is not finite and > 0, n_label outside
 * 1..4096, or a missing pointer. */
int npfn_mmd_sums(const float* z, int64_t n_obs, int64_t n_pool, int32_t dim, int32_t kernel,
                  const float* bandwidths, int32_t n_bw, const uint8_t* labels, int32_t n_label,
                  int64_t* sums, int64_t* total, int32_t* bad, void* stream);

/* Exact 2-Wasserstein assignment (npe_pfn.diagnostics.wasserstein_batched; the reference's
 * sqrt(ot.emd2(uniform, uniform, ot.dist(a, b))), scripts/evaluate_ropefm.py:592-710; needs no
 * engine).  a, b [n_obs, n, dim] (device): per observation two sets of n points with weight 1 / n
 * each, for which optimal transport under the squared-Euclidean cost is a linear assignment
 * problem.  scale [n_obs] double (device): the caller's power of two per observation
 * (npe_pfn.diagnostics.transport_scale) with d2 * scale <= 2^41.  Outputs (device), ZEROED BY THE
 * CALL itself on `stream`: assign [n_obs, n] int32, duals [n_obs, 2, n] int64 (may be NULL),
 * cost_sum [n_obs] int64, steps [n_obs] int64 (may be NULL), bad [n_obs] int32.
 *  - d2(i, j), fp32, as in npfn_mmd_sums: acc = 0; for k ascending t = fl(a_i[k] - b_j[k]), acc =
 *    fl(acc + fl(t * t)), every operation rounded on its own;
 *  - cq(i, j) = llrint((double)d2 * scale) (round half to even), an integer in 0..2^41;
 *  - the shortest-augmenting-path Hungarian method from zero duals, all in int64: rows i = 0..n-1
 *    are inserted in order; for row i, minv[j] = INF, used[j] = false and a virtual column holds
 *    row i; a step marks the current column j0 used, takes its row i0, sets for every unused j cur
 *    = cq[i0][j] - u[i0] - v[j] and, where cur < minv[j] (strictly), minv[j] = cur, way[j] = j0;
 *    delta = the minimum of minv over the unused columns, j1 its LOWEST column; u[row of j] +=
 *    delta and v[j] -= delta over the used columns (the virtual one's row i included), minv[j] -=
 *    delta over the unused; j0 = j1, until j0 has no row; then the path is flipped along way;
 *  - assign[u][i] = the column of b matched to row i of a, duals[u][0] = u, duals[u][1] = v,
 *    cost_sum[u] = sum over i of cq(i, assign[i]) (= sum(u) + sum(v)), steps[u] = the number of
 *    steps, at most n (n + 1) / 2.
 * All four equal npe_pfn.diagnostics.assignment_solve_host on transport_costs_host's cq bit for
 * bit, whatever the other observations of the call.  With n <= 2048 every potential and sum stays
 * below 2^53.  bad[u] = 1 for a non-finite coordinate, 2 for a cost above 2^41 (the scale broke
 * its promise), 3 for a step counter past n (n + 1) / 2; the observation's other outputs are then
 * unspecified.
 * Kernel: one workgroup per observation, of the smallest power of two of threads in 64..1024 that
 * is >= n / 2; a thread owns columns j and j + blockDim with their v, minv, way and used flag in
 * registers; u and the column -> row map are in LDS, as is b transposed (and a when both fit in
 * 159 KiB; otherwise the one row of a is read from global memory); each step recomputes its cost
 * row, reduces (value, lowest index) with DPP / permlane inside the wave and one LDS hop across
 * waves, and has one barrier.  No n x n array reaches global memory; no workgroup waits on
 * another.  Asynchronous; n_obs == 0 launches nothing.
 * Errors (host, before any launch): NPFN_EINVAL (message starting "w2_assign") for n_obs < 0, n
 * outside 1..2048, dim outside 1..64, n * dim > 32768 (b's LDS image), or a missing a, b, scale,
 * assign, cost_sum or bad. */
int npfn_w2_assign(const float* a, const float* b, int64_t n_obs, int32_t n, int32_t dim,
                   const double* scale, int32_t* assign, int64_t* duals, int64_t* cost_sum,
                   int64_t* steps, int32_t* bad, void* stream);

/* Classifier two-sample test (npe_pfn.diagnostics.c2st_batched; the reference's
 * classifier_two_samples_test_torch, scripts/evaluate_ropefm.py:119-280; needs no engine): per
 * (observation, fold) a small ReLU MLP is trained with Adam on the pooled points outside the fold
 * and scored on the points inside it, all in one launch.  z [n_obs, n_pool, dim] (device): per
 * observation the pooled sample; points 0..n_first-1 have label 0, the others label 1.  widths
 * (HOST) [n_layers + 1]: widths[0] = dim, widths[n_layers] = 2; layer l is a Linear of widths[l]
 * inputs and widths[l + 1] units, a ReLU behind every layer but the last.  init [P] (device): the
 * starting parameters of every (observation, fold), layer by layer W [out, in] row-major then b
 * [out]; P = sum of widths[l + 1] * (widths[l] + 1).  fold [n_pool] uint8 (device): the fold that
 * holds each point out.  order [n_folds, epochs, order_ld] int32 (device): row (f, e) lists, in its
 * first n_train[f] entries (n_train HOST [n_folds]), the pooled indices that fold f trains on in
 * epoch e, in visiting order (indices are clamped to 0..n_pool-1); batch j of an epoch is entries j
 * * batch .. min((j + 1) * batch, n_train[f]) - 1, a short last batch included.  adam [n_steps, 2]
 * float (device), n_steps >= epochs * ceil(max n_train / batch): for step t (0-based, counted over
 * the batches of all epochs) adam[t] = (lr / (1 - beta1^(t+1)), 1 / sqrt(1 - beta2^(t+1))).
 * Outputs (device), ZEROED BY THE CALL itself on `stream`: correct [n_obs, n_folds] int32, loss
 * [n_obs, n_folds, epochs], prob [n_obs, n_pool] (may be NULL), params_out [n_obs, n_folds, P] (may
 * be NULL), bad [n_obs] int32.  Everything in fp32, sums as chains of fmaf:
 *  - forward, per row: h_0 = the point; unit o of layer l = sum over i ascending of W[o][i] h_l[i],
 *    then + b[o]; h_{l+1} = the unit where it is >= 0, else 0; the last layer's two units are the
 *    logits (l0, l1), d = l1 - l0;
 *  - row loss = max(s, 0) + log1pf(expf(-|s|)), s = d for label 0 and -d for label 1 (cross-
 *    entropy); p1 = 1 / (1 + expf(-d)) (as e / (1 + e), e = expf(d), for d < 0); the error of logit
 *    1 is (p1 - label) / B and of logit 0 its negative, B the rows of the batch; the batch loss is
 *    (the row losses added in row order) / B, an epoch adds batch loss * B over its batches, and
 *    loss[u][f][e] = that / n_train[f] (the reference's epoch_loss / len(train_ds));
 *  - backward: the error of unit i of layer l = sum over o ascending of error_{l+1}[o] W_l[o][i]
 *    where h_l[i] > 0, else 0; dW[o][i] = sum over the batch's rows in order of error[o] h[i], db[o]
 *    likewise with h = 1;
 *  - Adam as torch.optim.Adam (no amsgrad): g = dW + weight_decay * w; m = beta1 m + (1 - beta1) g;
 *    v = beta2 v + (1 - beta2) g g; w -= adam[t][0] * (m / (sqrt(v) * adam[t][1] + eps)), 1 - beta
 *    formed in fp32 from the fp32 beta, sqrt and the division correctly rounded;
 *  - after the last epoch, for every point i with fold[i] == f: prob[u][i] = p1 of the fold's
 *    network, and correct[u][f] counts the points whose prediction (1 exactly when l1 > l0) equals
 *    their label.
 * bad[u] = 1 for a non-finite coordinate (nothing is trained), 2 when an epoch loss of some fold
 * is not finite; the observation's other outputs are then unspecified.  The result of an
 * (observation, fold) is bitwise the same from run to run and whatever other observations are in
 * the call: no atomics, every sum in the order above (npe_pfn.diagnostics.c2st_fit_host restates
 * it in torch, to rounding).
 * Kernel: one workgroup of 512 threads per (observation, fold).  Each layer's [W | b] sits in LDS
 * padded to a multiple of 4 rows and columns (padding entries are parameters that stay 0); a batch
 * is processed in tiles of 16 rows, whose activations and errors per layer are in LDS; the 4 x 4
 * tiles of all layers' padded [W | b] are dealt to the threads, at most 3 each, and a thread keeps
 * the gradient and both Adam moments of its 48 entries in registers for the whole training.  Batch
 * rows are read from global memory.  Asynchronous; n_obs == 0 launches nothing.
 * Caps: P <= 16384 and every width <= 128 -- "mlp" (dim, 4 dim, 8 dim, 8 dim, 4 dim, 2) up to dim
 * 11, "mlp_small" (dim, 4 dim, 4 dim, 2) up to dim 28, "linear" (dim, 2) up to dim 64.
 * Errors (host, before any launch): NPFN_EINVAL (message starting "c2st_fit") for n_obs < 0, dim
 * outside 1..64, n_pool outside 2..32768, n_first outside 1..n_pool-1, n_layers outside 1..5,
 * widths[0] != dim, a last width != 2, a width outside 1..128, P > 16384, n_folds outside 2..16,
 * epochs < 1, batch outside 1..4096, an n_train outside 1..min(order_ld, n_pool), or a missing z,
 * widths, init, fold, order, n_train, adam, correct, loss or bad. */
int npfn_c2st_fit(const float* z, int64_t n_obs, int32_t n_pool, int32_t n_first, int32_t dim,
                  const int32_t* widths, int32_t n_layers, const float* init, const uint8_t* fold,
                  int32_t n_folds, const int32_t* order, const int32_t* n_train, int32_t order_ld,
                  int32_t epochs, int32_t batch, const float* adam, float beta1, float beta2,
                  float eps, float weight_decay, int32_t* correct, float* loss, float* prob,
                  float* params_out, int32_t* bad, void* stream);

/* K12 standardized-Euclidean context filter (support_posterior.py:357-369):
 * idx_out[0:k] = indices of the k rows of x [n_rows, dim] closest to obs in
 * z-scored Euclidean distance, ascending (ties by lower index).
 * Column mean and unbiased std (n_rows - 1; n_rows itself for a single row) are fp64 sums of
 * the fp32 values rounded to fp32; the distance is fp32.  Rows are ordered by (distance, row):
 * equal distances keep their row order, and a NaN distance sorts after every number, again by
 * row.  A constant column (std 0) or a NaN cell in a column makes every distance NaN, so the
 * result is then rows 0 .. k-1.  k == 0 launches nothing (idx_out may then be NULL).
 * Errors: NPFN_EINVAL for dim < 1, n_rows < 1, n_rows > 2^32 - 1, k < 0, k > n_rows, a missing
 * x or obs, or a missing idx_out with k > 0; NPFN_ENOMEM when the sort keys (8 bytes per row,
 * rounded up to a power of two) do not fit. */
int npfn_filter_stdeuclid(const float* x, int64_t n_rows, int32_t dim, const float* obs, int64_t k,
                          int64_t* idx_out, void* stream);

/* K11 SIR resampling step of PosteriorSupport.sample_sir (support_posterior.py:
 * 216-241).  lpr, lq [n_groups * k]: prior / posterior log densities of the
 * proposals, group g = rows g*k .. g*k+k-1; thr: DEVICE float (the lq quantile).
 * Per group: log_ratio = nan_to_num(lpr - lq, nan=-inf) with lpr := -inf where
 * lq < *thr; ess_out[g] = 1 / sum softmax(log_ratio)^2; pick_out[g] = inverse-CDF
 * index of softmax(log_ratio) at u = Philox4x32-10(counter=(group_offset + g,
 * counter), key=seed).  If theta_out != NULL, theta_out[g, :] = theta[g*k + pick, :]
 * (theta [n_groups * k, dim]).
 * The truncation is strict: lq == *thr keeps its lpr.  A group whose ratios are all NaN has
 * ess NaN and pick 0.  group_offset only shifts the Philox row: a call on groups [a, b) of the
 * arrays with group_offset = a gives groups a .. b-1 of the unsplit call bit for bit.
 * n_groups == 0 launches nothing (every array may then be NULL).
 * Errors: NPFN_EINVAL for n_groups < 0, k < 1, group_offset < 0, more than 4 (2^31 - 1) groups, and with
 * n_groups > 0 a missing lpr, lq, thr, pick_out or ess_out, or theta_out without theta or with
 * dim < 1. */
int npfn_sir_select(const float* lpr, const float* lq, const float* thr, int64_t n_groups, int32_t k,
                    uint64_t seed, uint64_t counter, int64_t group_offset, const float* theta,
                    int32_t dim, int64_t* pick_out, float* ess_out, float* theta_out, void* stream);

/* K13: seeded k-means (Lloyd) of pts [n_rows, dim] into k clusters.  centers [k, dim] float32,
 * labels [n_rows] int64, counts [k] int64, n_iter [1] int64 -- all DEVICE.  Deterministic:
 * the same inputs and seed give the same bits on every run.
 * The algorithm (TabPFN_Based_Uncond_Estimator's clustering, reference npe_pfn.py:793-794;
 * all distances and sums in fp64 on the fp32 points):
 *  - tol_abs = tol * mean_j(population variance of column j) (sklearn's scaling of tol);
 *  - k-means++ seeding, one candidate per centre, u_c = Philox4x32-10(counter = (c, 0),
 *    key = seed): centre 0 = row min(floor(u_0 n), n - 1); centre c = the first row whose
 *    inclusive prefix sum of d2 (squared distance to the nearest chosen centre) exceeds
 *    u_c * sum(d2) (the last row with d2 > 0 if rounding puts the target past the total;
 *    row min(floor(u_c n), n - 1) if sum(d2) == 0);
 *  - Lloyd: labels = nearest centre (ties: lower index), centre = fp64 mean of its members
 *    (an empty cluster keeps its centre), shift = sum_c |new_c - old_c|^2; stops after the
 *    iteration with shift <= tol_abs or at max_iter; n_iter = iterations run;
 *  - the centres are rounded to fp32 and stored; labels and counts are computed against the
 *    stored centres, so npfn_kmeans_assign(pts, centers) returns labels bit for bit.
 * Iterations past convergence are no-ops on the device; the host reads the device's
 * convergence flag every 8 iterations, and for that read alone this call WAITS on the stream
 * (so it cannot be captured into a graph); it returns with the final assignment queued.
 * Errors: NPFN_EINVAL for k < 1, k > n_rows, dim < 1, k * dim > 4096 (the centres are held
 * in LDS as fp64, 32 KB) or n_rows >= 2^31; NPFN_ENOMEM when the workspace (8 n_rows bytes +
 * at most 16 MB of partial sums) does not fit; NPFN_EHIP for a launch error. */
int npfn_kmeans_fit(const float* pts, int64_t n_rows, int32_t dim, int32_t k, uint64_t seed,
                    int32_t max_iter, float tol, float* centers, int64_t* labels, int64_t* counts,
                    int64_t* n_iter, void* stream);
/* K13 predict: labels[i] = argmin_c ||pts[i] - centers[c]||^2 (ties: lower c), fp64 distances
 * of the fp32 inputs (KMeans.predict, reference npe_pfn.py:855).  Asynchronous.  Same caps on
 * dim, k * dim and n_rows as npfn_kmeans_fit.  n_rows == 0 launches nothing (pts and labels
 * may then be NULL). */
int npfn_kmeans_assign(const float* pts, int64_t n_rows, int32_t dim, const float* centers, int32_t k,
                       int64_t* labels, void* stream);

/* Estimator-parallel split (npe_pfn/distributed.py): from the next fit on,
 * fits and forwards compute only estimators [e0, e0 + count) of cfg.n_estimators (the
 * feature permutation and preprocessing of estimator e are the same as in the full
 * ensemble).  Calls that mix the ensemble (predict, predict_proba, ar_sample, ar_log_prob,
 * fit_classes) need the full range (0, n_estimators).  Invalidates the fit. */
int npfn_set_estimator_range(npfn_engine* h, int32_t e0, int32_t count);
/* The strided generalisation: fits and forwards compute estimators e0 + stride * i,
 * i < count (npfn_set_estimator_range = stride 1).  npfn_forward_targets writes their target
 * tokens in that order.  Estimator-parallel sampling gives rank r of an EP group of g ranks
 * the set (r, E / g, g), so that every rank holds the same mix of the ensemble's
 * preprocessing pipelines (the ensemble mode's estimators 0-3 and 4-7 differ in token
 * count by about 2x, which a contiguous split would put on different ranks). */
int npfn_set_estimator_set(npfn_engine* h, int32_t e0, int32_t count, int32_t stride);

/* The test-side forward of the estimator range over Xq [n_rows, n_features of the last
 * fit]: tokens_out (bf16, [count][n_rows][192]) = the last layer's target token of every
 * (estimator, row) -- the decoder input of predict (npe_pfn.py:143 up to the head). */
int npfn_forward_targets(npfn_engine* h, const float* Xq, int64_t ldq, int64_t n_rows, void* tokens_out,
                         void* stream);

/* The same forward plus the decoder head, before the ensemble mix: logits_out (fp16,
 * [count][n_rows][n_bars]) = the decoder logits of every (estimator, row) of the estimator
 * range, as npfn_predict's mix reads them.  Works under a partial range (nothing is mixed):
 * the per-estimator view for tests and diagnostics. */
int npfn_forward_logits(npfn_engine* h, const float* Xq, int64_t ldq, int64_t n_rows, void* logits_out,
                        void* stream);

/* Decoder head + ensemble mix + criterion.sample (+ NLL) of one autoregressive step
 * (npe_pfn.py:143-159) from the target tokens of ALL estimators: tokens (bf16,
 * [n_est][n_rows][192], n_est = cfg.n_estimators).  theta_out [n_rows]; row i draws
 * Philox row row_base + i at `counter`; if log_prob_acc != NULL its row i gets the step's
 * log density added (-inf -> log(eps)).  npfn_forward_targets + this = one step of
 * npfn_ar_sample, bit for bit. */
int npfn_head_sample(npfn_engine* h, const void* tokens, int32_t n_est, int64_t n_rows, uint64_t counter,
                     int64_t row_base, float* theta_out, float* log_prob_acc, float eps, void* stream);

/* The per-step fits of an autoregressive call driven step by step (the fit of
 * npe_pfn.py:135-140 for AR dimension k = fit on (x_ctx, theta_ctx[:, :k]) -> theta_ctx[:, k]),
 * for callers that run the steps themselves (estimator-parallel sampling: npfn_forward_targets
 * + an exchange + npfn_head_sample per step).  npfn_ar_fit_begin copies the context and, under
 * a fit token (npfn_set_fit_token), queues every step's preprocessing fit on the engine's side
 * stream at once (they read only the context); npfn_ar_fit_step(k) then makes step k's fit the
 * current one (its train forward after its preprocessing, or nothing when an earlier call under
 * the same token fitted it).  Without a token, step k is fitted in order on `stream`.  The
 * results equal npfn_fit(x_ctx | theta_ctx[:, :k], theta_ctx[:, k]) bit for bit. */
int npfn_ar_fit_begin(npfn_engine* h, const float* x_ctx, const float* theta_ctx, int64_t n_ctx, int32_t dim_x,
                      int32_t dim_theta, void* stream);
int npfn_ar_fit_step(npfn_engine* h, int32_t k, void* stream);

/* Fit reuse across calls (the reference refits inside every accept/reject batch,
 * npe_pfn.py:135-140 reached from accept_reject_sampler.py:51; the fit is deterministic):
 * while token != 0, npfn_ar_sample / npfn_ar_log_prob keep the fit of every AR step and
 * the next call with the same token, context shape, mode and estimator range uses them
 * instead of refitting.  The caller promises that the context (x_ctx, theta_ctx) is the
 * same for all calls under one token -- e.g. one token per sample() call.  0 (default)
 * refits every call.  npfn_fit / npfn_fit_classes never touch the cached fits.
 * Under a NEW non-zero token the fits are looked up in the fit cache (below) before anything
 * is refitted. */
int npfn_set_fit_token(npfn_engine* h, uint64_t token);

/* Fit cache: the per-step fits outlive their token.  Unlike the reference, which refits at
 * every step of every call, the engine refits only when the context table or a fit-relevant
 * setting has changed.  A cached set holds the fits of every AR step of one context table:
 * per step the preprocessing fits, the preprocessed train table and the train-side K/V cache
 * (n_layers * sum_e C_e * 6 * ntile * 2048 bf16 values; about 1 GB per step and 10 GB per set
 * at 1000 context rows, 10 + 10 columns and 8 estimators), plus the engine's own copy of the
 * table (n_ctx * (dim_x + dim_theta) floats).
 * The first npfn_ar_* / npfn_ar_fit_begin call under a new non-zero token compares its context
 * with the cached sets whose key is equal -- the key is (n_ctx, dim_x, dim_theta, the
 * preprocessing mode with its regressor / classifier pipelines and quantile divisor, the
 * estimator set) -- over the full content, on the 32-bit patterns (a table with NaN cells can
 * hit; +0 and -0 differ), never by address: one small kernel, one copy of a flag per candidate
 * back to the host and one synchronize of `stream`.  On a hit the set's fitted steps are used
 * as they are and only steps it does not hold yet are fitted; on a miss a free set, or the
 * least recently used one, is refitted.  The results are bit for bit those of a refit.
 * Calls on different streams are ordered by events inside the engine; the stepwise readers
 * (npfn_forward_targets / npfn_head_sample after npfn_ar_fit_step) are not, and stay on one
 * stream.  npfn_set_preprocessing and a switch between the regressor's and the classifier's
 * pipelines forget every cached fit; npfn_set_estimator_set keeps them (the set is in the key).
 * max_sets: sets kept (default 1: the memory one call holds anyway; 0: no reuse across tokens);
 * max_bytes: device memory of all sets, 0 = no limit (default) -- when a call leaves more than
 * that resident, least recently used sets are freed, down to one. */
int npfn_set_fit_cache(npfn_engine* h, int32_t max_sets, uint64_t max_bytes);
/* Lookups under new tokens that hit / missed since creation, sets that hold fits, and the device
 * memory of all sets.  Any pointer may be NULL. */
int npfn_fit_cache_stats(npfn_engine* h, uint64_t* hits, uint64_t* misses, int32_t* sets, uint64_t* bytes);
/* Frees every cached set (synchronizes with the calls that use them). */
int npfn_fit_cache_clear(npfn_engine* h);

/* Query rows per forward chunk of npfn_predict / npfn_predict_proba / npfn_ar_sample /
 * npfn_ar_log_prob (default 16384).  The reference runs one `predict` over every query
 * row (960 000 at config c5, npe_pfn.py:199, 211-241); the engine splits it into chunks
 * of this many rows to bound its workspaces.  Results do not depend on it beyond
 * floating-point summation order (tests cross the chunk boundaries this way). */
int npfn_set_chunk_rows(npfn_engine* h, int64_t rows);

/* Live per-kernel timing for bench.py: while enabled, every launch the engine
 * makes is bracketed by a HIP event pair on its stream; npfn_prof_read
 * synchronizes, returns per-kernel-function totals (launch count, summed
 * duration, algorithmic FLOPs and bytes) and resets the record.  While enabled, the AR
 * calls' fits run in order on the caller's stream instead of on the side streams, so that
 * every event pair times its launch alone (same results, less overlap). */
typedef struct npfn_prof_entry {
  char name[48];
  int64_t launches;
  double ms;
  double flops;
  double bytes;
} npfn_prof_entry;

int npfn_prof_enable(npfn_engine* h, int enable);
int npfn_prof_read(npfn_engine* h, npfn_prof_entry* out, int32_t max_entries, int32_t* n_entries);

/* Diagnostics: copies the first `rows` rows of the preprocessed table of the last fit or
 * forward ([rows][*vw_out] float32: raw | quantile | SVD | power | fingerprints, see
 * npfn_kernels.h ViewLayout) to the HOST buffer out (capacity rows * max_cols floats).
 * Synchronous.  Used by the tests to pin the device SVD and SHA-256 fingerprints. */
int npfn_debug_views(npfn_engine* h, float* out, int64_t rows, int32_t max_cols, int32_t* vw_out);

/* Diagnostics: the target-border translation of the last regressor fit, copied to HOST buffers.
 * Synchronous.  n_bars / n_est must be the engine's (they size the buffers).  ystats [6]: the
 * target's mean, std and the fit's third statistic, then (ensemble mode) mean, std and mean
 * z-score of the Yeo-Johnson-transformed target; *ylam its lambda; idx / share [n_bars + 1]: per
 * common border the source bucket and the share of it left of the border, share = -1 for a border
 * at / below the source range and 2 for one at / above it; tcancel [n_bars]: 1 for a bar the
 * border repair cancelled; ett [n_est]: 1 for an estimator whose bars are translated;
 * *translated = 1.  When no estimator of the current preprocessing mode transforms its target,
 * *translated = 0, ett is all 0, ystats[0..2] are written, ystats[3..5] and *ylam are NaN and the
 * tables are left alone ("no translation").  Used by the tests to feed npfn_mix_rows the engine's
 * own tables.
 * Errors: NPFN_EINVAL for a NULL engine or pointer, or n_bars / n_est that are not the engine's;
 * NPFN_ESTATE before a regressor fit. */
int npfn_debug_target_translation(npfn_engine* h, int32_t n_bars, int32_t n_est, double* ylam, float* ystats,
                                  int32_t* idx, float* share, uint8_t* tcancel, int32_t* ett,
                                  int32_t* translated);

/* Diagnostics: the ensemble mix and its step tails on caller-made logits (needs no engine).  One
 * 256-thread workgroup per row; the kernels are those of npfn_predict / npfn_ar_sample /
 * npfn_ar_log_prob / npfn_ar_score, picked by op through the same launchers, so a call on
 * npfn_forward_logits' output with npfn_debug_target_translation's tables reproduces those calls
 * bit for bit.  All pointers but the stream are DEVICE pointers.  Asynchronous.
 *   logits [n_est][ld_rows][n_bars] fp16; rows [row0, row0 + n_rows) are mixed (a window only for
 *   NPFN_MIX_LOG; the other ops need row0 = 0, ld_rows = n_rows).  Estimator e's row gives q_e =
 *   softmax(logits * inv_temperature); where ett[e] != 0 the bars with tcancel != 0 are removed
 *   first and q_e is translated through tab ([n_bars + 1] pairs (int32 idx, float share), the
 *   layout of npfn_debug_target_translation's idx / share interleaved).  ett / tab / tcancel may
 *   all be NULL (no translation); tcancel must be readable to n_bars + 4 bytes.  The mixture is
 *   p = mean_e q_e, or softmax(mean_e log q_e) for geo = 1.  An estimator row with no finite
 *   logit (after the cancelled bars are removed) has no mass: it adds nothing to the mean (the
 *   mean still divides by n_est), and under geo, or when every estimator is empty, the row has
 *   no mass at all.  Both code paths (the register path for n_bars % 4 == 0 up to 8192 bars and
 *   the generic one) follow this rule.  A row with no mass gives p = 0 (log: -inf), NaN for its
 *   draw, log density and CDF, as npfn_bar_stats documents.
 *   NPFN_MIX_LOG   out0[r * ldo + b] = log p_b (ldo >= n_bars).
 *   NPFN_MIX_PROB  out0[r * n_bars + b] = p_b.
 *   NPFN_MIX_SAMPLE  row r is global row g = row_offset + r: u = the Philox uniform of (seed,
 *     counter, philox_row0 + g); feat[g * ldf + col] = the draw (npfn_bar_sample's arithmetic on
 *     the borders bz * ystats[1] + ystats[0], bz [n_bars + 1]); if out0 != NULL, out0[g] += the
 *     draw's log density (-inf -> log_eps).
 *   NPFN_MIX_NLL   out0[g] += log density of feat[g * ldf + col] (npfn_bar_nll; -inf -> log_eps).
 *   NPFN_MIX_SCORE out0[g * ldo] = that log density, out1[g * ldo] = the CDF there (npfn_bar_cdf);
 *     either may be NULL.
 *   NPFN_MIX_GROUP_SAMPLE / _NLL / _SCORE  the same three tails with `logits` holding fp32 masses
 *     [*, n_bars] (a NPFN_MIX_PROB result): global row g reads row g / per.  n_est,
 *     inv_temperature, the translation, geo, ld_rows and row0 are ignored.  Equal to their
 *     NPFN_MIX_* twins bit for bit.
 * Errors (host, before any launch; message starting "mix_rows"): NPFN_EINVAL for an unknown op;
 * n_rows < 0 or >= 2^31; n_bars < 2; NULL logits; n_est outside 1..64; inv_temperature not
 * positive and finite; ett / tab / tcancel partly given; geo outside 0..1; a row window outside
 * ld_rows, or any window for an op other than NPFN_MIX_LOG; per < 1 (group ops); for the tails a
 * NULL bz / ystats / feat, row_offset < 0 or col outside [0, ldf); a missing output (out0; for
 * score both NULL, or ldo < 1; for log ldo < n_bars); or n_bars whose LDS need per workgroup --
 * 64 + 4 n_bars (+ 8 n_bars with translation; the register path overlays the two) + 2048 B --
 * exceeds hipDeviceAttributeMaxSharedMemoryPerBlock (such a call is never launched;
 * npfn_engine_create refuses the same n_bars).  NPFN_EHIP if the runtime refuses the launch.
 * n_rows = 0 is a no-op. */
#define NPFN_MIX_LOG 0
#define NPFN_MIX_PROB 1
#define NPFN_MIX_SAMPLE 2
#define NPFN_MIX_NLL 3
#define NPFN_MIX_SCORE 4
#define NPFN_MIX_GROUP_SAMPLE 5
#define NPFN_MIX_GROUP_NLL 6
#define NPFN_MIX_GROUP_SCORE 7
int npfn_mix_rows(int32_t op, const void* logits, int64_t ld_rows, int64_t row0, int64_t n_rows, int32_t n_est,
                  int32_t n_bars, float inv_temperature, const int32_t* ett, const void* tab,
                  const uint8_t* tcancel, int32_t geo, const float* bz, const float* ystats, uint64_t seed,
                  uint64_t counter, int64_t row_offset, uint64_t philox_row0, int64_t per, float* feat,
                  int64_t ldf, int32_t col, float* out0, float* out1, int64_t ldo, float log_eps, void* stream);

/* Diagnostics (process-wide): enable != 0 makes every item-attention block run its
 * online-softmax pass as well (the fallback of the reference-free first pass), so the
 * tests can compare both.  Off by default. */
int npfn_debug_item_attn_online(int enable);

/* Diagnostics (process-wide): every item-attention score is multiplied by scale (> 0; 1 by
 * default) -- stress runs that push queries out of the reference-free first pass's range
 * (bench.py --ia-stress).  Changes results; never set on a sampling path. */
int npfn_debug_item_attn_scale(float scale);

/* Diagnostics: the engine's n-th next row-kernel launch (n >= 1; 0 = off) is refused by the
 * HIP runtime (an oversized block; nothing runs on the device).  The call that hits one returns
 * NPFN_EHIP and leaves the engine usable: the stream's tile counter is not advanced for a
 * launch that did not go in, so later calls compute every tile (tests/test_gpu_engine.py). */
int npfn_debug_fail_row_launch(npfn_engine* h, int32_t n);

/* Item-attention fallback accounting of this engine since the last reset: out4[0] blocks that
 * ran the online-softmax pass, out4[1] blocks launched, out4[2] query rows that took the online
 * pass's result, out4[3] query rows ((token, head) queries / 32 lanes: ny * R per launch).
 * HOST output, synchronous; reset != 0 clears the counters.  Reference call of the path:
 * npe_pfn.py:143 (predict) -- the first pass is exact while every query's row sum stays in
 * [2^-100, 2^100]. */
int npfn_item_attn_fallback(npfn_engine* h, uint64_t* out4, int reset);

/* The fallback rows of npfn_item_attn_fallback split by cause (HOST output, synchronous, since
 * that call's last reset): out2[0] query rows whose first-pass sum overflowed (> 2^100, inf or
 * NaN), out2[1] rows whose sum underflowed (< 2^-100); the rest of out4[2] were forced
 * (npfn_debug_item_attn_online).  The padding keys of the last step are masked to P = 0 in both
 * passes, so padding never causes a fallback.  A query whose max over its FIRST 32 keys lies
 * outside [-64, 16] (log2 units) runs the first pass relative to that max + 60 (its own lane-local
 * reference), so a uniformly large or small score level no longer fails; only a spread of more
 * than ~160 log2 units between those first 32 keys and the rest does (csrc/npfn_kernels.hip,
 * kIaShiftHi / kIaShiftLo / kIaShiftMargin and the comment above them). */
int npfn_item_attn_fallback_causes(npfn_engine* h, uint64_t* out2);

#ifdef __cplusplus
}
#endif
#endif /* NPFN_H */
