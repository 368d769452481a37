"""NPE-PFN estimators (reference: npe_pfn/npe_pfn.py).

Public surface kept from the reference: ``NPE_PFN_Core`` (:26-600),
``TabPFN_Based_NPE_PFN`` (:708-744) and ``TabPFN_Based_Uncond_Estimator`` (:747-900) with ``append_simulations``, ``sample``,
``sample_batched``, ``log_prob`` and pickling.  The autoregressive loop
(``_sample`` :111-169, ``_sample_batched`` :171-251,
``_autoregressive_log_prob`` :462-524) has two implementations:

* **fused** -- when the estimator offers ``ar_sample`` / ``ar_log_prob``
  (the engine-backed :class:`npe_pfn.tabpfn.TabPFNRegressor`), the whole
  dimension loop runs on the GPU in one C-ABI call (``npfn_ar_sample``):
  context and samples stay in HBM, each step's fit is computed once;
* **generic** -- any object with the tabpfn ``fit`` / ``predict`` /
  ``criterion`` surface is driven step by step exactly like the reference.

Both produce the same numbers for the same estimator (tests/test_orchestration.py
pins the generic loop to golden vectors made by the reference itself).
"""

from __future__ import annotations

import contextlib
import math
from typing import Callable, Mapping, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor
from torch.distributions import Distribution

from .accept_reject_sampler import accept_reject_sample
from .diagnostics import (ClassifierTestResult, CoverageRanks, TransportResult, TwoSampleResult, bar_cdf, c2st_batched,
                          mmd_batched, rank_accumulate_host, wasserstein_batched)
from .kmeans import KMeansState
from .marginals import PosteriorMarginals
from .pair_marginals import MAX_PER as PAIR_MAX_PER
from .pair_marginals import PosteriorPairMarginals, grid_edges, pair_accumulate_host, tables_from_sums
from .support_posterior import (get_filtering_method, latest_filtering, no_filtering,
                                standardized_euclidean_filtering)
from .tabpfn import TabPFNClassifier, TabPFNRegressor


DETERMINISTIC_FILTERS = (no_filtering, latest_filtering, standardized_euclidean_filtering)


class NPE_PFN_Core:
    """Training-free neural posterior estimation with a tabular foundation model."""

    def __init__(
        self,
        show_progress_bars: bool = False,
        prior: Optional[Distribution] = None,
        embedding_net: Optional[torch.nn.Module] = None,
        x_shape: Optional[torch.Size] = None,
        regressor_init_kwargs: Mapping = {},
        classifier_init_kwargs: Mapping = {},
    ) -> None:
        self.show_progress_bars = show_progress_bars
        self.prior = prior
        self.embedding_net = embedding_net
        self.x_shape = x_shape
        self.regressor_init_kwargs = dict(regressor_init_kwargs)
        self.classifier_init_kwargs = dict(classifier_init_kwargs)
        self._model = TabPFNRegressor(**self.regressor_init_kwargs)
        self._model_classifier = None
        self._obs_offset = 0  # first observation index of this process's shard (npe_pfn.distributed)
        self._theta_train: Optional[Tensor] = None
        self._x_train: Optional[Tensor] = None

    # ------------------------------------------------------------- pickling
    def __getstate__(self):
        # the estimators hold device state; they are rebuilt on load (reference :57-71)
        state = dict(self.__dict__)
        state["_model"] = None
        state["_model_classifier"] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._model = TabPFNRegressor(**self.regressor_init_kwargs)

    # ------------------------------------------------------------- data
    def _embed(self, x: Tensor) -> Tensor:
        if self.embedding_net is None:
            return x
        return self.embedding_net(x.reshape(-1, *self.x_shape))

    def append_simulations(self, theta: Tensor, x: Tensor):
        """Replace the context table by (theta, x) (reference :73-82)."""
        self._theta_train = None
        self._x_train = None
        x = self._embed(x)
        self._theta_train = self._validate_theta(theta)
        self._x_train = self._validate_x(x)
        return self

    def get_context(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        return self._theta_train, self._x_train

    def _validate_x(self, x: Tensor) -> Tensor:
        if x is None:
            raise NotImplementedError("Setting a default x is not yet supported.")
        if x.ndim == 1:
            x = x.unsqueeze(0)
        assert x.ndim == 2, "x must be a 2D tensor."
        if self._x_train is not None:
            assert x.shape[1] == self._x_train.shape[1], "The number of features in x must match the training data."
        return x

    def _validate_theta(self, theta: Tensor) -> Tensor:
        if theta.ndim == 1:
            theta = theta.unsqueeze(0)
        assert theta.ndim == 2, "theta must be a 2D tensor."
        if self._theta_train is not None:
            assert theta.shape[1] == self._theta_train.shape[1], \
                "The number of features in theta must match the training data."
        return theta

    def _fused(self) -> bool:
        return hasattr(self._model, "ar_sample")

    def _context_is_deterministic(self) -> bool:
        """Whether get_context(x) returns the same table every time it is called with the same x."""
        return True

    def _reuse_fits(self):
        """One context for the block (one sample / sample_batched / log_prob call): the engine
        keeps every AR step's fit across the accept/reject batches instead of refitting.
        Only when the context is a deterministic function of x: a random filter draws a new
        subset per batch and the reference refits on each (npe_pfn.py:128, support_posterior.py:351)."""
        ctx = getattr(self._model, "reuse_fits", None)
        if ctx is None or not self._context_is_deterministic() or getattr(self, "_fits_held", False):
            # (inside a block that already holds a fit token -- coverage_batched scores and
            # samples on one set of fits -- the inner call joins it)
            return contextlib.nullcontext()
        return self._hold_fits(ctx)

    @contextlib.contextmanager
    def _hold_fits(self, ctx):
        self._fits_held = True
        try:
            with ctx():
                yield
        finally:
            self._fits_held = False

    # --------------------------------------------------- autoregressive core
    def _ar_generic(self, x_ctx: Tensor, theta_ctx: Tensor, x_query: Tensor, with_log_prob: bool,
                    eps: float) -> Tuple[Tensor, Optional[Tensor]]:
        """Dimension loop through the tabpfn surface (reference :128-169 / :202-241)."""
        joint = torch.cat([x_ctx, theta_ctx], dim=1)
        dx = x_ctx.shape[1]
        feats = x_query
        lp = torch.zeros(x_query.shape[0]) if with_log_prob else None
        for k in range(theta_ctx.shape[1]):
            self._model.fit(joint[:, : dx + k], joint[:, dx + k])
            pred = self._model.predict(feats, output_type="full", quantiles=[])
            draw = pred["criterion"].sample(pred["logits"])
            if with_log_prob:
                dev = pred["logits"].device
                step = -pred["criterion"](pred["logits"], draw.to(dev))
                step = torch.where(step == float("-inf"), torch.log(torch.tensor(eps, device=step.device)), step)
                lp = lp.to(step.device)
                lp += step
            feats = torch.cat([feats, draw[:, None].to(feats.device)], dim=1)
        return feats[:, dx:], lp

    def _ar(self, x_ctx: Tensor, theta_ctx: Tensor, x_query: Tensor, with_log_prob: bool,
            eps: float, row_base: int = 0, x_unique: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
        """``x_unique``: the distinct rows when ``x_query`` = ``x_unique.repeat_interleave(N // U, 0)``
        (the fused engine then runs AR step 0 once per distinct row)."""
        if self._fused():
            return self._model.ar_sample(x_ctx, theta_ctx, x_query, with_log_prob=with_log_prob, eps=eps,
                                         row_base=row_base, x_unique=x_unique)
        return self._ar_generic(x_ctx, theta_ctx, x_query, with_log_prob, eps)

    def _sample(self, sampling_batch_size: int, x: Tensor, repeat_x: bool = True, with_log_prob: bool = False,
                eps: float = 1e-15, row_base: int = 0, ar: Optional[Callable] = None) -> Tuple[Tensor, Optional[Tensor]]:
        """One batch of posterior draws for a single observation (reference :111-169).

        ``row_base``: Philox row of the batch's first draw (a row shard of a larger batch,
        npe_pfn.distributed); ``ar``: an alternative implementation of the dimension loop
        with :meth:`_ar`'s signature (the estimator-parallel multi-GPU loop).
        """
        x_query = x.repeat(sampling_batch_size, 1) if repeat_x else x
        x_unique = x if repeat_x and x.shape[0] == 1 else None  # one observation: every query row is x
        theta_ctx, x_ctx = self.get_context(x)
        if ar is not None:
            return ar(x_ctx, theta_ctx, x_query, with_log_prob, eps, row_base, x_unique=x_unique)
        return self._ar(x_ctx, theta_ctx, x_query, with_log_prob, eps, row_base=row_base, x_unique=x_unique)

    def _sample_batched(self, x: Tensor, num_samples_per_obs: int, with_log_prob: bool = False,
                        eps: float = 1e-15) -> Tuple[Tensor, Optional[Tensor]]:
        """Obs-major interleaved batch over all observations with the full context (reference :171-251)."""
        n_obs = x.shape[0]
        x_query = x.repeat_interleave(num_samples_per_obs, dim=0)
        # an observation shard [a, b) of a larger batch (npe_pfn.distributed) draws at the
        # Philox rows of the unsharded obs-major batch: row_base = a * samples per obs
        theta, lp = self._ar(self._x_train, self._theta_train, x_query, with_log_prob, eps,
                             row_base=self._obs_offset * num_samples_per_obs,
                             x_unique=x if num_samples_per_obs > 0 else None)
        theta = theta.reshape(n_obs, num_samples_per_obs, -1)
        if with_log_prob:
            return theta, lp.reshape(n_obs, num_samples_per_obs)
        return theta, None

    # ---------------------------------------------------------------- public
    def sample(self, sample_shape: torch.Size = torch.Size(), x: Tensor = None, max_sampling_batch_size: int = 10_000,
               with_log_prob: bool = False, eps: float = 1e-15, max_iter_rejection: Optional[int] = None,
               show_progress_bars: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """Posterior draws for ONE observation with prior-support rejection (reference :253-308)."""
        return self._sample_impl(sample_shape, x, max_sampling_batch_size, with_log_prob, eps, max_iter_rejection)

    def _sample_impl(self, sample_shape, x, max_sampling_batch_size: int, with_log_prob: bool, eps: float,
                     max_iter_rejection: Optional[int], row_base_of: Optional[Callable[[int], int]] = None,
                     ar: Optional[Callable] = None):
        """``sample`` with two multi-GPU hooks (npe_pfn.distributed): ``row_base_of(i)`` = Philox
        row of the first draw of accept/reject batch i, ``ar`` = the dimension loop to use."""
        x = self._validate_x(self._embed(x) if self.embedding_net else x)
        if x.shape[0] > 1:
            raise ValueError(".sample() supports only `batchsize == 1`. If you intend to sample multiple "
                             "observations, use `.sample_batched()`. ")
        out_device = x.device
        batch_index = [0]

        def proposal(batch_size, **_):
            i = batch_index[0]
            batch_index[0] += 1
            rb = row_base_of(i) if row_base_of is not None else 0
            return self._sample(batch_size, x, repeat_x=True, with_log_prob=with_log_prob, eps=eps, row_base=rb,
                                ar=ar)

        with (self._reuse_fits() if ar is None else contextlib.nullcontext()):
            samples, log_probs, _ = accept_reject_sample(
                proposal=proposal,
                accept_reject_fn=self._within_support,
                num_samples=torch.Size(sample_shape).numel(),
                show_progress_bars=self.show_progress_bars,
                max_sampling_batch_size=max_sampling_batch_size,
                proposal_sampling_kwargs={},
                max_iter_rejection=max_iter_rejection,
            )
        samples = samples.to(out_device)
        if with_log_prob:
            return samples, log_probs.to(out_device)
        return samples

    def sample_batched(self, x: Tensor, sample_shape: torch.Size = torch.Size(), max_sampling_batch_size: int = 10_000,
                       with_log_prob: bool = False, eps: float = 1e-15, oversample_factor: float = 1.5,
                       show_progress_bars: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """Posterior draws for many observations at once (reference :310-410).

        ``max_sampling_batch_size`` is accepted and, as in the reference, not used.
        """
        x = self._validate_x(self._embed(x) if self.embedding_net else x)
        n_obs = x.shape[0]
        n = torch.Size(sample_shape).numel()
        if self.prior is None:
            th, lp = self._sample_batched(x, n, with_log_prob=with_log_prob, eps=eps)
            th = th.to(x.device)
            return (th, lp.to(x.device)) if with_log_prob else th
        # Per-observation rejection (reference :360-397), vectorised over observations on the
        # samples' device: an accepted draw's rank within its observation decides whether it is
        # taken and where it lands, so every observation keeps its first accepted draws in
        # order, as the reference's per-observation loop does, with one host sync per round.
        per_round = int(n * oversample_factor)
        with self._reuse_fits():
            return self._sample_batched_rounds(x, n, n_obs, per_round, with_log_prob, eps)

    def _sample_batched_rounds(self, x, n, n_obs, per_round, with_log_prob, eps):
        out_th = out_lp = None
        need = filled = None
        for _ in range(10):
            if need is not None and int(need.sum()) == 0:
                break
            th, lp = self._sample_batched(x, per_round, with_log_prob=with_log_prob, eps=eps)
            dev = th.device
            if out_th is None:
                out_th = torch.empty(n_obs, n, th.shape[-1], dtype=th.dtype, device=dev)
                out_lp = torch.empty(n_obs, n, dtype=lp.dtype, device=dev) if with_log_prob else None
                need = torch.full((n_obs,), n, dtype=torch.int64, device=dev)
                filled = torch.zeros(n_obs, dtype=torch.int64, device=dev)
            ok = self._within_support(th.reshape(n_obs * per_round, -1)).reshape(n_obs, per_round).to(dev)
            rank = torch.cumsum(ok.to(torch.int64), 1) - 1
            sel = ok & (rank < need[:, None])
            oi, ri = sel.nonzero(as_tuple=True)
            dest = filled[oi] + rank[oi, ri]
            out_th[oi, dest] = th[oi, ri]
            if with_log_prob:
                out_lp[oi, dest] = lp.to(dev)[oi, ri]
            taken = sel.sum(1)
            filled += taken
            need -= taken
        if int(need.sum()) != 0:
            # the reference's final torch.stack fails on unequal per-observation counts
            raise RuntimeError(f"sample_batched: {int((need > 0).sum())} observation(s) got fewer than {n} "
                               f"samples inside the prior support after 10 rounds")
        samples = out_th.to(x.device)
        if with_log_prob:
            return samples, out_lp.to(x.device)
        return samples

    def log_prob(self, theta: Tensor, x: Tensor, max_sampling_batch_size: int = 10_000, mode: str = "autoregressive",
                 eps: float = 1e-15, *, leakage_correction: bool = False,
                 support_fraction: Optional[Union[float, Tensor]] = None, num_rejection_samples: int = 10_000,
                 **ratio_kwargs) -> Tensor:
        """log q(theta | x), in chunks of ``max_sampling_batch_size`` rows (reference :412-455).

        ``leakage_correction=True`` (autoregressive mode, needs a prior) returns the log density of
        the posterior truncated to the prior's support, the distribution :meth:`sample` draws
        from: ``log q - log(support_fraction)`` inside the support and ``-inf`` outside (the
        correction the reference leaves as a TODO at ``_autoregressive_log_prob``).
        ``support_fraction`` is taken as given, or estimated once per call by
        :meth:`support_fraction` with ``num_rejection_samples`` draws (which advances the sample
        counter).  The defaults change nothing."""
        if self.embedding_net:
            x = self._embed(x)
        theta = self._validate_theta(theta)
        x = self._validate_x(x)
        if mode not in ("autoregressive", "ratio_based"):
            raise ValueError(f"Invalid mode: {mode}")
        if leakage_correction:
            if mode != "autoregressive":
                raise ValueError("log_prob: leakage_correction applies to mode='autoregressive' only")
            log_frac = self._log_support_fraction(x, support_fraction, num_rejection_samples, 1)
        out = torch.zeros(theta.shape[0])
        with (self._reuse_fits() if mode == "autoregressive" else contextlib.nullcontext()):
            for i in range(0, theta.shape[0], max_sampling_batch_size):
                chunk = theta[i: i + max_sampling_batch_size]
                if mode == "autoregressive":
                    out[i: i + max_sampling_batch_size] = self._autoregressive_log_prob(chunk, x, eps=eps).cpu()
                else:
                    out[i: i + max_sampling_batch_size] = self._ratio_based_log_prob(chunk, x, eps=eps,
                                                                                     **ratio_kwargs).cpu()
        if leakage_correction:
            out = out - log_frac.cpu().to(out.dtype)
            out = torch.where(self._within_support(theta).cpu(), out, torch.full_like(out, float("-inf")))
        return out

    def log_prob_batched(self, theta: Tensor, x: Tensor, eps: float = 1e-15, return_steps: bool = False, *,
                         leakage_correction: bool = False, support_fraction: Optional[Tensor] = None,
                         num_rejection_samples: int = 10_000):
        """Autoregressive log q(theta_m | x_m) of many (theta, x) pairs in one teacher-forced pass
        (the reference declares this method and leaves it unimplemented, :457-460).

        ``x`` [M, dx]; ``theta`` [M, d_theta] gives [M], ``theta`` [M, K, d_theta] (K thetas per
        observation) gives [M, K].  The context is the full table, as in ``sample_batched`` (no
        per-observation filter), so every autoregressive step is fitted once for all pairs.
        ``return_steps=True`` also returns the per-dimension log densities [..., d_theta], whose
        sum over the last axis (in order) is the first result.  On the device of ``x``.

        ``leakage_correction=True`` (needs a prior): the summed result becomes ``log q -
        log(support_fraction)`` (the logarithm taken in fp64, rounded to the result's type) inside
        the prior's support and ``-inf`` outside, as in :meth:`log_prob`; ``support_fraction`` [M]
        is taken as given or estimated once per observation by :meth:`support_fraction` with
        ``num_rejection_samples`` draws.  The per-step values are not corrected."""
        if leakage_correction and self.prior is None:
            raise ValueError("leakage_correction needs a prior: the correction is the prior support's share of q")
        lp, steps, _ = self._score_batched(theta, x, eps, want_logp=True, want_cdf=False)
        if leakage_correction:
            xv =self._validate_x(self._embed(x) if self.embedding_net else x)
            log_frac = self._log_support_fraction(xv, support_fraction, num_rejection_samples, xv.shape[0])
            log_frac = log_frac.to(device=lp.device, dtype=lp.dtype).reshape(-1, *([1] * (lp.ndim - 1)))
            th = torch.as_tensor(theta)
            inside = self._within_support(th.reshape(-1, th.shape[-1])).reshape(lp.shape).to(lp.device)
            lp = torch.where(inside, lp - log_frac, torch.full_like(lp, float("-inf")))
        return (lp, steps) if return_steps else lp

    def support_fraction(self, x: Tensor, num_draws: int = 10_000, max_sampling_batch_size: int = 10_000) -> Tensor:
        """[M] float64: the share of ``num_draws`` unrejected sampler draws per observation that lie
        inside the prior's support -- one minus the estimator's leakage, the normalising constant
        of the truncated posterior that :meth:`sample` draws from.

        ``x`` is [dx] or [1, dx] (the context is ``get_context(x)``, as in :meth:`sample`) or [M,
        dx] (the full table, as in :meth:`sample_batched`); at most ``max_sampling_batch_size``
        query rows go into one sampler call.  Plain sampler calls: the sample counter advances as
        in :meth:`sample`.  On the device of ``x``.  ValueError without a prior."""
        if self.prior is None:
            raise ValueError("support_fraction: the estimator has no prior, so there is no support to leak from")
        x = self._validate_x(self._embed(x) if self.embedding_net else x)
        return self._support_fraction(x, int(num_draws), int(max_sampling_batch_size))

    def _support_fraction(self, x: Tensor, num_draws: int, cap: int) -> Tensor:
        """:meth:`support_fraction` of an ``x`` that is already embedded and validated."""
        n_obs = x.shape[0]
        if num_draws < 1 or cap < 1:
            raise ValueError(f"support_fraction: num_draws ({num_draws}) and max_sampling_batch_size ({cap}) must "
                             "be >= 1")
        if n_obs == 1:
            theta_ctx, x_ctx = self.get_context(x)
        else:
            theta_ctx, x_ctx = self._theta_train, self._x_train
        per_call = max(1, cap // n_obs)
        counts = None
        done = 0
        with self._reuse_fits():
            while done < num_draws:
                d = min(per_call, num_draws - done)
                rb = self._obs_offset * d if n_obs > 1 else 0
                th, _ = self._ar(x_ctx, theta_ctx, x.repeat_interleave(d, dim=0), False, 1e-15, row_base=rb,
                                 x_unique=x)
                ok = self._within_support(th).reshape(n_obs, d).sum(1)
                counts = ok if counts is None else counts + ok.to(counts.device)
                done += d
        return counts.to(device=x.device, dtype=torch.float64) / num_draws

    def _log_support_fraction(self, x: Tensor, given, num_draws: int, n_obs: int) -> Tensor:
        """log of the support fraction of each of ``n_obs`` observations (float64 [n_obs]): ``given``
        if passed, else :meth:`support_fraction` of ``x``.  ValueError without a prior, for a wrong
        number of fractions, or for a fraction of 0 (nothing to normalise by)."""
        if self.prior is None:
            raise ValueError("leakage_correction needs a prior: the correction is the prior support's share of q")
        if given is None:
            frac = self._support_fraction(x, int(num_draws), 10_000)
        else:
            frac = torch.as_tensor(given, dtype=torch.float64).reshape(-1)
            if frac.numel() == 1 and n_obs > 1:
                frac = frac.expand(n_obs)
        if frac.numel() != n_obs:
            raise ValueError(f"support_fraction has {frac.numel()} entries for {n_obs} observation(s)")
        if not bool((frac > 0).all()):
            raise ValueError("leakage_correction: a support fraction of 0 (no draw inside the prior's support) "
                             "cannot normalise the density")
        return torch.log(frac)

    def coverage_batched(self, theta_true: Tensor, x: Tensor, num_posterior_samples: int = 1000,
                         references: Optional[Tensor] = None, max_sampling_batch_size: int = 10_000,
                         oversample_factor: float = 1.5, eps: float = 1e-15,
                         return_samples: bool = False) -> CoverageRanks:
        """Coverage ranks of M true parameters among ``num_posterior_samples`` posterior draws each:
        simulation-based-calibration ranks per parameter, the HPD rank (draws denser than the
        truth) and the TARP rank (draws closer to a reference point than the truth), as a
        :class:`npe_pfn.diagnostics.CoverageRanks` (:func:`~npe_pfn.diagnostics.rank_ks_statistic`
        and :func:`~npe_pfn.diagnostics.expected_coverage` read it).

        ``theta_true`` [M, d_theta] (finite), ``x`` [M, dx]; the context is the full table, as in
        :meth:`sample_batched` / :meth:`log_prob_batched`.  Observations go in blocks of ``max(1,
        max_sampling_batch_size // int(S * oversample_factor))``; a block scores its truths and
        draws on one set of fits, with :meth:`sample_batched`'s rounds and selection rule (an
        observation keeps its first S accepted draws in order), and every round is folded into
        integer counts as it is produced (``npfn_rank_accumulate`` on the engine,
        :func:`~npe_pfn.diagnostics.rank_accumulate_host` otherwise): without
        ``return_samples=True`` no [M, S, ...] buffer exists.  The sample counter advances as
        ``sample_batched`` on each block in turn would advance it, and the draws are those calls'.

        With a prior, all ranks refer to the posterior truncated to the prior's support, the
        draws ``sample_batched`` returns.  The truncation divides the density of the truth and of
        every draw of one observation by the same support fraction, so the constant cancels in
        the HPD comparison and the uncorrected log densities are compared (``log_prob_true`` is
        :meth:`log_prob_batched`'s, uncorrected).

        TARP ``references`` [M, d_theta]: as given; by default ``prior.sample((M,))``, without a
        prior uniform between the per-dimension minimum and maximum of the context thetas (CPU
        torch generator).  Distances are scaled per dimension by ``inv_scale`` = 1 / (max - min)
        of the context thetas (1 where they coincide).  RuntimeError when an observation is still
        short after 10 rounds, like ``sample_batched``.  Results on the device of ``x``."""
        x = self._validate_x(self._embed(x) if self.embedding_net else x)
        theta_true = torch.as_tensor(theta_true)
        n_obs, dth = x.shape[0], self._theta_train.shape[1]
        if theta_true.ndim != 2 or theta_true.shape != (n_obs, dth):
            raise ValueError(f"coverage_batched: theta_true {tuple(theta_true.shape)} is not [{n_obs}, {dth}] (one "
                             "true parameter per row of x)")
        if not bool(torch.isfinite(theta_true).all()):
            raise ValueError("coverage_batched: theta_true has non-finite entries")
        n, cap = int(num_posterior_samples), int(max_sampling_batch_size)
        if n < 1 or cap < 1:
            raise ValueError(f"coverage_batched: num_posterior_samples ({n}) and max_sampling_batch_size ({cap}) "
                             "must be >= 1")
        ctx_lo = self._theta_train.min(dim=0).values.to(torch.float32)
        ctx_hi = self._theta_train.max(dim=0).values.to(torch.float32)
        span = ctx_hi - ctx_lo
        inv_scale = torch.where(span > 0, 1.0 / torch.where(span > 0, span, torch.ones_like(span)),
                                torch.ones_like(span))
        if references is not None:
            references = torch.as_tensor(references)
            if references.shape != (n_obs, dth):
                raise ValueError(f"coverage_batched: references {tuple(references.shape)} is not [{n_obs}, {dth}]")
        elif self.prior is not None:
            references = self.prior.sample((n_obs,)).reshape(n_obs, dth)
        else:
            references = ctx_lo.cpu() + torch.rand(n_obs, dth) * span.cpu()
        references = references.to(torch.float32)
        per_round = int(n * oversample_factor) if self.prior is not None else n
        block = max(1, cap // max(1, int(n * oversample_factor)))
        parts = []
        for a in range(0, n_obs, block):
            b = min(n_obs, a + block)
            with self._reuse_fits():
                parts.append(self._coverage_block(theta_true[a:b], x[a:b], references[a:b], inv_scale, n, per_round,
                                                  eps, return_samples))
        dev = x.device
        cat = [None if p[0] is None else torch.cat(p, 0).to(dev) for p in zip(*parts)]
        counts, lp_true, samples, sample_lp = cat
        return CoverageRanks(counts[:, :, 0].contiguous(), counts[:, :, 1].contiguous(), n, lp_true,
                             references.to(dev), inv_scale.to(dev), samples, sample_lp)

    def _coverage_block(self, theta_true, x, references, inv_scale, n, per_round, eps, return_samples):
        """One block of :meth:`coverage_batched` under one fit token: (counts [B, d_theta + 2, 2],
        log_prob_true [B], samples or None, sample_log_probs or None), on the sampler's device
        except ``log_prob_true`` (the device of ``x``)."""
        n_obs, dth = theta_true.shape
        lp_true, _, _ = self._score_batched(theta_true, x, eps, want_logp=True, want_cdf=False)
        counts = need = filled = out_th = out_lp = None
        for _ in range(10):
            if need is not None and int(need.sum()) == 0:
                break
            th, lp = self._sample_batched(x, per_round, with_log_prob=True, eps=eps)
            dev = th.device
            lp = lp.to(dev)
            if counts is None:
                counts = torch.zeros((n_obs, dth + 2, 2), dtype=torch.int64, device=dev)
                need = torch.full((n_obs,), n, dtype=torch.int64, device=dev)
                filled = torch.zeros(n_obs, dtype=torch.int64, device=dev)
                truth = [t.to(dev).contiguous() for t in (theta_true, lp_true, references, inv_scale)]
                if return_samples:
                    out_th = torch.empty(n_obs, n, dth, dtype=th.dtype, device=dev)
                    out_lp = torch.empty(n_obs, n, dtype=lp.dtype, device=dev)
            if self.prior is None:
                sel, taken = None, torch.full_like(need, per_round)
            else:
                # sample_batched's selection: an observation keeps its first accepted draws in order
                ok = self._within_support(th.reshape(n_obs * per_round, -1)).reshape(n_obs, per_round).to(dev)
                rank = torch.cumsum(ok.to(torch.int64), 1) - 1
                sel = ok & (rank < need[:, None])
                taken = sel.sum(1)
            if self._fused() and dev.type == "cuda":
                fold = self._model.engine.rank_accumulate
            else:
                fold = rank_accumulate_host
            fold(th.reshape(n_obs * per_round, dth), lp.reshape(-1), None if sel is None else sel.reshape(-1), n_obs,
                 per_round, truth[0], truth[1], truth[2], truth[3], counts)
            if return_samples:
                if sel is None:
                    out_th.copy_(th)
                    out_lp.copy_(lp)
                else:
                    oi, ri = sel.nonzero(as_tuple=True)
                    dest = filled[oi] + rank[oi, ri]
                    out_th[oi, dest] = th[oi, ri]
                    out_lp[oi, dest] = lp[oi, ri]
            filled += taken
            need -= taken
        if int(need.sum()) != 0:
            raise RuntimeError(f"coverage_batched: {int((need > 0).sum())} observation(s) got fewer than {n} samples "
                               "inside the prior support after 10 rounds")
        return counts, lp_true, out_th, out_lp

    def mmd_batched(self, theta_ref: Tensor, x: Tensor, num_posterior_samples: Optional[int] = None,
                    **kw) -> TwoSampleResult:
        """MMD two-sample test of this estimator's draws against reference draws, observation by
        observation: ``theta_ref`` [M, T, d_theta] are the reference draws (a ground-truth
        posterior, another estimator, another seed) for ``x`` [M, dx].  Draws
        ``num_posterior_samples`` (default T) per observation with :meth:`sample_batched` -- the
        sample counter advances as that call advances it -- and returns
        :func:`npe_pfn.diagnostics.mmd_batched` ``(draws, theta_ref, **kw)``: ``kernel``,
        ``bandwidths``, ``num_permutations``, ``seed`` and ``z_score`` are its arguments."""
        theta_ref = torch.as_tensor(theta_ref)
        n_obs = 1 if torch.as_tensor(x).ndim < 2 else x.shape[0]
        dth = self._theta_train.shape[1]
        if theta_ref.ndim != 3 or theta_ref.shape[0] != n_obs or theta_ref.shape[1] < 1 or theta_ref.shape[2] != dth:
            raise ValueError(f"mmd_batched: theta_ref {tuple(theta_ref.shape)} is not [{n_obs}, T >= 1, {dth}] (the "
                             "reference draws of every row of x)")
        n = theta_ref.shape[1] if num_posterior_samples is None else int(num_posterior_samples)
        if n < 1:
            raise ValueError(f"mmd_batched: num_posterior_samples ({n}) must be >= 1")
        draws = self.sample_batched(x, (n,))
        engine = self._model.engine if self._fused() and draws.device.type == "cuda" else None
        return mmd_batched(draws, theta_ref.to(draws.device), engine=engine, **kw)

    def wasserstein_batched(self, theta_ref: Tensor, x: Tensor, num_posterior_samples: Optional[int] = None,
                            **kw) -> TransportResult:
        """Exact 2-Wasserstein distance of this estimator's draws from reference draws, observation
        by observation: ``theta_ref`` [M, T, d_theta] are the reference draws for ``x`` [M, dx].
        Draws T per observation with :meth:`sample_batched` -- the sample counter advances as that
        call advances it -- and returns :func:`npe_pfn.diagnostics.wasserstein_batched` ``(draws,
        theta_ref, **kw)`` (``z_score`` is its argument).  The two sets must be of equal size, so
        ``num_posterior_samples`` is T or None."""
        theta_ref = torch.as_tensor(theta_ref)
        n_obs = 1 if torch.as_tensor(x).ndim < 2 else x.shape[0]
        dth = self._theta_train.shape[1]
        if theta_ref.ndim != 3 or theta_ref.shape[0] != n_obs or theta_ref.shape[1] < 1 or theta_ref.shape[2] != dth:
            raise ValueError(f"wasserstein_batched: theta_ref {tuple(theta_ref.shape)} is not [{n_obs}, T >= 1, {dth}] "
                             "(the reference draws of every row of x)")
        T = theta_ref.shape[1]
        if num_posterior_samples is not None and int(num_posterior_samples) != T:
            raise ValueError(f"wasserstein_batched: num_posterior_samples ({num_posterior_samples}) must equal the "
                             f"{T} reference draws per observation: uniform transport between sets of unequal size "
                             "is not an assignment")
        draws = self.sample_batched(x, (T,))
        engine = self._model.engine if self._fused() and draws.device.type == "cuda" else None
        return wasserstein_batched(draws, theta_ref.to(draws.device), engine=engine, **kw)

    def c2st_batched(self, theta_ref: Tensor, x: Tensor, num_posterior_samples: Optional[int] = None,
                     **kw) -> ClassifierTestResult:
        """Classifier two-sample test of this estimator's draws against reference draws,
        observation by observation: ``theta_ref`` [M, T, d_theta] are the reference draws for ``x``
        [M, dx].  Draws ``num_posterior_samples`` (default T) per observation with
        :meth:`sample_batched` -- the sample counter advances as that call advances it -- and
        returns :func:`npe_pfn.diagnostics.c2st_batched` ``(draws, theta_ref, **kw)``: ``seed``,
        ``n_folds``, ``model``, ``z_score``, ``epochs``, ``batch_size``, ``lr``, ``weight_decay`` and
        ``return_probs`` are its arguments.  The draws are the first set, as in the reference
        harness, so they set the z-score."""
        theta_ref = torch.as_tensor(theta_ref)
        n_obs = 1 if torch.as_tensor(x).ndim < 2 else x.shape[0]
        dth = self._theta_train.shape[1]
        if theta_ref.ndim != 3 or theta_ref.shape[0] != n_obs or theta_ref.shape[1] < 1 or theta_ref.shape[2] != dth:
            raise ValueError(f"c2st_batched: theta_ref {tuple(theta_ref.shape)} is not [{n_obs}, T >= 1, {dth}] (the "
                             "reference draws of every row of x)")
        n = theta_ref.shape[1] if num_posterior_samples is None else int(num_posterior_samples)
        if n < 1:
            raise ValueError(f"c2st_batched: num_posterior_samples ({n}) must be >= 1")
        draws = self.sample_batched(x, (n,))
        engine = self._model.engine if self._fused() and draws.device.type == "cuda" else None
        return c2st_batched(draws, theta_ref.to(draws.device), engine=engine, **kw)

    def pit_batched(self, theta: Tensor, x: Tensor) -> Tensor:
        """Per-dimension probability integral transform u_k = F_k(theta_k | x, theta_<k) of the
        pairs of :meth:`log_prob_batched` (same shapes): [..., d_theta].  Uniform on [0, 1] in
        dimension k exactly when conditional k is calibrated on the true pairs
        (:func:`npe_pfn.diagnostics.pit_ks_statistic`); needs no posterior samples."""
        return self._score_batched(theta, x, 1e-15, want_logp=False, want_cdf=True)[2]

    def marginals(self, x: Tensor, num_draws: int = 10_000, max_sampling_batch_size: int = 10_000,
                  return_samples: bool = False) -> PosteriorMarginals:
        """Per-parameter posterior marginals q(theta_k | x) as bar distributions, averaged over the
        conditionals of ``num_draws`` sampler draws per observation ("Rao-Blackwellised": the
        mean over the draws of the full predictive distribution each theta_k was drawn from,
        instead of a histogram of the draws; no extra forward pass).

        ``x`` is [dx] or [1, dx] (one observation: the context is ``get_context(x)``, as in
        :meth:`sample`) or [M, dx] (the context is the full table, as in :meth:`sample_batched`).
        At most ``max_sampling_batch_size`` query rows go into one sampler call; the calls'
        marginals are combined on the host in fp64, weighted by their draws.  Counters and Philox
        rows advance as in :meth:`sample` / :meth:`sample_batched`.

        The marginals are those of the estimator BEFORE truncation to the prior's support (the
        rejection step of :meth:`sample` is not applied and nothing is reweighted);
        ``support_fraction`` [M] reports the share of the draws inside the support, i.e. one
        minus the estimator's leakage (NaN without a prior).  ``return_samples=True`` keeps the
        draws as ``samples`` [M, num_draws, d_theta].  Results live on the sampler's device."""
        x = self._validate_x(self._embed(x) if self.embedding_net else x)
        num_draws, cap = int(num_draws), int(max_sampling_batch_size)
        n_obs = x.shape[0]
        if num_draws < 1 or cap < 1:
            raise ValueError(f"marginals: num_draws ({num_draws}) and max_sampling_batch_size ({cap}) must be >= 1")
        if n_obs == 1:
            theta_ctx, x_ctx = self.get_context(x)
        else:
            theta_ctx, x_ctx = self._theta_train, self._x_train
        per_call = max(1, cap // n_obs)
        acc = borders = counts = None
        draws = []
        done = 0
        with self._reuse_fits():
            while done < num_draws:
                d = min(per_call, num_draws - done)
                # an observation shard of a larger batch draws at the unsharded batch's Philox rows
                rb = self._obs_offset * d if n_obs > 1 else 0
                if hasattr(self._model, "ar_marginals"):
                    th, _, probs, bd = self._model.ar_marginals(x_ctx, theta_ctx, x, n_obs * d, row_base=rb)
                else:
                    th, probs, bd = self._marginals_generic(x_ctx, theta_ctx, x, d)
                part = probs.to(torch.float64) * d
                acc = part if acc is None else acc + part
                borders = bd if borders is None else borders
                if self.prior is not None:
                    ok = self._within_support(th).reshape(n_obs, d).sum(1)
                    counts = ok if counts is None else counts + ok.to(counts.device)
                if return_samples:
                    draws.append(th.reshape(n_obs, d, -1))
                done += d
        probs = (acc / num_draws).to(torch.float32)
        frac = None if counts is None else counts.to(device=probs.device, dtype=torch.float64) / num_draws
        return PosteriorMarginals(probs, borders, num_draws, frac,
                                  engine=self._model.engine if self._fused() and probs.is_cuda else None,
                                  samples=torch.cat(draws, 1) if return_samples else None)

    def _marginals_generic(self, x_ctx: Tensor, theta_ctx: Tensor, x: Tensor, per: int):
        """:meth:`_ar_generic` over ``x`` repeated obs-major ``per`` times, with every step's
        predictive masses (softmax of the full logits, fp64) averaged over each observation's
        rows: (theta [M * per, d_theta], probs [M, d_theta, n_bars] fp64, borders [d_theta, n_bars + 1])."""
        joint = torch.cat([x_ctx, theta_ctx], dim=1)
        dx = x_ctx.shape[1]
        n_obs = x.shape[0]
        feats = x.repeat_interleave(per, dim=0)
        probs, borders = [], []
        for k in range(theta_ctx.shape[1]):
            self._model.fit(joint[:, : dx + k], joint[:, dx + k])
            pred = self._model.predict(feats, output_type="full", quantiles=[])
            draw = pred["criterion"].sample(pred["logits"])
            p = torch.softmax(torch.as_tensor(pred["logits"]).to(torch.float64), dim=-1)
            probs.append(p.reshape(n_obs, per, -1).mean(1))
            borders.append(torch.as_tensor(pred["criterion"].borders).to(p.device))
            feats = torch.cat([feats, draw[:, None].to(feats.device)], dim=1)
        return feats[:, dx:], torch.stack(probs, 1), torch.stack(borders, 0)

    def pair_marginals(self, x: Tensor, num_draws: int = 10_000, bins: int = 64, limits=None,
                       max_sampling_batch_size: int = 10_000, return_samples: bool = False) -> PosteriorPairMarginals:
        """2-D posterior marginals of every pair of parameters on a grid of ``bins`` x ``bins`` cells
        (what a corner plot draws), folded from the conditionals of ``num_draws`` sampler draws per
        observation: for a pair (j, k), j < k, the earlier parameter enters through the draw's
        cell, the later one through the cell masses of the full predictive distribution theta_k
        was drawn from ("half Rao-Blackwellised"; no extra forward pass).  See
        :mod:`npe_pfn.pair_marginals`.

        ``x``, the contexts, ``max_sampling_batch_size``, counters and Philox rows are those of
        :meth:`marginals`; the calls' tables are combined on the host in fp64, weighted by their
        draws.  ``limits`` [d_theta, 2] are the outer edges of the grid: by default the box prior's
        bounds when the prior is a box, else the per-dimension min / max of the call's context
        thetas.  The edges are ``lo + (hi - lo) * c / bins`` in fp64 rounded to fp32, the last one
        exactly ``hi``; ValueError for a degenerate or non-finite limit or ``bins`` outside 2..128.
        Mass outside the limits is not in the tables (``mass_inside``); nothing is truncated to
        the prior's support or reweighted.  ``return_samples=True`` keeps the draws as ``samples``
        [M, num_draws, d_theta].  Results live on the sampler's device."""
        x = self._validate_x(self._embed(x) if self.embedding_net else x)
        num_draws, cap = int(num_draws), int(max_sampling_batch_size)
        n_obs = x.shape[0]
        if num_draws < 1 or cap < 1:
            raise ValueError(f"pair_marginals: num_draws ({num_draws}) and max_sampling_batch_size ({cap}) must be "
                             ">= 1")
        if n_obs == 1:
            theta_ctx, x_ctx = self.get_context(x)
        else:
            theta_ctx, x_ctx = self._theta_train, self._x_train
        d = theta_ctx.shape[1]
        if limits is None:
            bounds = _box_bounds(self.prior) if self.prior is not None else None
            if bounds is not None:
                limits = torch.stack([bounds[0].detach().reshape(-1), bounds[1].detach().reshape(-1)], 1)
            else:
                limits = torch.stack([theta_ctx.min(0).values, theta_ctx.max(0).values], 1)
        limits = torch.as_tensor(limits)
        if tuple(limits.shape) != (d, 2):
            raise ValueError(f"pair_marginals: limits must be [{d}, 2], got {tuple(limits.shape)}")
        edges = grid_edges(limits.cpu(), bins).to(x.device)
        per_call = max(1, min(cap // n_obs, PAIR_MAX_PER))
        acc_pair = acc_cell = None
        draws = []
        done = 0
        with self._reuse_fits():
            while done < num_draws:
                n = min(per_call, num_draws - done)
                # an observation shard of a larger batch draws at the unsharded batch's Philox rows
                rb = self._obs_offset * n if n_obs > 1 else 0
                if hasattr(self._model, "ar_pair_marginals"):
                    th, _, pair, cell = self._model.ar_pair_marginals(x_ctx, theta_ctx, x, n_obs * n, edges,
                                                                      row_base=rb)
                else:
                    th, pair, cell = self._pair_marginals_generic(x_ctx, theta_ctx, x, n, edges)
                pair, cell = pair.to(torch.float64) * n, cell.to(torch.float64) * n
                acc_pair = pair if acc_pair is None else acc_pair + pair
                acc_cell = cell if acc_cell is None else acc_cell + cell
                if return_samples:
                    draws.append(th.reshape(n_obs, n, -1))
                done += n
        return PosteriorPairMarginals((acc_pair / num_draws).to(torch.float32), (acc_cell / num_draws).to(torch.float32),
                                      edges.to(acc_pair.device), num_draws,
                                      samples=torch.cat(draws, 1) if return_samples else None)

    def _pair_marginals_generic(self, x_ctx: Tensor, theta_ctx: Tensor, x: Tensor, per: int, edges: Tensor):
        """:meth:`_ar_generic` over ``x`` repeated obs-major ``per`` times, with every step's
        predictive distributions (fp64 softmax of the full logits) re-binned onto ``edges`` --
        cell masses from :func:`npe_pfn.diagnostics.bar_cdf` differences -- and folded by
        :func:`pair_accumulate_host`: (theta [M * per, d_theta], pair [M, n_pairs, G, G], cell [M,
        d_theta, G]), the tables fp32 as the engine's."""
        joint = torch.cat([x_ctx, theta_ctx], dim=1)
        dx, d = x_ctx.shape[1], theta_ctx.shape[1]
        n_obs, G = x.shape[0], edges.shape[1] - 1
        feats = x.repeat_interleave(per, dim=0)
        pairs, cells = [], []
        for k in range(d):
            self._model.fit(joint[:, : dx + k], joint[:, dx + k])
            pred = self._model.predict(feats, output_type="full", quantiles=[])
            draw = pred["criterion"].sample(pred["logits"])
            logits = torch.as_tensor(pred["logits"])
            dev = logits.device
            ones = torch.ones(logits.shape[0], dtype=torch.float64, device=dev)
            F = torch.stack([bar_cdf(logits, pred["criterion"].borders, ones * float(e)) for e in edges[k].tolist()], 1)
            w = (F[:, 1:] - F[:, :-1]).clamp(min=0.0)
            pairQ = torch.zeros((n_obs, k, G, G), dtype=torch.int64, device=dev)
            cellQ = torch.zeros((n_obs, G), dtype=torch.int64, device=dev)
            bad = torch.zeros(n_obs, dtype=torch.int32, device=dev)
            pair_accumulate_host(w, feats[:, dx:] if k else None, edges[:k] if k else None, 0, per, pairQ, cellQ, bad)
            if k:
                pairs.append(tables_from_sums(pairQ, bad, per))
            cells.append(tables_from_sums(cellQ, bad, per))
            feats = torch.cat([feats, draw[:, None].to(feats.device)], dim=1)
        dev = cells[0].device
        pair = torch.cat(pairs, 1) if pairs else torch.zeros((n_obs, 0, G, G), dtype=torch.float32, device=dev)
        return feats[:, dx:], pair, torch.stack(cells, 1)

    def _score_batched(self, theta: Tensor, x: Tensor, eps: float, want_logp: bool, want_cdf: bool):
        """(summed log density [...], per-step log densities [..., d_theta], PIT [..., d_theta]) of
        one teacher-forced pass over the full table; entries not asked for are None."""
        x = self._validate_x(self._embed(x) if self.embedding_net else x)
        theta = torch.as_tensor(theta)
        if theta.ndim not in (2, 3):
            raise ValueError(f"theta must be [M, d_theta] or [M, K, d_theta], got shape {tuple(theta.shape)}")
        n_obs, dth = x.shape[0], self._theta_train.shape[1]
        if theta.shape[0] != n_obs:
            raise ValueError(f"theta has {theta.shape[0]} observations, x has {n_obs}")
        if theta.shape[-1] != dth:
            raise ValueError(f"theta has {theta.shape[-1]} dimensions, the training data {dth}")
        lead = theta.shape[:-1]
        flat = theta.reshape(-1, dth)
        with self._reuse_fits():
            if hasattr(self._model, "ar_score"):
                steps, pit = self._model.ar_score(self._x_train, self._theta_train, x, flat, eps=eps,
                                                  want_logp=want_logp, want_cdf=want_cdf)
            else:
                x_query = x if theta.ndim == 2 else x.repeat_interleave(theta.shape[1], dim=0)
                steps, pit = self._score_generic(x_query, flat, eps, want_logp, want_cdf)
        lp = None
        if want_logp:
            lp = torch.zeros(flat.shape[0], dtype=steps.dtype, device=steps.device)
            for k in range(dth):   # in order: the engine's own summation of ar_log_prob
                lp += steps[:, k]
            lp = lp.reshape(lead).to(x.device)
            steps = steps.reshape(*lead, dth).to(x.device)
        if want_cdf:
            pit = pit.reshape(*lead, dth).to(x.device)
        return lp, steps, pit

    def _score_generic(self, x_query: Tensor, theta: Tensor, eps: float, want_logp: bool, want_cdf: bool):
        """The dimension loop of :meth:`_autoregressive_log_prob` through the tabpfn surface, with
        every step's log density and CDF (:func:`npe_pfn.diagnostics.bar_cdf`) kept."""
        joint = torch.cat([self._x_train, self._theta_train], dim=1)
        test = torch.cat([x_query, theta], dim=1)
        dx = self._x_train.shape[1]
        steps, pit = [], []
        for k in range(theta.shape[1]):
            self._model.fit(joint[:, : dx + k], joint[:, dx + k])
            pred = self._model.predict(test[:, : dx + k], output_type="full", quantiles=[])
            if want_logp:
                step = -pred["criterion"](pred["logits"], test[:, dx + k])
                steps.append(torch.where(step == float("-inf"), torch.log(torch.tensor(eps)).to(step), step))
            if want_cdf:
                pit.append(bar_cdf(pred["logits"], pred["criterion"].borders, test[:, dx + k]))
        return (torch.stack(steps, 1) if want_logp else None), (torch.stack(pit, 1) if want_cdf else None)

    def _autoregressive_log_prob(self, theta: Tensor, x: Tensor = None, repeat_x: bool = True,
                                 eps: float = 1e-15) -> Tensor:
        """Teacher-forced sum of per-dimension log densities (reference :462-524)."""
        n = theta.shape[0]
        x_query = x.repeat(n, 1) if repeat_x else x
        assert x_query.shape[0] == n
        theta_ctx, x_ctx = self.get_context(x)
        if hasattr(self._model, "ar_log_prob"):
            x_unique = x if repeat_x and x.shape[0] == 1 else None  # one observation: every query row is x
            return self._model.ar_log_prob(x_ctx, theta_ctx, x_query, theta, eps=eps, x_unique=x_unique)
        joint = torch.cat([x_ctx, theta_ctx], dim=1)
        test = torch.cat([x_query, theta], dim=1)
        dx = x_ctx.shape[1]
        lp = torch.zeros(n)
        for k in range(theta_ctx.shape[1]):
            self._model.fit(joint[:, : dx + k], joint[:, dx + k])
            pred = self._model.predict(test[:, : dx + k], output_type="full", quantiles=[])
            step = -pred["criterion"](pred["logits"], test[:, dx + k])
            step = torch.where(step == float("-inf"), torch.log(torch.tensor(eps)), step)
            lp += step
        return lp

    def _ratio_based_log_prob(self, theta: Tensor, x: Tensor = None, num_posterior_samples: int = 5000,
                              boundary_padding: float = 0.1, reuse_estimator_if_possible: bool = True,
                              eps: float = 1e-15) -> Tensor:
        """Classifier-based density ratio (reference :526-570) -- needs the classifier engine."""
        if self._model_classifier is None:
            self._model_classifier = DensityRatioWrapper(**self.classifier_init_kwargs)
        theta_ctx, x_ctx = self.get_context(x)
        if not reuse_estimator_if_possible or self._model_classifier.refit_necessary(
                x, x_ctx, theta_ctx, num_posterior_samples, boundary_padding):
            post = self.sample(sample_shape=torch.Size([num_posterior_samples]), x=x)
            self._model_classifier.fit(x, post, boundary_padding, x_ctx, theta_ctx)
        return self._model_classifier.ratio_log_probs(theta, eps)

    def _get_classifier_bounds(self):
        if self._model_classifier is None:
            return None, None
        return self._model_classifier._padded_dim_min, self._model_classifier._padded_dim_max

    def _within_support(self, theta: Tensor) -> Tensor:
        """Prior-support mask (reference :581-600).

        On the GPU a box prior (BoxUniform / Independent(Uniform)) is checked by
        the K9 kernel ``npfn_box_support``; any other prior is evaluated by torch
        on the prior's own device.
        """
        if theta.is_cuda and self._fused():
            bounds = _box_bounds(self.prior)
            if bounds is not None:
                return self._model.engine.box_support(theta, bounds[0], bounds[1])
        try:
            return self._support_mask(theta).to(theta.device)
        except RuntimeError:
            # parameters of the prior live on another device (e.g. a CPU box prior)
            prior_dev = _distribution_device(self.prior)
            return self._support_mask(theta.to(prior_dev)).to(theta.device)

    def _support_mask(self, th: Tensor) -> Tensor:
        try:
            chk = self.prior.support.check(th)
            if chk.shape == th.shape:
                chk = torch.all(chk, dim=-1)
            return chk
        except (NotImplementedError, AttributeError):
            return torch.isfinite(self.prior.log_prob(th))


def _distribution_device(dist) -> Optional[torch.device]:
    base = dist
    while hasattr(base, "base_dist"):
        base = base.base_dist
    for name in ("loc", "low", "scale", "high", "probs", "logits", "covariance_matrix"):
        t = getattr(base, name, None)
        if isinstance(t, Tensor):
            return t.device
    return None


def _box_bounds(prior) -> Optional[Tuple[Tensor, Tensor]]:
    """(low, high) if the prior is a box uniform, else None."""
    base = prior
    if isinstance(base, torch.distributions.Independent):
        base = base.base_dist
    if isinstance(base, torch.distributions.Uniform):
        return base.low.reshape(-1), base.high.reshape(-1)
    return None


class DensityRatioWrapper:
    """Ratio-based log density q(θ|x) ∝ U_box(θ) · p(post|θ) / p(unif|θ) (reference :603-704).

    ``fit`` draws as many uniform samples on the padded bounding box of the
    posterior samples as there are posterior samples and trains the engine
    classifier (``TabPFNClassifier``, label 0 = uniform, 1 = posterior);
    ``ratio_log_probs`` = log U + log(p1 + eps) - log(p0 + eps) inside the box and
    log U + log eps - log(1 + eps) outside it.  The classifier is reused while
    x, the context and the settings are unchanged (``refit_necessary``).  All
    tensors stay on the device of the posterior samples.
    """

    def __init__(self, **init_kwargs):
        self._classifier = TabPFNClassifier(**init_kwargs)
        self._ratio_log_prob_x = None
        self._num_posterior_samples = None
        self._boundary_padding = None
        self._padded_dim_min = None
        self._padded_dim_max = None
        self._uniform_log_prob = None

    def fit(self, x: Tensor, posterior_samples: Tensor, boundary_padding: float, x_context: Tensor,
            theta_context: Tensor) -> None:
        lo = posterior_samples.min(dim=0).values
        hi = posterior_samples.max(dim=0).values
        span = hi - lo
        pad_lo = lo - boundary_padding * span
        pad_hi = hi + boundary_padding * span
        pad_span = pad_hi - pad_lo
        uniform_log_prob = -torch.log(pad_span).sum()
        uniform = torch.rand_like(posterior_samples) * pad_span + pad_lo
        n = posterior_samples.shape[0]
        X = torch.cat([uniform, posterior_samples], dim=0)
        y = torch.cat([torch.zeros(n), torch.ones(n)], dim=0)
        self._ratio_log_prob_x = x
        self._num_posterior_samples = n
        self._boundary_padding = boundary_padding
        self._x_context = x_context
        self._theta_context = theta_context
        self._padded_dim_min = pad_lo
        self._padded_dim_max = pad_hi
        self._uniform_log_prob = uniform_log_prob
        self._classifier.fit(X, y)

    def refit_necessary(self, x: Tensor, x_context: Tensor, theta_context: Tensor, num_posterior_samples: int,
                        boundary_padding: float) -> bool:
        if self._ratio_log_prob_x is None:
            return True
        return not (torch.allclose(x, self._ratio_log_prob_x)
                    and x_context.shape == self._x_context.shape and torch.allclose(x_context, self._x_context)
                    and theta_context.shape == self._theta_context.shape
                    and torch.allclose(theta_context, self._theta_context)
                    and num_posterior_samples == self._num_posterior_samples
                    and math.isclose(boundary_padding, self._boundary_padding))

    def _proba(self, theta: Tensor) -> Tensor:
        clf = self._classifier
        if hasattr(clf, "predict_proba_tensor"):
            return clf.predict_proba_tensor(theta).to(theta.device)
        return torch.as_tensor(clf.predict_proba(theta)).to(theta.device)  # numpy, as tabpfn returns it

    def ratio_log_probs(self, theta: Tensor, eps: float = 1e-15) -> Tensor:
        lo = self._padded_dim_min.to(theta.device)
        hi = self._padded_dim_max.to(theta.device)
        inside = torch.all((theta >= lo) & (theta <= hi), dim=1)
        ulp = self._uniform_log_prob.to(theta.device)
        outside_val = ulp + torch.log(torch.tensor(eps)).to(theta.device) - torch.log(torch.tensor(1 + eps)).to(theta.device)
        out = outside_val.expand(theta.shape[0]).clone()
        if inside.any():
            p = self._proba(theta[inside])
            out[inside] = ulp + torch.log(p[:, 1] + eps) - torch.log(p[:, 0] + eps)
        return out


class TabPFN_Based_NPE_PFN(NPE_PFN_Core):
    """NPE-PFN whose context is filtered per observation (reference :708-744)."""

    def __init__(
        self,
        show_progress_bars: bool = False,
        prior: Optional[Distribution] = None,
        filter_type: Union[str, Callable] = "standardized_euclidean_filtering",
        filter_context_size: int = 10_000,
        regressor_init_kwargs: Mapping = {},
        classifier_init_kwargs: Mapping = {},
        embedding_net: Optional[torch.nn.Module] = None,
        x_shape: Optional[torch.Size] = None,
    ):
        super().__init__(show_progress_bars, prior, regressor_init_kwargs=regressor_init_kwargs,
                         classifier_init_kwargs=classifier_init_kwargs, embedding_net=embedding_net,
                         x_shape=x_shape)
        self.filter = get_filtering_method(filter_type)
        self.filter_context_size = filter_context_size

    def _context_is_deterministic(self) -> bool:
        # random_filtering draws a new randperm subset per call; a user callable is unknown
        return self.filter in DETERMINISTIC_FILTERS

    def get_context(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        x = self._validate_x(x)
        return self.filter(x, self._theta_train, self._x_train, self.filter_context_size)


class TabPFN_Based_Uncond_Estimator(NPE_PFN_Core):
    """Unconditional density estimator of theta (reference :747-900, "experimental" there).

    The thetas are clustered by k-means (``num_clusters=1``: no clustering) and each cluster is
    modelled by the autoregressive TabPFN sampler on a dummy one-column x ~ N(0, 1); the mixture
    weights are the cluster sizes.  The clustering is the seeded k-means of :mod:`npe_pfn.kmeans`
    (K13: on the device with the engine-backed regressor, in numpy with any other estimator)
    instead of the reference's host-side sklearn ``KMeans``; its seed is
    ``regressor_init_kwargs["random_state"]``.  Every host draw (``randperm``, ``randn``,
    ``multinomial``) comes from the CPU generators in the reference's order, so one
    ``torch.manual_seed`` / ``np.random.seed`` gives the same stream with every estimator.
    """

    def __init__(
        self,
        num_clusters: int = 1,
        show_progress_bars: bool = False,
        regressor_init_kwargs: Mapping = {},
        classifier_init_kwargs: Mapping = {},
    ):
        super().__init__(show_progress_bars, prior=None, regressor_init_kwargs=regressor_init_kwargs,
                         classifier_init_kwargs=classifier_init_kwargs)
        self.context_size = 10_000  # rows of a cluster beyond this are cut off (reference :764-765)
        self.num_clusters = num_clusters
        self.cluster_state = 0
        self.kmeans: Optional[KMeansState] = None
        self.counts = None

    def set_cluster_state(self, cluster_idx: int = 0):
        self.cluster_state = cluster_idx

    def _kmeans_engine(self):
        """The engine that clusters on the device; None with a generic estimator (host k-means)."""
        return self._model.engine if self._fused() else None

    def get_context(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        """The current cluster's first ``context_size`` rows (reference :774-781)."""
        member = self.kmeans.labels_ == self.cluster_state
        return self._theta_train[member][: self.context_size], self._x_train[member][: self.context_size]

    def append_simulations(self, theta: Tensor, x: Tensor = None):
        """Replace the training thetas (``x`` is ignored) and cluster them (reference :783-800)."""
        self._theta_train = None
        self._x_train = None
        theta = self._validate_theta(theta)
        if not bool(torch.isfinite(theta).all()):
            raise ValueError("append_simulations: theta has non-finite entries (k-means needs finite thetas)")
        n = theta.shape[0]
        # permuted because only the first context_size rows of a cluster reach the context
        self._theta_train = theta[torch.randperm(n).to(theta.device)]
        self._x_train = torch.randn(n, 1).to(theta.device)
        seed = self.regressor_init_kwargs.get("random_state", 0)
        self.kmeans = KMeansState(self.num_clusters, seed=0 if seed is None else int(seed))
        self.kmeans.fit(self._theta_train, engine=self._kmeans_engine())
        counts = self.kmeans.counts.numpy()
        assert counts.min() > 1, "Too few samples in some clusters, need at least 2."
        self.counts = counts
        self._size_fit_cache()
        return self

    # share of the device's free memory the clusters' cached fits may hold
    FIT_CACHE_FREE_FRACTION = 0.5

    def _size_fit_cache(self):
        """One cached set of per-step fits per cluster (TabPFNRegressor.size_fit_cache): from the
        second ``sample`` / ``log_prob`` on no cluster is refitted.  The sets may hold at most
        ``FIT_CACHE_FREE_FRACTION`` of the memory that is free on the device when the limit is
        applied (after clustering; after unpickling, when the engine is rebuilt) -- the rest stays
        for the forwards' workspaces and the caller; past the limit the engine frees the least
        recently used clusters' fits and refits them when they come round again.
        ``regressor_init_kwargs["fit_cache_sets"] = 0`` is honoured: the cache stays off and every
        call refits, as the reference does."""
        if not self._fused() or self._model.fit_cache_sets == 0:
            return
        self._model.size_fit_cache(max(int(self.num_clusters), 1), self.FIT_CACHE_FREE_FRACTION)

    def __setstate__(self, state):
        super().__setstate__(state)   # a new regressor without an engine
        if self.kmeans is not None:
            self._size_fit_cache()    # recorded on the regressor, applied when its engine is built

    def sample(self, sample_shape: torch.Size = torch.Size(), x: Tensor = None, max_sampling_batch_size: int = 10_000,
               with_log_prob: bool = False, eps: float = 1e-15) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """``sample_shape[0]`` draws of the mixture (reference :802-844); ``x`` is ignored.

        Every cluster visit runs under its own fit token; the engine's fit cache holds one set of
        fits per cluster (:meth:`_size_fit_cache`), found again by the cluster's context."""
        per_cluster = np.random.multinomial(sample_shape[0], self.counts / self.counts.sum())
        draws, lps = [], []
        for c, m in enumerate(per_cluster):
            self.set_cluster_state(c)
            if m == 0:
                continue
            with self._reuse_fits():
                th, lp = self._sample(max_sampling_batch_size, torch.randn(int(m), 1), repeat_x=False,
                                      with_log_prob=with_log_prob, eps=eps)
            draws.append(th)
            lps.append(lp)
        self.set_cluster_state()
        out_device = self._theta_train.device
        samples = torch.cat(draws, dim=0)
        perm = torch.randperm(samples.shape[0])
        samples = samples[perm.to(samples.device)].to(out_device)
        if with_log_prob:
            log_probs = torch.cat(lps, dim=0)
            return samples, log_probs[perm.to(log_probs.device)].to(out_device)
        return samples

    def log_prob_batched(self, theta: Tensor, x: Tensor = None, eps: float = 1e-15, return_steps: bool = False):
        """Not provided: this estimator's ``x`` is a dummy column, so there are no (theta, x) pairs
        to score together; use :meth:`log_prob`."""
        raise NotImplementedError("TabPFN_Based_Uncond_Estimator has no observations to batch over (its x is a "
                                  "dummy column); use log_prob(theta)")

    def marginals(self, x: Tensor = None, num_draws: int = 10_000, max_sampling_batch_size: int = 10_000,
                  return_samples: bool = False):
        """Not provided: every cluster is fitted on its own context and so has its own bar borders;
        the mixture's marginal is not a column average on one grid."""
        raise NotImplementedError("TabPFN_Based_Uncond_Estimator.marginals: the clusters' bar borders differ, so "
                                  "their mixtures do not average on one grid")

    def pair_marginals(self, num_draws: int = 10_000, bins: int = 64, limits=None,
                       max_sampling_batch_size: int = 10_000, return_samples: bool = False) -> PosteriorPairMarginals:
        """2-D marginals of the mixture (:meth:`NPE_PFN_Core.pair_marginals`): every cluster folds
        ``num_draws`` draws of its own sampler -- on its own context, given one dummy x ~ N(0, 1)
        -- onto the SAME cell edges, and the clusters' tables are mixed with the weights ``counts_c
        / n`` in fp64.  The clusters' bar borders differ, but a common coarse grid does not care.
        ``limits`` default to the per-dimension min / max of all training thetas.  ``samples``
        (when asked for) are [1, num_clusters * num_draws, d_theta], cluster after cluster (NOT
        draws of the mixture: every cluster contributes ``num_draws``)."""
        if limits is None:
            limits = torch.stack([self._theta_train.min(0).values, self._theta_train.max(0).values], 1)
        weights = self.counts / self.counts.sum()
        pair = cell = edges = None
        draws = []
        try:
            for c in range(self.num_clusters):
                self.set_cluster_state(c)
                pm = super().pair_marginals(torch.randn(1, 1).to(self._theta_train.device), num_draws, bins, limits,
                                            max_sampling_batch_size, return_samples)
                wp, wc = pm.probs.to(torch.float64) * float(weights[c]), pm.marginal_probs.to(torch.float64) * float(weights[c])
                pair = wp if pair is None else pair + wp
                cell = wc if cell is None else cell + wc
                edges = pm.edges
                draws.append(pm.samples)
        finally:
            self.set_cluster_state()
        return PosteriorPairMarginals(pair.to(torch.float32), cell.to(torch.float32), edges, int(num_draws),
                                      samples=torch.cat(draws, 1) if return_samples else None)

    def pit_batched(self, theta: Tensor, x: Tensor = None) -> Tensor:
        """Not provided, for the reason given at :meth:`log_prob_batched`."""
        raise NotImplementedError("TabPFN_Based_Uncond_Estimator has no observations to batch over (its x is a "
                                  "dummy column)")

    def coverage_batched(self, theta_true: Tensor, x: Tensor = None, *args, **kwargs):
        """Not provided, for the reason given at :meth:`log_prob_batched`."""
        raise NotImplementedError("TabPFN_Based_Uncond_Estimator has no observations to batch over (its x is a "
                                  "dummy column); use log_prob(theta)")

    def mmd_batched(self, theta_ref: Tensor, x: Tensor = None, *args, **kwargs):
        """Not provided, for the reason given at :meth:`log_prob_batched`; compare draws of
        :meth:`sample` with :func:`npe_pfn.diagnostics.mmd_batched`."""
        raise NotImplementedError("TabPFN_Based_Uncond_Estimator has no observations to batch over (its x is a "
                                  "dummy column); call npe_pfn.diagnostics.mmd_batched on sample()'s draws")

    def wasserstein_batched(self, theta_ref: Tensor, x: Tensor = None, *args, **kwargs):
        """Not provided, for the reason given at :meth:`log_prob_batched`; compare draws of
        :meth:`sample` with :func:`npe_pfn.diagnostics.wasserstein_batched`."""
        raise NotImplementedError("TabPFN_Based_Uncond_Estimator has no observations to batch over (its x is a "
                                  "dummy column); call npe_pfn.diagnostics.wasserstein_batched on sample()'s draws")

    def c2st_batched(self, theta_ref: Tensor, x: Tensor = None, *args, **kwargs):
        """Not provided, for the reason given at :meth:`log_prob_batched`; compare draws of
        :meth:`sample` with :func:`npe_pfn.diagnostics.c2st_batched`."""
        raise NotImplementedError("TabPFN_Based_Uncond_Estimator has no observations to batch over (its x is a "
                                  "dummy column); call npe_pfn.diagnostics.c2st_batched on sample()'s draws")

    def log_prob(self, theta: Tensor, x: Tensor = None, max_sampling_batch_size: int = 10_000,
                 mode: str = "autoregressive", eps: float = 1e-15, **ratio_kwargs) -> Tensor:
        """log of the mixture's component density at theta's own cluster plus the log cluster
        weight (reference :846-900); ``x`` is ignored.  Every cluster visit takes a fresh fit
        token around its chunks: a token kept across clusters would let two clusters of equal
        size reuse each other's fits.  Under a fresh token the engine's fit cache finds the
        cluster's fits by the content of its context (:meth:`_size_fit_cache`)."""
        if mode == "ratio_based":
            raise NotImplementedError(
                "TabPFN_Based_Uncond_Estimator.log_prob: mode='ratio_based' is not provided (the reference's "
                "version draws from the whole mixture inside the per-cluster loop and adds the cluster weight "
                "twice); use mode='autoregressive'")
        if mode != "autoregressive":
            raise ValueError(f"Invalid mode: {mode}")
        theta = self._validate_theta(theta)
        labels = self.kmeans.predict(theta, engine=self._kmeans_engine())
        log_weights = np.log(self.counts / self.counts.sum())
        out = torch.zeros(theta.shape[0])
        for c in range(self.num_clusters):
            self.set_cluster_state(c)
            rows = (labels == c).nonzero(as_tuple=True)[0]
            if rows.numel() == 0:
                continue
            members = theta[rows]
            lp = torch.zeros(members.shape[0])
            with self._reuse_fits():
                for i in range(0, members.shape[0], max_sampling_batch_size):
                    chunk = members[i: i + max_sampling_batch_size]
                    lp[i: i + max_sampling_batch_size] = self._autoregressive_log_prob(
                        chunk, torch.randn(chunk.shape[0], 1), repeat_x=False, eps=eps).cpu()
            out[rows.cpu()] = lp + float(log_weights[c])
        self.set_cluster_state()
        return out
