"""NPE_PFN_RestrictedPrior (reference: npe_pfn/restricted_prior.py:8-97).

The prior restricted to the region where the simulator works: the user labels every
simulated theta as valid (1) or invalid (0), a TabPFN classifier learns the valid region,
and the prior is sampled by rejection against
``classifier.predict_proba(theta)[:, -1] > acceptance_threshold`` (reference :25-28).

The reference inherits the sampling loop and ``log_prob`` from ``sbi.utils.RestrictedPrior``;
this class is a plain ``torch.distributions.Distribution`` with the same surface and does not
import ``sbi``.  Differences from the reference, on purpose ("Restricted prior"):

* with a box prior and the engine classifier a rejection round runs on the device
  (``Engine.restricted_box_round``): proposals from the Philox row stream, the classifier
  forward, the accept decision and the ordered append, with one 16-byte readback per round.
  The result is *the first n accepted rows of the row stream*, so it does not depend on the
  batch schedule;
* ``append_simulations`` subsamples every class without replacement (the reference's top-up
  of the larger class from a second permutation can repeat rows);
* more than ``max_iter_rejection`` rounds raise instead of looping on.
"""

from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor
from torch.distributions import Distribution

from .accept_reject_sampler import accept_reject_sample
from .npe_pfn import _box_bounds
from .tabpfn import TabPFNClassifier


def kept_counts(n0: int, n1: int, max_context_rows: int) -> Tuple[int, int]:
    """Rows of class 0 / class 1 that ``append_simulations`` keeps for the classifier fit.

    With H = max_context_rows // 2 each class keeps at most H rows, except that a class may
    fill the room the other one leaves below H (reference :61-85) -- as far as it has distinct
    rows for it."""
    half = max_context_rows // 2
    b0, b1 = min(n0, half), min(n1, half)
    c0 = min(n0, max_context_rows - b1) if n1 < half else b0
    c1 = min(n1, max_context_rows - b0) if n0 < half else b1
    return c0, c1


def _subsample(rows: Tensor, count: int) -> Tensor:
    """``count`` distinct rows in the order of one ``torch.randperm``; all rows, in their own
    order, when none has to go."""
    if count >= rows.shape[0]:
        return rows
    return rows[torch.randperm(rows.shape[0])[:count]]


class NPE_PFN_RestrictedPrior(Distribution):
    """``prior`` restricted to where the classifier's last class ("valid") has probability
    above ``acceptance_threshold``.

    ``classifier`` is a plain attribute (this package's ``TabPFNClassifier(**kwargs)``): any
    object with ``fit(X, y)`` and ``predict_proba(X) -> [N, n_classes]`` can replace it.
    """

    arg_constraints: Dict = {}

    def __init__(self, prior, acceptance_threshold: float = 0.3, tabpfn_classifier_kwargs: Optional[dict] = None,
                 max_context_rows: int = 10_000):
        if int(max_context_rows) < 2:
            raise ValueError(f"max_context_rows must be at least 2, got {max_context_rows}")
        super().__init__(batch_shape=prior.batch_shape, event_shape=prior.event_shape, validate_args=False)
        self.prior = prior
        self.acceptance_threshold = float(acceptance_threshold)
        self.max_context_rows = int(max_context_rows)
        self.classifier = TabPFNClassifier(**(tabpfn_classifier_kwargs or {}))
        self.thetas = torch.tensor([])
        self.y_labels = torch.tensor([])
        self.acceptance_rate: Optional[float] = None
        self.sample_counter = 0  # Philox counter of the next sample() call (dim counters per call)
        self._fitted = False

    @property
    def support(self):
        return self.prior.support

    # ------------------------------------------------------------------ training
    def append_simulations(self, theta, y_label):
        """Adds labelled simulations (1 = valid, 0 = invalid) and refits the classifier on at
        most ``max_context_rows`` of all of them, class 0 first (reference :41-97)."""
        theta = torch.as_tensor(theta).detach().cpu().to(torch.float32)
        y_label = torch.as_tensor(y_label).detach().cpu().reshape(-1).to(torch.float32)
        if theta.ndim != 2 or theta.shape[0] != y_label.shape[0]:
            raise ValueError(f"append_simulations: theta {tuple(theta.shape)} and y_label {tuple(y_label.shape)} "
                             "do not match")
        self.thetas = torch.cat([self.thetas, theta], dim=0) if self.thetas.numel() else theta
        self.y_labels = torch.cat([self.y_labels, y_label], dim=0) if self.y_labels.numel() else y_label
        class0 = self.thetas[self.y_labels == 0]
        class1 = self.thetas[self.y_labels == 1]
        c0, c1 = kept_counts(class0.shape[0], class1.shape[0], self.max_context_rows)
        class0 = _subsample(class0, c0)
        class1 = _subsample(class1, c1)
        self.classifier.fit(torch.cat([class0, class1], dim=0), torch.cat([torch.zeros(c0), torch.ones(c1)], dim=0))
        self._fitted = True
        self.acceptance_rate = None  # belongs to the previous classifier
        return self

    # ------------------------------------------------------------------ accept
    def _engine(self):
        """The classifier's engine when the accept decision can run in it: this package's
        classifier with the probabilities as the engine mixes them (``balance_probabilities``
        reweights them on the host side of the classifier)."""
        clf = self.classifier
        if isinstance(clf, TabPFNClassifier) and not clf.balance_probabilities:
            return clf.engine
        return None

    def _need_fit(self, what: str) -> None:
        if not self._fitted:
            raise RuntimeError(f"NPE_PFN_RestrictedPrior.{what} before append_simulations: the classifier has no fit")

    @torch.no_grad()
    def accept(self, theta) -> Tensor:
        """Bool [N]: ``predict_proba(theta)[:, -1] > acceptance_threshold`` (reference :25-28)."""
        self._need_fit("accept")
        theta = torch.as_tensor(theta, dtype=torch.float32)
        eng = self._engine()
        if eng is not None:
            return eng.predict_accept(theta, self.acceptance_threshold).to(theta.device)
        p = torch.as_tensor(self.classifier.predict_proba(theta))
        return (p[:, -1] > self.acceptance_threshold).to(theta.device)

    # ------------------------------------------------------------------ sample
    @staticmethod
    def _next_batch(remaining: int, accepted: int, proposed: int, max_bs: int) -> int:
        """accept_reject_sampler's schedule (reference accept_reject_sampler.py:68-72)."""
        rate = accepted / proposed
        return min(max_bs, max(int(1.5 * remaining / max(rate, 1e-12)), 100))

    @staticmethod
    def _too_many(max_iter: int, accepted: int, n: int, proposed: int) -> RuntimeError:
        return RuntimeError(f"restricted prior: more than max_iter_rejection={max_iter} rejection rounds: "
                            f"{accepted} of the {n} samples accepted out of {proposed} proposed "
                            "(lower acceptance_threshold or raise max_iter_rejection)")

    def _sample_box_engine(self, eng, bounds, n: int, dim: int, max_bs: int, max_iter: int):
        low, high = eng.box_bounds(bounds[0], bounds[1], dim)
        theta_out = torch.empty((n, dim), dtype=torch.float32, device=eng.device)
        counts = torch.zeros(2, dtype=torch.int64, device=eng.device)
        counter = self.sample_counter
        self.sample_counter += dim
        proposed = accepted = stored = rounds = 0
        batch = min(n, max_bs)
        while stored < n:
            if rounds >= max_iter:
                raise self._too_many(max_iter, accepted, n, proposed)
            eng.restricted_box_round(low, high, self.acceptance_threshold, batch, counter, proposed, theta_out, counts,
                                     seed=self.classifier.random_state)
            rounds += 1
            proposed += batch
            stored, accepted = (int(v) for v in counts.tolist())  # the round's one readback
            batch = self._next_batch(n - stored, accepted, proposed, max_bs)
        return theta_out.to(bounds[0].device), accepted, proposed

    def _sample_generic(self, n: int, max_bs: int, max_iter: int, show_progress_bars: bool):
        tally = {"rounds": 0, "accepted": 0, "proposed": 0}

        def proposal(batch):
            if tally["rounds"] >= max_iter:
                raise self._too_many(max_iter, tally["accepted"], n, tally["proposed"])
            return self.prior.sample((batch,)), None

        def accept(theta):
            mask = self.accept(theta)
            tally["rounds"] += 1
            tally["accepted"] += int(mask.sum())
            tally["proposed"] += int(theta.shape[0])
            return mask

        samples, _, _ = accept_reject_sample(proposal, accept, n, show_progress_bars=show_progress_bars,
                                             max_sampling_batch_size=max_bs)
        return samples, tally["accepted"], tally["proposed"]

    @torch.no_grad()
    def sample(self, sample_shape=torch.Size(), max_sampling_batch_size: int = 10_000,
               save_acceptance_rate: bool = False, max_iter_rejection: int = 1000,
               show_progress_bars: bool = False) -> Tensor:
        """``[*sample_shape, dim]`` draws of the prior that the classifier accepts.

        Box prior and engine classifier: the first n accepted rows of the Philox row stream
        (key = the classifier's ``random_state``, counters ``sample_counter + j``), on the prior's
        device.  Otherwise ``accept_reject_sample`` on ``prior.sample`` and :meth:`accept`."""
        self._need_fit("sample")
        sample_shape = torch.Size(sample_shape)
        n = sample_shape.numel()
        dim = int(self.prior.event_shape[0]) if len(self.prior.event_shape) else 1
        max_bs, max_iter = int(max_sampling_batch_size), int(max_iter_rejection)
        if max_bs < 1:
            raise ValueError(f"max_sampling_batch_size must be positive, got {max_sampling_batch_size}")
        if n == 0:
            return torch.empty((*sample_shape, dim), dtype=torch.float32)
        bounds = _box_bounds(self.prior)
        eng = self._engine() if bounds is not None else None
        if eng is not None:
            samples, accepted, proposed = self._sample_box_engine(eng, bounds, n, dim, max_bs, max_iter)
        else:
            samples, accepted, proposed = self._sample_generic(n, max_bs, max_iter, show_progress_bars)
        if save_acceptance_rate:
            self.acceptance_rate = accepted / proposed
        return samples.reshape(*sample_shape, dim)

    # ------------------------------------------------------------------ log_prob
    @torch.no_grad()
    def log_prob(self, theta, norm_restricted_prior: bool = False,
                 prior_acceptance_params: Optional[dict] = None) -> Tensor:
        """``prior.log_prob(theta)`` where accepted, ``-inf`` elsewhere; with
        ``norm_restricted_prior`` minus ``log(acceptance_rate)``, estimated first by one
        ``sample((max_sampling_batch_size,), save_acceptance_rate=True)`` if none is stored
        (the default False is the reference's, :33)."""
        self._need_fit("log_prob")
        theta = torch.as_tensor(theta, dtype=torch.float32)
        dim = int(self.prior.event_shape[0]) if len(self.prior.event_shape) else 1
        flat = theta.reshape(-1, dim)
        lp = self.prior.log_prob(flat).reshape(-1)
        lp = torch.where(self.accept(flat).to(lp.device), lp, torch.full_like(lp, -math.inf))
        if norm_restricted_prior:
            if self.acceptance_rate is None:
                params = dict(prior_acceptance_params or {})
                self.sample((int(params.get("max_sampling_batch_size", 10_000)),), save_acceptance_rate=True, **params)
            lp = lp - math.log(self.acceptance_rate)
        return lp.reshape(theta.shape[:-1])
