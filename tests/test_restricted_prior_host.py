"""Host logic of NPE_PFN_RestrictedPrior (npe_pfn/restricted_prior.py; reference
restricted_prior.py:8-97) with a stub classifier: the kept counts of ``append_simulations``,
the generic rejection path, ``log_prob``, the iteration cap, pickling -- and the numpy
restatement of the box proposals (tests/restricted_ref.py) at the edge of the box.  No GPU.
"""
import math
import pickle

import numpy as np
import pytest
import torch
from torch.distributions import Independent, MultivariateNormal, Uniform

import restricted_ref as ref

CUT = 0.5  # the stub accepts theta[:, 0] > CUT


class StubClassifier:
    """fit records its arguments; predict_proba is a fixed function of theta: the last class
    has probability 0.9 where theta[:, 0] > cut, else 0.1."""

    def __init__(self, cut=CUT):
        self.cut = cut
        self.fits = []
        self.rows_seen = 0

    def fit(self, X, y):
        y = torch.as_tensor(y)
        if torch.unique(y).numel() < 2:
            raise ValueError("stub: needs two classes")
        self.fits.append((torch.as_tensor(X).clone(), y.clone()))
        return self

    def predict_proba(self, X):
        X = torch.as_tensor(X)
        self.rows_seen += int(X.shape[0])
        p1 = np.where(X[:, 0].cpu().numpy() > self.cut, 0.9, 0.1).astype(np.float32)
        return np.stack([1.0 - p1, p1], axis=1)


def box_prior():
    return Independent(Uniform(-torch.ones(2), torch.ones(2)), 1)


def normal_prior():
    return MultivariateNormal(torch.zeros(2), torch.eye(2))


# fraction of each prior's mass the stub accepts
AREA = {"box": (1.0 - CUT) / 2.0, "normal": 0.5 * math.erfc(CUT / math.sqrt(2.0))}
PRIORS = {"box": box_prior, "normal": normal_prior}


def labelled(n0, n1, seed=0):
    """n0 rows of class 0 (theta[:, 0] < 0) and n1 of class 1 (theta[:, 0] > 0), interleaved."""
    g = torch.Generator().manual_seed(seed)
    th0 = torch.rand(n0, 2, generator=g) * torch.tensor([-1.0, 1.0]) - torch.tensor([1e-3, 0.0])
    th1 = torch.rand(n1, 2, generator=g) + torch.tensor([1e-3, 0.0])
    theta = torch.cat([th0, th1])
    y = torch.cat([torch.zeros(n0), torch.ones(n1)])
    order = torch.randperm(n0 + n1, generator=g)
    return theta[order], y[order]


def make(prior="box", cut=CUT, **kw):
    from npe_pfn import NPE_PFN_RestrictedPrior

    rp = NPE_PFN_RestrictedPrior(PRIORS[prior](), **kw)
    rp.classifier = StubClassifier(cut)
    th, y = labelled(20, 20)
    rp.append_simulations(th, y)
    return rp


def test_class_is_exported():
    import npe_pfn

    assert "NPE_PFN_RestrictedPrior" in npe_pfn.__all__
    assert npe_pfn.NPE_PFN_RestrictedPrior.__mro__[1] is torch.distributions.Distribution
    import sys

    assert "sbi" not in sys.modules


@pytest.mark.parametrize("n0,n1,want", [(5, 5, (5, 5)), (80, 10, (80, 10)), (10, 80, (10, 80)), (80, 80, (50, 50)),
                                        (70, 40, (60, 40)), (51, 3, (51, 3))])
def test_kept_counts_no_duplicates_class_order(n0, n1, want):
    from npe_pfn import NPE_PFN_RestrictedPrior

    assert ref.kept_counts(n0, n1, 100) == want  # the restatement itself, against the stated table
    theta, y = labelled(n0, n1, seed=n0 + n1)
    # two calls with both classes in each: the classifier is refitted on everything so far
    i0, i1 = torch.nonzero(y == 0).reshape(-1), torch.nonzero(y == 1).reshape(-1)
    first = torch.cat([i0[: n0 // 2], i1[: n1 // 2]]).sort().values
    second = torch.cat([i0[n0 // 2:], i1[n1 // 2:]]).sort().values
    fits = []
    for _ in range(2):
        rp = NPE_PFN_RestrictedPrior(box_prior(), max_context_rows=100)
        rp.classifier = StubClassifier()
        torch.manual_seed(11)
        rp.append_simulations(theta[first], y[first])
        rp.append_simulations(theta[second].numpy(), y[second].numpy())
        assert len(rp.classifier.fits) == 2 and rp.thetas.shape == (n0 + n1, 2)
        fits.append(rp.classifier.fits[-1])
    X, yy = fits[0]
    c0, c1 = want
    assert X.shape == (c0 + c1, 2)
    assert torch.equal(yy, torch.cat([torch.zeros(c0), torch.ones(c1)]))  # class 0 first
    assert (X[:c0, 0] < 0).all() and (X[c0:, 0] > 0).all()                # rows of their own class
    assert torch.unique(X, dim=0).shape[0] == c0 + c1                     # no row twice
    pool = {tuple(r) for r in theta.tolist()}
    assert all(tuple(r) in pool for r in X.tolist())
    assert torch.equal(fits[0][0], fits[1][0]) and torch.equal(fits[0][1], fits[1][1])  # torch.manual_seed


def test_subsample_depends_on_the_torch_seed():
    from npe_pfn import NPE_PFN_RestrictedPrior

    theta, y = labelled(80, 80)
    got = []
    for seed in (1, 2):
        rp = NPE_PFN_RestrictedPrior(box_prior(), max_context_rows=100)
        rp.classifier = StubClassifier()
        torch.manual_seed(seed)
        rp.append_simulations(theta, y)
        got.append(rp.classifier.fits[-1][0])
    assert not torch.equal(got[0], got[1])


def test_single_class_error_of_the_classifier_passes_through():
    """(N0, N1) = (200, 0): the package's own classifier refuses a one-class fit before it
    touches an engine; the error is the caller's to see."""
    from npe_pfn import NPE_PFN_RestrictedPrior

    rp = NPE_PFN_RestrictedPrior(box_prior(), max_context_rows=100)
    theta, y = labelled(200, 0)
    with pytest.raises(ValueError, match="two classes"):
        rp.append_simulations(theta, y)
    with pytest.raises(RuntimeError, match="append_simulations"):
        rp.sample((3,))


@pytest.mark.parametrize("prior", ["box", "normal"])
def test_sample_shapes_accepted_and_rate(prior):
    rp = make(prior)
    torch.manual_seed(5)
    for shape in ((), (7,), (3, 4)):
        s = rp.sample(shape)
        assert s.shape == (*shape, 2) and s.dtype == torch.float32
        assert rp.accept(s.reshape(-1, 2)).all()
        assert (s.reshape(-1, 2)[:, 0] > CUT).all()
    assert rp.acceptance_rate is None
    seen = rp.classifier.rows_seen
    s = rp.sample((4000,), max_sampling_batch_size=2000, save_acceptance_rate=True)
    proposed = rp.classifier.rows_seen - seen
    assert s.shape == (4000, 2) and proposed >= 4000
    f = AREA[prior]
    se = math.sqrt(f * (1.0 - f) / proposed)
    assert abs(rp.acceptance_rate - f) <= 4.0 * se, (rp.acceptance_rate, f, se, proposed)


@pytest.mark.parametrize("prior", ["box", "normal"])
def test_log_prob(prior):
    rp = make(prior)
    theta = torch.tensor([[0.9, 0.1], [0.2, -0.3], [0.6, 0.6], [-0.7, 0.0], [0.51, -0.9]])
    inside = theta[:, 0] > CUT
    lp = rp.log_prob(theta)
    assert lp.shape == (5,)
    assert torch.equal(lp[inside], rp.prior.log_prob(theta)[inside])
    assert torch.isneginf(lp[~inside]).all()
    assert rp.log_prob(theta[0]).shape == ()
    # normalised: a stored rate is used as it is ...
    rp.acceptance_rate = 0.25
    lpn = rp.log_prob(theta, norm_restricted_prior=True)
    torch.testing.assert_close(lpn[inside], rp.prior.log_prob(theta)[inside] - math.log(0.25), rtol=0, atol=1e-6)
    assert torch.isneginf(lpn[~inside]).all()
    # ... and estimated by one sample() call when there is none
    rp.acceptance_rate = None
    torch.manual_seed(3)
    lpn = rp.log_prob(theta, norm_restricted_prior=True, prior_acceptance_params={"max_sampling_batch_size": 2000})
    assert rp.acceptance_rate is not None and abs(rp.acceptance_rate - AREA[prior]) < 0.05
    torch.testing.assert_close(lpn[inside], rp.prior.log_prob(theta)[inside] - math.log(rp.acceptance_rate),
                               rtol=0, atol=1e-6)


@pytest.mark.parametrize("prior", ["box", "normal"])
def test_nothing_accepted_raises_after_max_iter(prior):
    rp = make(prior, cut=1e9)
    seen = rp.classifier.rows_seen
    with pytest.raises(RuntimeError, match=r"max_iter_rejection=2.*\b0 of the 10 samples.*110 proposed"):
        rp.sample((10,), max_sampling_batch_size=100, max_iter_rejection=2)
    assert rp.classifier.rows_seen - seen == 10 + 100  # two rounds (10, then 100 rows), not a third


def test_sample_before_append_simulations_raises():
    from npe_pfn import NPE_PFN_RestrictedPrior

    rp = NPE_PFN_RestrictedPrior(box_prior())
    with pytest.raises(RuntimeError, match="append_simulations"):
        rp.sample((3,))
    with pytest.raises(RuntimeError, match="append_simulations"):
        rp.log_prob(torch.zeros(1, 2))


def test_pickle_round_trip():
    rp = make("box", acceptance_threshold=0.4, max_context_rows=64)
    rp.sample((5,), save_acceptance_rate=True)
    rp2 = pickle.loads(pickle.dumps(rp))
    assert rp2.acceptance_threshold == 0.4 and rp2.max_context_rows == 64
    assert torch.equal(rp2.thetas, rp.thetas) and torch.equal(rp2.y_labels, rp.y_labels)
    assert rp2.acceptance_rate == rp.acceptance_rate and rp2.sample_counter == rp.sample_counter
    s = rp2.sample((6,))
    assert s.shape == (6, 2) and (s[:, 0] > CUT).all()
    # the default classifier (no engine yet) pickles too
    from npe_pfn import NPE_PFN_RestrictedPrior

    rp3 = pickle.loads(pickle.dumps(NPE_PFN_RestrictedPrior(box_prior(), tabpfn_classifier_kwargs={"random_state": 9})))
    assert rp3.classifier.random_state == 9 and rp3.classifier._engine is None


def test_restated_proposals_stay_in_the_box_when_the_span_rounds_up():
    """fl(high - low) > high - low: low + u * span could pass high for u close to 1; the min
    keeps the restatement (and with it the kernel it is bit-equal to) inside [low, high]."""
    rng = np.random.default_rng(0)
    found = 0
    for _ in range(200):
        low = np.float32(rng.uniform(-3, 3))
        high = np.float32(low + np.float32(rng.uniform(1e-3, 5)))
        if not float(np.float32(high - low)) > float(high) - float(low):
            continue
        found += 1
        x = ref.proposals([low], [high], 4096, seed=found, counter=3, row_base=2**32 - 50)
        assert x.dtype == np.float32 and x.shape == (4096, 1)
        assert (x >= low).all() and (x <= high).all()
        if found == 6:
            break
    assert found == 6
    # the largest u = 1 - 2^-24 itself, through the restatement's arithmetic
    low, high = np.float32(-0.1), np.float32(0.7)
    u = np.float32(1.0 - 2.0**-24)
    x = np.minimum(np.float32(low + np.float32(u * np.float32(high - low))), high)
    assert low <= x <= high
    # a degenerate column is its bound
    x = ref.proposals([0.25, -1.0], [0.25, 1.0], 10, seed=1, counter=0)
    assert (x[:, 0] == np.float32(0.25)).all()


def test_restated_append():
    rows = np.arange(12, dtype=np.float32).reshape(6, 2)
    mask = np.array([1, 0, 1, 1, 0, 1], dtype=bool)
    out, counts = ref.append(np.full((3, 2), -1, np.float32), [1, 4], rows, mask, 3)
    assert counts == [3, 8]
    np.testing.assert_array_equal(out, [[-1, -1], [0, 1], [4, 5]])
    out, counts = ref.append(np.full((3, 2), -1, np.float32), [0, 0], rows, mask, 0)
    assert counts == [0, 4] and (out == -1).all()
