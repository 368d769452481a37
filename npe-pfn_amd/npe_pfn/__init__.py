"""MI355X-native NPE-PFN.

Same public names as the reference package (npe_pfn/__init__.py:1-12), so
``from npe_pfn import TabPFN_Based_NPE_PFN, TabPFN_Based_Uncond_Estimator,
NPE_PFN_RestrictedPrior, run_tsnpe_pfn`` keeps working with
this directory (``npe-pfn_amd``) on ``sys.path``.  The TabPFN forward runs in
the HIP engine ``npe_pfn/_lib/libnpfn.so`` (C-ABI: include/npfn.h).
"""

from npe_pfn.diagnostics import (ClassifierTestResult, CoverageRanks, TransportResult, TwoSampleResult,
                                 assignment_solve_host, bar_cdf, c2st_batched, c2st_fit_host, c2st_folds, c2st_init,
                                 c2st_order, expected_coverage, mmd_batched, mmd_sums_host, permutation_labels,
                                 pit_ks_statistic, rank_accumulate_host, rank_ks_statistic, transport_costs_host,
                                 wasserstein_batched)
from npe_pfn.marginals import PosteriorMarginals
from npe_pfn.npe_pfn import NPE_PFN_Core, TabPFN_Based_NPE_PFN, TabPFN_Based_Uncond_Estimator
from npe_pfn.pair_marginals import PosteriorPairMarginals
from npe_pfn.restricted_prior import NPE_PFN_RestrictedPrior
from npe_pfn.tsnpe_pfn import run_tsnpe_pfn

__all__ = [
    "ClassifierTestResult",
    "CoverageRanks",
    "NPE_PFN_Core",
    "NPE_PFN_RestrictedPrior",
    "PosteriorMarginals",
    "PosteriorPairMarginals",
    "TabPFN_Based_NPE_PFN",
    "TabPFN_Based_Uncond_Estimator",
    "TransportResult",
    "TwoSampleResult",
    "assignment_solve_host",
    "bar_cdf",
    "c2st_batched",
    "c2st_fit_host",
    "c2st_folds",
    "c2st_init",
    "c2st_order",
    "expected_coverage",
    "mmd_batched",
    "mmd_sums_host",
    "permutation_labels",
    "pit_ks_statistic",
    "rank_accumulate_host",
    "rank_ks_statistic",
    "run_tsnpe_pfn",
    "transport_costs_host",
    "wasserstein_batched",
]
