"""The two entry points of the batched log density / PIT feature are exported by the built
library, declared in include/npfn.h and bound in engine.SIGNATURES (tests/test_abi.py then checks
their argument types against the header like every other symbol's).  No GPU needed."""
import ctypes

from test_abi import declared_functions, declared_prototypes


def test_library_exports_bar_cdf_and_ar_score():
    from npe_pfn.engine import SIGNATURES, load_library

    lib = load_library()
    for name in ("npfn_bar_cdf", "npfn_ar_score"):
        assert name in declared_functions(), name
        assert hasattr(lib, name), f"{name} is not exported by libnpfn.so"
        assert name in SIGNATURES, f"{name} has no ctypes signature"
    protos = declared_prototypes()
    assert len(protos["npfn_bar_cdf"]) == 7 and len(protos["npfn_ar_score"]) == 14
    assert SIGNATURES["npfn_ar_score"][1][-2] == ctypes.c_float       # eps
    assert SIGNATURES["npfn_bar_cdf"][1][3:5] == [ctypes.c_int64, ctypes.c_int32]   # n_rows, n_bars


def test_bad_arguments_are_refused_before_any_launch():
    """The argument checks of npfn_bar_cdf run on the host: no device is touched."""
    from npe_pfn.engine import load_library

    lib = load_library()
    assert lib.npfn_bar_cdf(None, None, None, 1, 1, None, None) == -1     # n_bars < 2
    assert lib.npfn_bar_cdf(None, None, None, -1, 8, None, None) == -1    # n_rows < 0
    assert lib.npfn_bar_cdf(None, None, None, 4, 8, None, None) == -1     # missing pointers
    assert b"bar_cdf" in lib.npfn_last_error()
    assert lib.npfn_bar_cdf(None, None, None, 0, 8, None, None) == 0      # nothing to do
