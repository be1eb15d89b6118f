"""CPU tier of mutual ratio-test matching (efx_match_mutual_async / efx_match_mutual_batch_async): the C ABI
declares and exports both entry points, and the numpy reference the GPU tests compare against agrees with a literal
restatement of the reference sample's loop."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import cef_loader
from tests import mutual_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cef():
    import __graft_entry__
    __graft_entry__.build()
    return cef_loader.load()


def test_mutual_entry_points_declared_and_exported(cef):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "efx.h")).read(), flags=re.S)
    for name in ("efx_match_mutual_async", "efx_match_mutual_batch_async"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(cef.lib(), name), name
        assert name in cef.ABI_SYMBOLS


def test_mutual_argument_errors_before_the_device(cef):
    """Bad arguments are refused before anything reaches the device (no matcher needs to exist for a NULL handle)."""
    lib = cef.lib()
    P = ctypes.c_void_p
    assert lib.efx_match_mutual_async(None, P(64), 32, None, 10, P(64), 32, None, 10, 32, 0.9, P(64), P(64), None) == -1
    assert lib.efx_match_mutual_batch_async(None, 1, None, 32, None, 10, None, 32, None, 10, 32, 0.9, None, None, None) == -1


SIZES = [0, 1, 2, 3, 50]
RATIOS = [0.0, 0.5, 0.9, 1.0, 2.0]


@pytest.mark.parametrize("nbytes", [32, 64])
def test_reference_equals_sample_loop_random(nbytes):
    rng = np.random.default_rng(15 + nbytes)
    for nq, nt in itertools.product(SIZES, SIZES):
        q, t = MR.random_set(rng, nq, nbytes), MR.random_set(rng, nt, nbytes)
        for r in RATIOS:
            got, want = MR.mutual(q, t, r), MR.sample_loop(q, t, r)
            assert np.array_equal(got, want), (nq, nt, r)


@pytest.mark.parametrize("distinct", [1, 2, 4])
def test_reference_equals_sample_loop_tie_heavy(distinct):
    rng = np.random.default_rng(150 + distinct)
    for nq, nt in itertools.product(SIZES, SIZES):
        q, t = MR.random_set(rng, nq, 32, distinct), MR.random_set(rng, nt, 32, distinct)
        for r in RATIOS:
            got, want = MR.mutual(q, t, r), MR.sample_loop(q, t, r)
            assert np.array_equal(got, want), (nq, nt, r, distinct)


def test_reference_ratio_one_is_crosscheck():
    """ratio >= 1 never rejects (d0 <= d1): the filter is the cross check, compacted."""
    from oracle import matcher_oracle as MO
    rng = np.random.default_rng(7)
    for distinct in (None, 3):
        q, t = MR.random_set(rng, 60, 32, distinct), MR.random_set(rng, 45, 32, distinct)
        m, d = MO.crosscheck(q, t)
        keep = np.nonzero(m >= 0)[0]
        want = np.stack([keep, m[keep], d[keep]], axis=1).astype(np.int32).reshape(-1, 3)
        assert np.array_equal(MR.mutual(q, t, 1.0), want)
        assert np.array_equal(MR.mutual(q, t, 2.0), want)
