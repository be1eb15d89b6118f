"""CPU tier of guided (spatially gated) mutual matching (efx_match_guided_async / efx_match_guided_batch_async): the C
ABI declares and exports the entry points and refuses bad arguments before the device; the numpy reference the GPU tests compare
against equals a literal per-pair restatement of the spec on small sets (ties, duplicate locations, points exactly `radius` away,
priors with W <= 0, a prior without a model, an empty side) and has the two consequences the spec promises; the compiled kernels
use no scratch memory."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cef_loader
from tests import guided_reference as GR
from tests import mutual_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-efficient-features_amd", "csrc")
NAMES = ("efx_default_guided_params", "efx_match_guided_async", "efx_match_guided_batch_async")


@pytest.fixture(scope="module")
def cef():
    import __graft_entry__
    __graft_entry__.build()
    return cef_loader.load()


def test_guided_entry_points_declared_and_exported(cef):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "efx.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(cef.lib(), name), name
        assert name in cef.ABI_SYMBOLS
    assert re.search(r"typedef struct efx_guided_params", hdr)
    assert ctypes.sizeof(cef.GuidedParams) == 24
    assert "#define EFX_VERSION 100" in hdr and cef.lib().efx_version() == 100


def test_default_guided_params(cef):
    p = cef.GuidedParams()
    cef.lib().efx_default_guided_params(ctypes.byref(p))
    assert (p.radius, p.max_octave_diff, p.ratio, p.width, p.height) == (16.0, -1, 0.9, 0, 0)
    cef.lib().efx_default_guided_params(None)


def test_guided_argument_errors_before_the_device(cef):
    """A NULL matcher is refused with EFX_ERR_BAD_ARG before anything reaches the device, even for npairs = 0 (the parameter,
    capacity and pointer checks that need a matcher run in the GPU tier)."""
    lib = cef.lib()
    P = ctypes.c_void_p
    good = cef.GuidedParams()
    lib.efx_default_guided_params(ctypes.byref(good))
    assert lib.efx_match_guided_async(None, P(64), 32, None, 10, P(64), 4000, P(64), 32, None, 10, P(64), 4000, 32, None, ctypes.byref(good),
                                      P(64), P(64), None) == -1
    assert lib.efx_match_guided_batch_async(None, 1, None, 32, None, 10, None, 4000, None, 32, None, 10, None, 4000, 32, None,
                                            ctypes.byref(good), None, None, None) == -1
    assert lib.efx_match_guided_batch_async(None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, 32, None, ctypes.byref(good), None,
                                            None, None) == -1


# ---- the reference against the literal loop ----

def _noisy_pairs(rng, n, nbytes, flips=20, pool=None):
    """train = query with a few flipped bits (true matches), or both drawn from a small pool (ties)"""
    if pool:
        base = MR.random_set(rng, pool, nbytes)
        return base[rng.integers(0, pool, n)], base[rng.integers(0, pool, n)]
    q = MR.random_set(rng, n, nbytes)
    t = q.copy()
    for r in t:
        for b in rng.integers(0, nbytes * 8, flips):
            r[b >> 3] ^= 1 << (b & 7)
    return q, t


def _check(q, t, lq, lt, oq, ot, prior, radius, mod, ratio, tag):
    got = GR.guided(q, t, lq, lt, oq, ot, prior, radius, mod, ratio)
    want = GR.literal(q, t, lq, lt, oq, ot, prior, radius, mod, ratio)
    assert np.array_equal(got, want), (tag, got, want)
    return got


def test_reference_equals_the_literal_loop_on_random_sets():
    rng = np.random.default_rng(1700)
    total = 0
    for trial in range(12):
        nq, nt = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        nbytes = (32, 64)[trial & 1]
        q, t = _noisy_pairs(rng, max(nq, nt), nbytes, pool=(None, 6)[(trial >> 1) & 1])
        q, t = q[:nq], t[:nt]
        lq = rng.integers(0, 60, (nq, 2))
        lt = np.concatenate([lq, lq])[:nt] + rng.integers(-3, 4, (nt, 2)) if nt <= 2 * nq else rng.integers(0, 60, (nt, 2))
        oq, ot = rng.integers(0, 4, nq), rng.integers(0, 4, nt)
        H = np.array([[1.02, 0.01, -1.5], [-0.02, 0.99, 2.25], [1e-4, -2e-4, 1.0]])
        for prior in (None, (H, 3)):
            for radius, mod in [(1.0, -1), (4.5, 0), (16.0, 1), (70000.0, -1)]:
                total += len(_check(q, t, lq, lt, oq, ot, prior, radius, mod, (0.9, 0.7, 1.5)[trial % 3], (trial, radius, mod)))
    assert total > 100


def test_reference_ties_and_duplicate_locations():
    rng = np.random.default_rng(1701)
    pool = MR.random_set(rng, 3, 32)
    q, t = pool[rng.integers(0, 3, 40)], pool[rng.integers(0, 3, 40)]
    lq = np.tile([[10, 10]], (40, 1))                      # every keypoint at one location: C is everything
    rows = _check(q, t, lq, lq, None, None, None, 1.0, -1, 0.9, "one location")
    assert np.array_equal(rows, MR.mutual(q, t, 0.9))
    lq = rng.integers(0, 3, (40, 2)) * 5                   # nine locations, many duplicates
    lt = rng.integers(0, 3, (40, 2)) * 5
    for radius in (0.5, 5.0, 7.5):
        _check(q, t, lq, lt, None, None, None, radius, -1, 1.0, ("duplicates", radius))


def test_reference_window_is_square_and_inclusive():
    rng = np.random.default_rng(1702)
    q = MR.random_set(rng, 1, 32)
    t = np.repeat(q, 6, axis=0)
    t[:, 0] ^= np.arange(1, 7, dtype=np.uint8)             # distinct distances, train 0 is the nearest
    lq = np.array([[100, 100]])
    lt = np.array([[108, 100], [100, 92], [108, 108], [109, 100], [100, 91], [92, 92]])
    rows = _check(q, t, lq, lt, None, None, None, 8.0, -1, 2.0, "inclusive")
    assert rows.tolist() == [[0, 0, 1]]                    # exactly radius away in x: a candidate, and the nearest
    ii, jj = GR.candidates(lq, lt, None, None, None, 8.0, -1)
    assert jj.tolist() == [0, 1, 2, 5]                     # the corners (108, 108) and (92, 92) are inside: the window is square
    ii, jj = GR.candidates(lq, lt, None, None, None, np.float32(7.9999995), -1)
    assert jj.tolist() == []
    # the radius is a float: 16.5 is exact, a prediction of .5 makes both neighbours of a half-pixel candidates
    H = np.array([[1, 0, 0.5], [0, 1, 0], [0, 0, 1.0]])
    ii, jj = GR.candidates([[10, 10]], [[27, 10], [-6, 10], [28, 10], [-7, 10]], None, None, (H, 0), 16.5, -1)
    assert jj.tolist() == [0, 1]


def test_reference_priors_without_a_prediction():
    rng = np.random.default_rng(1703)
    q, t = _noisy_pairs(rng, 50, 32)
    lq = np.stack([np.arange(50) * 4, rng.integers(0, 50, 50)], axis=1)
    H = np.array([[1.0, 0, 0], [0, 1.0, 0], [-0.01, 0, 1.0]])        # W = 1 - x / 100: zero at x = 100, negative beyond
    px, py, valid = GR.predict(lq, (H, 0))
    assert valid[:25].all() and not valid[25:].any()
    lt = np.zeros((50, 2), np.int64)
    lt[:25] = np.rint(np.stack([px[:25], py[:25]], axis=1))
    lt[25:] = lq[25:]
    rows = _check(q, t, lq, lt, None, None, (H, 0), 2.0, -1, 0.9, "W <= 0")
    assert len(rows) > 15 and rows[:, 0].max() < 25
    big = np.array([[1e300, 0, 0], [0, 1e300, 0], [0, 0, 1e-300]])   # X / W overflows: not finite
    assert len(_check(q, t, lq, lq, None, None, (big, 0), 70000.0, -1, 0.9, "overflow")) == 0
    far = np.array([[1.0, 0, 1e7], [0, 1.0, -1e7], [0, 0, 1.0]])     # every prediction far outside the frame
    assert len(_check(q, t, lq, lq, None, None, (far, 0), 64.0, -1, 0.9, "far")) == 0
    assert len(_check(q, t, lq, lq, None, None, (np.zeros((3, 3)), -1), 16.0, -1, 0.9, "no model")) == 0
    assert len(_check(q, t, lq, lq, None, None, (np.eye(3), -1), 16.0, -1, 0.9, "no model, H set")) == 0
    assert len(_check(q, t, lq, lq, None, None, (np.eye(3), 0), 16.0, -1, 0.9, "identity")) == 50


def test_reference_empty_sides():
    rng = np.random.default_rng(1704)
    q = MR.random_set(rng, 5, 32)
    e = np.zeros((0, 32), np.uint8)
    l5, l0 = rng.integers(0, 9, (5, 2)), np.zeros((0, 2), np.int64)
    for a, b, la, lb in [(q, e, l5, l0), (e, q, l0, l5), (e, e, l0, l0)]:
        assert _check(a, b, la, lb, None, None, None, 16.0, -1, 0.9, "empty").shape == (0, 3)


def _scene(rng, n, nbytes, w=400, h=300, shift=3):
    q, t = _noisy_pairs(rng, n, nbytes, flips=30)
    pool = MR.random_set(rng, 5, nbytes)                   # a repeated structure: a fifth of the rows come from five descriptors
    rep = rng.random(n) < 0.2
    q[rep] = pool[rng.integers(0, 5, rep.sum())]
    t[rep] = pool[rng.integers(0, 5, rep.sum())]
    lq = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1)
    lt = lq + rng.integers(-shift, shift + 1, (n, 2))
    perm = rng.permutation(n)
    return q, t[perm], lq, lt[perm], rng.integers(0, 8, n), rng.integers(0, 8, n)


@pytest.mark.parametrize("nbytes", [32, 64])
def test_consequence_a_everything_in_the_window_is_brute_force(nbytes):
    rng = np.random.default_rng(1705 + nbytes)
    for n in (1, 2, 150, 600):
        q, t, lq, lt, oq, ot = _scene(rng, n, nbytes)
        lq[0] = (-32768, -32768)
        lt[-1] = (32767, 32767)                            # the extremes of the short range: 65 535 apart
        for ratio in (0.9, 1.0):
            want = MR.mutual(q, t, ratio, knn2=MR.MO.knn2_c)
            assert np.array_equal(GR.guided(q, t, lq, lt, oq, ot, None, 65535.0, -1, ratio), want), n
            assert np.array_equal(GR.guided(q, t, lq, lt, None, None, None, 1e30, -1, ratio), want), n


@pytest.mark.parametrize("nbytes", [32, 64])
def test_consequence_b_gated_brute_force_rows_survive(nbytes):
    rng = np.random.default_rng(1715 + nbytes)
    kept = recovered = 0
    for n in (200, 900):
        q, t, lq, lt, oq, ot = _scene(rng, n, nbytes)
        brute = MR.mutual(q, t, 0.9, knn2=MR.MO.knn2_c)
        H = np.array([[1.001, 0.002, -0.4], [-0.001, 0.999, 0.3], [1e-6, 0, 1.0]])
        for prior in (None, (H, 1)):
            for radius, mod in [(1.0, -1), (4.0, 1), (16.0, -1), (64.0, 0)]:
                g = GR.guided(q, t, lq, lt, oq, ot, prior, radius, mod, 0.9)
                inside = GR.within_gate(brute, lq, lt, oq, ot, prior, radius, mod)
                gs = {tuple(r) for r in g.tolist()}
                assert all(tuple(r) in gs for r in inside.tolist()), (n, radius, mod)
                kept += len(inside)
                recovered += len(g) - len(inside)
    assert kept > 500 and recovered > 0                    # the window keeps matches the global ratio test discards


def test_guided_kernels_use_no_scratch():
    """hipcc -S of guided_kernels.hip: no kernel has a private segment (a dispatch with one stalls, DESIGN history)."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc (ROCm) on this machine")
    import tempfile
    flags = "-std=c++17 -O3 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math --cuda-device-only -S".split()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "guided.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + [os.path.join(CSRC, "guided_kernels.hip"), "-o", out], cwd=CSRC,
                              stderr=subprocess.DEVNULL)
        text = open(out).read()
    kernels = re.findall(r"^(_Z\w+):.*?\.amdhsa_private_segment_fixed_size (\d+)", text, flags=re.S | re.M)
    names = [k for k, _ in kernels]
    parts = ("bin", "cellsum", "scan", "scatter", "search")
    assert len(kernels) == 6 and all(any("guided_%s_kernel" % s in k for k in names) for s in parts), names
    assert all(int(v) == 0 for _, v in kernels), kernels
