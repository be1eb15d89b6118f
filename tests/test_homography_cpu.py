"""CPU tier of RANSAC homography verification (efx_match_homography_async / efx_match_homography_batch_async): the C ABI
declares and exports the entry points and refuses bad arguments before the device; the numpy reference the GPU tests compare
against restates every step of the spec (checked here against literal loops and brute force) and recovers known models; the
compiled kernels use no scratch memory."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cef_loader
from tests import homography_reference as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-efficient-features_amd", "csrc")
NAMES = ("efx_default_ransac_params", "efx_match_homography_async", "efx_match_homography_batch_async")


@pytest.fixture(scope="module")
def cef():
    import __graft_entry__
    __graft_entry__.build()
    return cef_loader.load()


def test_homography_entry_points_declared_and_exported(cef):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "efx.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(cef.lib(), name), name
        assert name in cef.ABI_SYMBOLS
    assert re.search(r"typedef struct efx_homography", hdr)
    assert ctypes.sizeof(cef.RansacParams) == 24 and cef.HOMOGRAPHY_BYTES == 88


def test_default_ransac_params(cef):
    p = cef.RansacParams()
    cef.lib().efx_default_ransac_params(ctypes.byref(p))
    assert (p.hypotheses, p.threshold, p.seed, p.refine) == (2048, 3.0, 0, 1)


def test_homography_argument_errors_before_the_device(cef):
    """A NULL matcher is refused with EFX_ERR_BAD_ARG before anything reaches the device, even for npairs = 0 (no matcher needs to
    exist; the parameter, capacity and pointer checks that need one run in the GPU tier)."""
    lib = cef.lib()
    P = ctypes.c_void_p
    good = cef.RansacParams()
    lib.efx_default_ransac_params(ctypes.byref(good))
    assert lib.efx_match_homography_async(None, P(64), 4000, 10, P(64), 4000, 10, P(64), None, 10, ctypes.byref(good), P(64), P(64), None) == -1
    assert lib.efx_match_homography_batch_async(None, 1, None, 4000, 10, None, 4000, 10, None, None, 10, ctypes.byref(good), None, None,
                                                None) == -1
    assert lib.efx_match_homography_batch_async(None, 0, None, 0, 0, None, 0, 0, None, None, 0, ctypes.byref(good), None, None, None) == -1


# ---- the reference against literal restatements of S16 ----

def _splitmix_literal(x):
    M = (1 << 64) - 1
    z = (x + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def _sample_literal(n, seed, h):
    taken = []
    for j in range(4):
        r = _splitmix_literal((seed + 4 * h + j) & ((1 << 64) - 1))
        v = ((r >> 32) * (n - j)) >> 32
        for e in sorted(taken):
            if v >= e:
                v += 1
        taken.append(v)
    return taken


@pytest.mark.parametrize("n,seed", [(4, 0), (5, 1), (7, 2 ** 64 - 3), (100, 12345), (40000, 2 ** 63 + 11)])
def test_sampler_equals_the_literal_loop(n, seed):
    got = HR.sample(n, seed, 300)
    for h in range(300):
        want = _sample_literal(n, seed, h)
        assert list(got[h]) == want, (n, seed, h)
        assert len(set(want)) == 4 and all(0 <= v < n for v in want)


def test_sampler_indices_distinct_and_cover_the_range():
    for n in (4, 5, 6, 9, 1000):
        idx = HR.sample(n, 99, 20000)
        s = np.sort(idx, axis=1)
        assert np.all(np.diff(s, axis=1) > 0) and idx.min() >= 0 and idx.max() < n
        if n <= 9:
            assert len(np.unique(idx)) == n
    # the offset of a later hypothesis block equals the block from 0 (counter-based, no state)
    assert np.array_equal(HR.sample(50, 7, 100, first=900), HR.sample(50, 7, 1000)[900:])


def _subset_literal(s, d):
    def cr(a, b, c):
        return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    flips = 0
    for i, j, k in HR.TRIPLES:
        cs, cd = cr(s[i], s[j], s[k]), cr(d[i], d[j], d[k])
        if cs == 0 or cd == 0:
            return False
        flips += (cs > 0) != (cd > 0)
    return flips in (0, 4)


def test_subset_check_equals_brute_force():
    rng = np.random.default_rng(16)
    for span in (3, 6, 2000, 32767):
        s = rng.integers(-span, span + 1, (3000, 4, 2)).astype(np.int64)
        d = rng.integers(-span, span + 1, (3000, 4, 2)).astype(np.int64)
        d[:500] = s[:500]                                  # identity samples: valid unless degenerate
        d[500:800] = -s[500:800]                           # a point reflection keeps every orientation
        d[800:1000, :, 0] = -s[800:1000, :, 0]             # a mirror flips all four
        d[800:1000, :, 1] = s[800:1000, :, 1]
        got = HR.subset_ok(s, d)
        want = np.array([_subset_literal([tuple(map(int, p)) for p in s[i]], [tuple(map(int, p)) for p in d[i]]) for i in range(len(s))])
        assert np.array_equal(got, want), span
        assert got.any() and (~got).any()


def test_subset_check_degenerate_samples():
    s = np.array([[[0, 0], [10, 0], [20, 0], [5, 7]]], dtype=np.int64)            # a collinear triple
    assert not HR.subset_ok(s, s)[0]
    s = np.array([[[0, 0], [10, 0], [10, 10], [0, 0]]], dtype=np.int64)           # a repeated location
    assert not HR.subset_ok(s, s)[0]
    s = np.array([[[0, 0], [10, 0], [10, 10], [0, 10]]], dtype=np.int64)
    assert HR.subset_ok(s, s)[0]
    d = s.copy()
    d[0, 2] = [-10, -10]                                   # one corner pulled through: a bow tie, orientations disagree
    assert not HR.subset_ok(s, d)[0]


def test_four_point_reproduces_a_known_model():
    rng = np.random.default_rng(160)
    for _ in range(200):
        H = HR.true_homography(rng, rot=0.5, scale=0.3, persp=1e-4)
        s = np.stack([rng.integers(0, 1920, 4), rng.integers(0, 1080, 4)], axis=1).astype(np.int64)
        d = HR.project(H, s.astype(np.float64))
        # exact correspondences need integer dst: scale the model so they are (H' = diag(1/k) ... is not integral); instead
        # take the four-point fit of (s, d) with rounded d and check it maps s onto the rounded d exactly (to 1e-6)
        di = np.rint(d).astype(np.int64)
        if not HR.subset_ok(s[None], di[None])[0]:
            continue
        M, ok = HR.four_point(s[None], di[None])
        assert ok[0]
        assert np.allclose(HR.project(M[0].reshape(3, 3), s.astype(np.float64)), di, atol=1e-6)
        assert M[0, 8] == 1.0
    # an exact integer model: a similarity with integer coefficients maps integer points to integer points
    H = np.array([[2.0, -1.0, 30.0], [1.0, 2.0, -7.0], [0.0, 0.0, 1.0]])
    s = np.array([[[3, 4], [100, 7], [90, 80], [10, 60]]], dtype=np.int64)
    d = np.rint(HR.project(H, s[0].astype(np.float64))).astype(np.int64)[None]
    M, ok = HR.four_point(s, d)
    assert ok[0] and np.allclose(M[0].reshape(3, 3), H, rtol=0, atol=1e-12)


def test_four_point_agrees_with_the_dlt_solve():
    rng = np.random.default_rng(161)
    checked = 0
    for _ in range(500):
        s = rng.integers(0, 1920, (4, 2)).astype(np.int64)
        d = rng.integers(0, 1920, (4, 2)).astype(np.int64)
        if not HR.subset_ok(s[None], d[None])[0]:
            continue
        M, ok = HR.four_point(s[None], d[None])
        A, b = HR.dlt_system(s.astype(np.float64), d.astype(np.float64))
        h = np.linalg.solve(A, b)
        want = np.append(h, 1.0)
        assert ok[0]
        assert np.max(np.abs(M[0] - want)) <= 1e-9 * np.max(np.abs(want)), (s, d)
        checked += 1
    assert checked > 100


def test_score_equals_a_per_element_loop():
    rng = np.random.default_rng(162)
    f = np.float32
    c = rng.normal(0, 1, (8, 9)).astype(f)
    c[:, 6:8] *= f(1e-3)
    c[0] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    c[1, 6:9] = 0                                          # W == 0 everywhere
    x, y = rng.integers(0, 1920, 300).astype(f), rng.integers(0, 1080, 300).astype(f)
    xd, yd = (x + rng.integers(-4, 5, 300)).astype(f), (y + rng.integers(-4, 5, 300)).astype(f)
    got = HR.inliers(c, x, y, xd, yd, 3.0)
    t2 = f(3.0) * f(3.0)
    with np.errstate(all="ignore"):
        for k in range(len(c)):
            for i in range(len(x)):
                X = (c[k, 0] * x[i] + c[k, 1] * y[i]) + c[k, 2]
                Y = (c[k, 3] * x[i] + c[k, 4] * y[i]) + c[k, 5]
                W = (c[k, 6] * x[i] + c[k, 7] * y[i]) + c[k, 8]
                ex, ey = X - xd[i] * W, Y - yd[i] * W
                assert type(ex) is np.float32 and type(W) is np.float32
                want = bool(W != 0) and bool(ex * ex + ey * ey <= t2 * (W * W))
                assert got[k, i] == want, (k, i)
    assert got[0].any() and not got[1].any()


@pytest.mark.parametrize("outliers", [0.3, 0.5, 0.7])
def test_reference_recovers_the_true_model(outliers):
    rng = np.random.default_rng(int(outliers * 100))
    for trial in range(3):
        H = HR.true_homography(rng)
        q, t, m = HR.synth_matches(rng, 1500, outliers, H, q_extra=50, t_extra=30)
        r = HR.ransac(q, t, m, None, len(m), seed=trial, hyps=2048)
        assert r["hypothesis"] >= 0 and r["refined"] == 1
        err = np.abs(HR.project(r["H"], HR.corners()) - HR.project(H, HR.corners())).max()
        assert err < 1.0, (outliers, trial, err)
        assert r["ninliers"] == int(r["mask"].sum()) >= int(0.6 * (1 - outliers) * len(m))


def test_reference_no_model_cases():
    rng = np.random.default_rng(163)
    q = rng.integers(0, 100, (10, 2))
    m = np.stack([np.arange(10), np.arange(10), np.zeros(10)], axis=1).astype(np.int32)
    for n in (0, 1, 3):
        r = HR.ransac(q, q, m, n, 10, hyps=64)
        assert r["hypothesis"] == -1 and r["ninliers"] == 0 and not r["mask"].any() and not r["H"].any()
    line = np.stack([np.arange(10) * 7, np.arange(10) * 3], axis=1)
    r = HR.ransac(line, line, m, None, 10, hyps=64)
    assert r["hypothesis"] == -1 and r["valid_hypotheses"] == 0


def test_homography_kernels_use_no_scratch():
    """hipcc -S of homography_kernels.hip: no kernel has a private segment (a dispatch with one stalls, DESIGN history)."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc (ROCm) on this machine")
    import tempfile
    flags = "-std=c++17 -O3 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math --cuda-device-only -S".split()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "hom.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + [os.path.join(CSRC, "homography_kernels.hip"), "-o", out], cwd=CSRC,
                              stderr=subprocess.DEVNULL)
        text = open(out).read()
    kernels = re.findall(r"^(_Z\w+):.*?\.amdhsa_private_segment_fixed_size (\d+)", text, flags=re.S | re.M)
    names = [k for k, _ in kernels]
    parts = ("gather", "hyp", "score", "mask", "dist", "normal", "finish")
    assert len(kernels) == len(parts) and all(any("hom_%s_kernel" % s in k for k in names) for s in parts), names
    assert all(int(v) == 0 for _, v in kernels), kernels
