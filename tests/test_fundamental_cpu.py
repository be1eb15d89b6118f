"""CPU tier of RANSAC fundamental-matrix verification (efx_match_fundamental_async / efx_match_fundamental_batch_async, DESIGN.md
S18): the C ABI declares and exports the entry points and refuses bad arguments before the device; the numpy reference the GPU tests
compare against restates every step of the spec (checked here against literal per-element loops), its models are correct (against
numpy.linalg) and it recovers known epipolar geometry; the compiled kernels use no scratch memory."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cef_loader
from tests import fundamental_reference as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-efficient-features_amd", "csrc")
NAMES = ("efx_match_fundamental_async", "efx_match_fundamental_batch_async")
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def cef():
    import __graft_entry__
    __graft_entry__.build()
    return cef_loader.load()


def test_fundamental_entry_points_declared_and_exported(cef):
    raw = open(os.path.join(ROOT, "include", "efx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(cef.lib(), name), name
        assert name in cef.ABI_SYMBOLS
    assert re.search(r"typedef struct efx_fundamental", hdr)
    assert cef.FUNDAMENTAL_BYTES == cef.HOMOGRAPHY_BYTES == 88
    assert "NOT a prior for efx_match_guided_async" in raw
    assert "not a prior" in cef.BFMatcher.findFundamental.__doc__.lower()
    assert cef.lib().efx_version() == 100
    for name in ("findFundamental", "findFundamentalBatch"):
        assert hasattr(cef.BFMatcher, name)
    assert issubclass(cef.FundamentalBatch, cef.HomographyBatch)
    hpp = open(os.path.join(ROOT, "cuda-efficient-features_amd", "host", "efficient_features.hpp")).read()
    for name in ("findFundamentalAsync", "findFundamentalBatchAsync", "efx_fundamental findFundamental("):
        assert name in hpp, name


def test_fundamental_argument_errors_before_the_device(cef):
    """A NULL matcher is refused with EFX_ERR_BAD_ARG before anything reaches the device, even for npairs = 0 (the checks that need
    a matcher run in the GPU tier)."""
    lib = cef.lib()
    P = ctypes.c_void_p
    good = cef.RansacParams()
    lib.efx_default_ransac_params(ctypes.byref(good))
    assert lib.efx_match_fundamental_async(None, P(64), 4000, 10, P(64), 4000, 10, P(64), None, 10, ctypes.byref(good), P(64), P(64), None) == -1
    assert lib.efx_match_fundamental_batch_async(None, 1, None, 4000, 10, None, 4000, 10, None, None, 10, ctypes.byref(good), None, None,
                                                 None) == -1
    assert lib.efx_match_fundamental_batch_async(None, 0, None, 0, 0, None, 0, 0, None, None, 0, ctypes.byref(good), None, None, None) == -1


# ---- the reference against literal restatements of S18 ----

def _splitmix_literal(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _sample_literal(n, seed, h):
    taken = []
    for j in range(8):
        r = _splitmix_literal((seed + 8 * h + j) & M64)
        v = ((r >> 32) * (n - j)) >> 32
        for e in sorted(taken):
            if v >= e:
                v += 1
        taken.append(v)
    return taken


@pytest.mark.parametrize("n,seed", [(8, 0), (9, 1), (11, 2 ** 64 - 3), (100, 12345), (40000, 2 ** 63 + 11)])
def test_sampler_equals_the_literal_loop(n, seed):
    got = FR.sample(n, seed, 300)
    for h in range(300):
        want = _sample_literal(n, seed, h)
        assert list(got[h]) == want, (n, seed, h)
        assert len(set(want)) == 8 and all(0 <= v < n for v in want)


def test_sampler_indices_distinct_and_cover_the_range():
    for n in (8, 9, 10, 17, 1000):
        idx = FR.sample(n, 99, 20000)
        s = np.sort(idx, axis=1)
        assert np.all(np.diff(s, axis=1) > 0) and idx.min() >= 0 and idx.max() < n
        if n <= 17:
            assert len(np.unique(idx)) == n
    assert np.array_equal(FR.sample(50, 7, 100, first=900), FR.sample(50, 7, 1000)[900:])


def _eight_point_literal(s, d):
    """S18 steps 3 and 4 for one sample, element by element on Python ints and floats (IEEE double, one rounding per operation):
    (nine floats or None)"""
    s = [tuple(int(v) for v in p) for p in s]
    d = [tuple(int(v) for v in p) for p in d]
    for i in range(8):
        for j in range(i + 1, 8):
            if s[i] == s[j] or d[i] == d[j]:
                return None
    a = []
    for k in range(1, 8):
        x, y, u, v = s[k][0] - s[0][0], s[k][1] - s[0][1], d[k][0] - d[0][0], d[k][1] - d[0][1]
        a.append([float(u * x), float(u * y), float(u), float(v * x), float(v * y), float(v), float(x), float(y)])
    perm = list(range(8))
    for c in range(7):
        best, pr, pc = -1.0, c, c
        for r in range(c, 7):
            for j in range(c, 8):
                if abs(a[r][j]) > best:
                    best, pr, pc = abs(a[r][j]), r, j
        if not best > 0.0:
            return None
        a[c], a[pr] = a[pr], a[c]
        for r in range(7):
            a[r][c], a[r][pc] = a[r][pc], a[r][c]
        perm[c], perm[pc] = perm[pc], perm[c]
        for r in range(c + 1, 7):
            f = a[r][c] / a[c][c]
            for j in range(c, 8):
                a[r][j] = a[r][j] - f * a[c][j]
    z = [0.0] * 8
    z[7] = 1.0
    for r in range(6, -1, -1):
        acc = 0.0
        for j in range(r + 1, 8):
            acc = acc + a[r][j] * z[j]
        z[r] = (0.0 - acc) / a[r][r]
    f = [0.0] * 8
    for j in range(8):
        f[perm[j]] = z[j]
    ox, oy, ou, ov = float(s[0][0]), float(s[0][1]), float(d[0][0]), float(d[0][1])
    g2 = f[2] - (f[0] * ox + f[1] * oy)
    g5 = f[5] - (f[3] * ox + f[4] * oy)
    g8 = 0.0 - (f[6] * ox + f[7] * oy)
    r6 = f[6] - (ou * f[0] + ov * f[3])
    r7 = f[7] - (ou * f[1] + ov * f[4])
    r8 = g8 - (ou * g2 + ov * g5)
    F = [f[0], f[1], g2, f[3], f[4], g5, r6, r7, r8]
    m, dv = 0.0, 0.0
    for v in F:
        if abs(v) > m:
            m, dv = abs(v), v
    if dv == 0.0:
        return None
    try:
        F = [v / dv for v in F]
    except ZeroDivisionError:
        return None
    return F if all(np.isfinite(F)) else None


def _check_against_literal(s, d):
    F, fin = FR.eight_point(s, d)
    ok = FR.sample_ok(s, d) & fin
    for i in range(len(s)):
        want = _eight_point_literal(s[i], d[i])
        assert bool(ok[i]) == (want is not None), i
        if want is not None:
            assert np.array_equal(F[i].view(np.uint64), np.array(want).view(np.uint64)), (i, F[i], want)
    return ok


def test_eight_point_equals_the_literal_loop_on_random_samples():
    rng = np.random.default_rng(180)
    for span in (4, 40, 2000, 32767):
        s = rng.integers(-span, span + 1, (400, 8, 2)).astype(np.int64)
        d = rng.integers(-span, span + 1, (400, 8, 2)).astype(np.int64)
        d[:100] = s[:100] + rng.integers(-3, 4, (100, 8, 2))                   # near-identity motion
        ok = _check_against_literal(s, d)
        assert ok.any()
    # samples of a true scene: the well-conditioned case the GPU runs most
    q, t, good, _ = FR.scene(np.random.default_rng(181), 600, 0.3)
    idx = FR.sample(600, 5, 300)
    assert _check_against_literal(q[idx], t[idx]).sum() > 250


def test_eight_point_degenerate_samples():
    rng = np.random.default_rng(182)
    s = rng.integers(0, 1000, (6, 8, 2)).astype(np.int64)
    d = rng.integers(0, 1000, (6, 8, 2)).astype(np.int64)
    s[0, 5] = s[0, 2]                                      # a repeated query location
    d[1, 7] = d[1, 0]                                      # a repeated train location
    k = np.arange(8)
    s[2] = np.stack([3 * k + 1, 2 * k + 5], axis=1)        # eight collinear points on both sides
    d[2] = np.stack([5 * k, 7 * k + 2], axis=1)
    s[3] = np.stack([k * k, 10 * k], axis=1)               # a pure shift: the system has a two-dimensional null space or more
    d[3] = s[3] + 5
    ok = _check_against_literal(s, d)
    assert not ok[0] and not ok[1] and not ok[2] and ok[4] and ok[5]
    assert not FR.sample_ok(s, d)[0] and not FR.sample_ok(s, d)[1] and FR.sample_ok(s, d)[2]
    # a NaN row (an out-of-range index) invalidates the hypotheses that draw it, and only those
    q, t, _, _ = FR.scene(rng, 12, 0.0)
    m = FR.identity_matches(12)
    m[4, 0] = 99
    src, dst, rows = FR.gather(q, t, m, None, 12)
    F, valid = FR.hypotheses(src, dst, rows, 3, 200)
    idx = FR.sample(12, 3, 200)
    drew = np.any(idx == 4, axis=1)
    assert not valid[drew].any() and valid[~drew].any()
    # n = 7 / 8 / 9
    for n, any_valid in ((7, False), (8, True), (9, True)):
        r = FR.ransac(q, t, FR.identity_matches(12), n, 12, hyps=64)
        assert (r["hypothesis"] >= 0) == any_valid, n
        if n == 7:
            assert r["ninliers"] == 0 and not r["mask"].any() and not r["F"].any() and r["valid_hypotheses"] == 0
        else:
            assert r["valid_hypotheses"] == 64 and r["ninliers"] >= 8 and not r["mask"][n:].any()


def test_score_equals_a_per_element_loop():
    rng = np.random.default_rng(183)
    f = np.float32
    q, t, good, Ft = FR.scene(rng, 300, 0.5)
    c = rng.normal(0, 1, (6, 9)).astype(f)
    c[0] = (Ft / FR.first_largest(Ft.reshape(1, 9))[0]).reshape(9).astype(f)
    c[1] = 0                                               # g == 0 everywhere
    x, y, u, v = (w.astype(f) for w in (q[:, 0], q[:, 1], t[:, 0], t[:, 1]))
    x[7] = y[7] = u[7] = v[7] = np.nan
    got = FR.inliers(c, x, y, u, v, 3.0)
    t2 = f(3.0) * f(3.0)
    with np.errstate(all="ignore"):
        for k in range(len(c)):
            for i in range(len(x)):
                a = (c[k, 0] * x[i] + c[k, 1] * y[i]) + c[k, 2]
                b = (c[k, 3] * x[i] + c[k, 4] * y[i]) + c[k, 5]
                cc = (c[k, 6] * x[i] + c[k, 7] * y[i]) + c[k, 8]
                a2 = (c[k, 0] * u[i] + c[k, 3] * v[i]) + c[k, 6]
                b2 = (c[k, 1] * u[i] + c[k, 4] * v[i]) + c[k, 7]
                r = (a * u[i] + b * v[i]) + cc
                g = (a * a + b * b) + (a2 * a2 + b2 * b2)
                assert type(r) is np.float32 and type(g) is np.float32
                assert got[k, i] == (bool(g > 0) and bool(r * r <= t2 * g)), (k, i)
    assert got[0][good].sum() > 100 and not got[1].any() and not got[:, 7].any()


# ---- the models are right ----

def test_eight_point_annihilates_its_points_and_agrees_with_svd():
    rng = np.random.default_rng(184)
    q, t, _, _ = FR.scene(rng, 2000, 0.4)
    idx = FR.sample(2000, 1, 400)
    s, d = q[idx], t[idx]
    F, fin = FR.eight_point(s, d)
    ok = FR.sample_ok(s, d) & fin
    assert ok.sum() > 350
    eps = np.finfo(np.float64).eps
    agreed, worst = 0, 0.0
    for i in np.nonzero(ok)[0]:
        M = F[i].reshape(3, 3)
        a = np.concatenate([s[i], np.ones((8, 1))], axis=1)
        b = np.concatenate([d[i], np.ones((8, 1))], axis=1)
        A = np.stack([b[:, j // 3] * a[:, j % 3] for j in range(9)], axis=1)                 # 8 x 9, A f = 0
        sv = np.linalg.svd(A, compute_uv=False)
        cond = sv[0] / sv[7]
        # x'^T F x at the double rounding level relative to |F| |x| |x'|, whatever the conditioning: elimination with complete
        # pivoting is backward stable, so the residual is small even where the model itself is badly determined
        res = np.abs(np.einsum("ki,ij,kj->k", b, M, a))
        scale = np.linalg.norm(M) * np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)
        worst = max(worst, float((res / scale).max()))
        assert np.all(res <= 64 * eps * scale), (i, res / scale, cond)
        if cond < 1e8:                                                                        # a well-conditioned sample
            nv = np.linalg.svd(A)[2][8]
            nv = nv / FR.first_largest(nv[None])[0]
            assert np.max(np.abs(nv - F[i])) <= 1e-6, (i, cond)
            agreed += 1
    print("worst |x'^T F x| / (|F| |x| |x'|): %.3g (eps %.3g); %d samples agree with the svd" % (worst, eps, agreed))
    assert agreed > 50


def test_refit_agrees_with_a_textbook_fit_and_has_rank_two():
    for seed, n, outliers in ((185, 2000, 0.3), (186, 400, 0.4), (187, 40, 0.0), (188, 8, 0.0)):
        rng = np.random.default_rng(seed)
        q, t, good, _ = FR.scene(rng, n, outliers)
        F = FR.refit(q[good], t[good])
        T = FR.textbook_fit(q[good], t[good])
        assert F is not None and np.abs(F).max() == 1.0
        diff = np.abs(np.abs(FR.sampson(F, q[good], t[good])) - np.abs(FR.sampson(T, q[good], t[good])))
        assert diff.max() < 1e-3, (seed, diff.max())                                          # the refit tolerance of the GPU tier
        assert abs(np.linalg.det(F)) <= 1e-12 * np.linalg.norm(F) ** 3, np.linalg.det(F)


def test_jacobi_equals_eigh():
    rng = np.random.default_rng(189)
    for n in (3, 9):
        B = rng.normal(0, 1, (20, n))
        M = B.T @ B
        w, V = FR.jacobi(M)
        assert np.allclose(np.sort(w), np.linalg.eigvalsh(M), rtol=1e-12, atol=1e-12)
        assert np.allclose(V.T @ V, np.eye(n), atol=1e-13) and np.allclose(M @ V, V * w, atol=1e-11)


CASES = [(2000, 0.3), (2000, 0.5), (400, 0.4)]


@pytest.mark.parametrize("n,outliers", CASES)
def test_reference_recovers_the_true_model(n, outliers):
    """The acceptance conditions of S18 on FR.scene (a camera moving through a 3-D scene, rounded locations, random outliers):
    recall >= 0.95 of the true inliers and precision >= 0.97 at 2048 hypotheses and threshold 3.0, seeds fixed."""
    for trial in range(3):
        rng = np.random.default_rng(1800 + 10 * CASES.index((n, outliers)) + trial)
        q, t, good, Ft = FR.scene(rng, n, outliers)
        qq, tt, m = FR.shuffled_matches(rng, q, t, q_extra=40, t_extra=25)
        r = FR.ransac(qq, tt, m, None, n, seed=trial, hyps=2048, threshold=3.0)
        mask = r["mask"].astype(bool)
        recall = (mask & good).sum() / good.sum()
        precision = (mask & good).sum() / max(mask.sum(), 1)
        print("n %d outliers %.1f trial %d: recall %.4f precision %.4f" % (n, outliers, trial, recall, precision))
        assert r["hypothesis"] >= 0 and r["refined"] == 1 and r["ninliers"] == mask.sum()
        assert recall >= 0.95 and precision >= 0.97, (n, outliers, trial, recall, precision)


def test_reference_no_model_cases():
    rng = np.random.default_rng(190)
    q = rng.integers(0, 100, (20, 2))
    m = FR.identity_matches(20)
    for n in (0, 1, 7):
        r = FR.ransac(q, q + 3, m, n, 20, hyps=64)
        assert r["hypothesis"] == -1 and r["ninliers"] == 0 and not r["mask"].any() and not r["F"].any()
    line = np.stack([np.arange(20) * 7, np.arange(20) * 3], axis=1)
    r = FR.ransac(line, line, m, None, 20, hyps=64)
    assert r["hypothesis"] == -1 and r["valid_hypotheses"] == 0
    same = np.tile([[5, 6]], (20, 1))
    r = FR.ransac(same, same, m, None, 20, hyps=64)
    assert r["hypothesis"] == -1 and r["valid_hypotheses"] == 0


def test_fundamental_kernels_use_no_scratch():
    """hipcc -S of fundamental_kernels.hip: no kernel has a private segment (a dispatch with one stalls, DESIGN history); the
    hypothesis kernel keeps its 7 x 8 system in LDS instead."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc (ROCm) on this machine")
    import tempfile
    flags = "-std=c++17 -O3 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math --cuda-device-only -S".split()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "fun.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + [os.path.join(CSRC, "fundamental_kernels.hip"), "-o", out], cwd=CSRC,
                              stderr=subprocess.DEVNULL)
        text = open(out).read()
    kernels = re.findall(r"^(_Z\w+):.*?\.amdhsa_private_segment_fixed_size (\d+)", text, flags=re.S | re.M)
    names = [k for k, _ in kernels]
    parts = ("hom_gather", "fun_hyp", "fun_score", "fun_mask", "fun_dist", "fun_normal", "fun_finish")
    assert len(kernels) == len(parts) and all(any("%s_kernel" % s in k for k in names) for s in parts), names
    assert all(int(v) == 0 for _, v in kernels), kernels
    score = text[text.index("fun_score_kernel"):text.index("fun_mask_kernel")]
    assert "v_pk_mul_f32" in score and "v_pk_add_f32" in score
