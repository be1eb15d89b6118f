"""GPU tier of RANSAC fundamental-matrix verification (efx_match_fundamental_async / efx_match_fundamental_batch_async, DESIGN.md
S18): every case is compared with the numpy reference (tests/fundamental_reference.py, itself checked against literal restatements
of the spec in the CPU tier).  The winner, the valid-hypothesis count, the inlier count, the mask and the eight-point model are
equal bit for bit; the refit is compared by the signed Sampson distance of every row.  Counts come from device ints; rows past a
count hold garbage."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import fundamental_reference as FR
from tests import homography_reference as HR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFIT_TOL = 1e-3         # px of signed Sampson distance, S16's refit tolerance; summation order alone moves it by < 1e-9


@pytest.fixture(scope="module")
def cef():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cef_loader
    return cef_loader.load()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    return torch


def _cnt(torch, n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def _upload(torch, q, t, m, cap=None, seed=0):
    """keypoint matrices (LOCATION = q / t) and a cap x 3 match list whose rows past len(m) hold garbage"""
    cap = len(m) if cap is None else cap
    rng = np.random.default_rng(seed)
    mm = rng.integers(-(1 << 30), 1 << 30, (max(cap, 1), 3)).astype(np.int32)
    mm[:len(m)] = m
    kq = torch.from_numpy(FR.pack_location(q)).cuda()
    kt = torch.from_numpy(FR.pack_location(t)).cuda()
    dm = torch.from_numpy(mm).cuda()[:cap]
    return kq, kt, dm, mm[:cap]


def _info(out):
    F, info, mask = out
    i = info.cpu().numpy()
    return F.cpu().numpy(), dict(ninliers=int(i[0]), hypothesis=int(i[1]), valid_hypotheses=int(i[2]), refined=int(i[3])), mask.cpu().numpy()


def _rows(q, t, hm, n, cap):
    """the correspondences below the clamped count whose indices are in range"""
    src, dst, ok = FR.gather(q, t, hm, n, cap)
    return src[ok], dst[ok]


def _compare(got, ref, refine, tag, rows=None):
    """rows: (src, dst) for the refit parity; None compares the bit-exact parts only (inputs that leave F undetermined)"""
    F, info, mask = _info(got)
    assert info["hypothesis"] == ref["hypothesis"], (tag, info, ref["hypothesis"])
    assert info["valid_hypotheses"] == ref["valid_hypotheses"], (tag, info, ref["valid_hypotheses"])
    assert info["ninliers"] == ref["ninliers"], (tag, info, ref["ninliers"])
    assert np.array_equal(mask, ref["mask"]), tag
    if ref["hypothesis"] < 0:
        assert not F.any() and info["refined"] == 0, tag
        return
    if not refine:
        assert info["refined"] == 0, tag
        assert np.array_equal(F.view(np.uint64), ref["eight_point"].view(np.uint64)), (tag, F, ref["eight_point"])
        return
    if rows is None:
        if info["refined"] == 0:
            assert np.array_equal(F.view(np.uint64), ref["eight_point"].view(np.uint64)), tag
        return
    assert info["refined"] == ref["refined"], (tag, info)
    if ref["refined"]:
        assert np.abs(F).max() == 1.0, tag
        d = np.abs(FR.sampson(F, *rows) - FR.sampson(ref["F"], *rows))
        print("refit parity", tag, "max |d Sampson| %.3g px over %d rows" % (d.max() if len(d) else 0.0, len(d)))
        assert np.all(d < REFIT_TOL), (tag, d.max())
    else:
        assert np.array_equal(F.view(np.uint64), ref["eight_point"].view(np.uint64)), tag


SIZES = [0, 1, 7, 8, 9, 64, 1000, 5000, 40000]


@pytest.mark.parametrize("outliers", [0.0, 0.5, 0.9])
def test_fundamental_sizes_outliers_budgets(cef, torch_mod, outliers):
    rng = np.random.default_rng(int(outliers * 10) + 1800)
    mt = cef.BFMatcher.create()
    for n in SIZES:
        q0, t0, good, Ft = FR.scene(rng, n, outliers)
        q, t, m = FR.shuffled_matches(rng, q0, t0, q_extra=7, t_extra=3)
        kq, kt, dm, hm = _upload(torch_mod, q, t, m, cap=n + 11, seed=n)
        cnt = _cnt(torch_mod, n)
        rows = _rows(q, t, hm, n, n + 11)
        for hyps in (1, 64, 2048):
            seed = n * 7 + hyps
            ref = FR.ransac(q, t, hm, n, n + 11, seed=seed, hyps=hyps, threshold=3.0)
            for refine in (False, True):
                got = mt.findFundamental(kq, kt, dm, cnt, threshold=3.0, hypotheses=hyps, seed=seed, refine=refine)
                _compare(got, ref, refine, (n, outliers, hyps, refine), rows)
            if n >= 1000 and hyps == 2048 and outliers <= 0.5:
                mask = ref["mask"][:n].astype(bool)
                assert ref["refined"] == 1
                assert (mask & good).sum() >= 0.95 * good.sum() and (mask & good).sum() >= 0.97 * mask.sum(), (n, outliers)


def test_fundamental_thresholds_and_seeds(cef, torch_mod):
    rng = np.random.default_rng(1810)
    mt = cef.BFMatcher.create()
    q0, t0, _, _ = FR.scene(rng, 3000, 0.4)
    q, t, m = FR.shuffled_matches(rng, q0, t0)
    kq, kt, dm, hm = _upload(torch_mod, q, t, m)
    rows = _rows(q, t, hm, None, len(m))
    for thr, seed in [(0.5, 1), (1.0, 2 ** 64 - 1), (3.0, 2 ** 40), (10.0, 5), (250.0, 6), (2.0, 2 ** 64 - 9)]:
        ref = FR.ransac(q, t, hm, None, len(m), seed=seed, hyps=300, threshold=thr)
        _compare(mt.findFundamental(kq, kt, dm, None, threshold=thr, hypotheses=300, seed=seed, refine=False), ref, False, (thr, seed))
        _compare(mt.findFundamental(kq, kt, dm, None, threshold=thr, hypotheses=300, seed=seed), ref, True, (thr, seed), rows)


def test_fundamental_degenerate_sets(cef, torch_mod):
    """Collinear points, repeated locations, out-of-range indices, garbage past the count, counts above the capacity and below 0;
    a planar scene and a purely rotating camera (F undetermined: the bit-exact parts only)."""
    rng = np.random.default_rng(1820)
    mt = cef.BFMatcher.create()
    cases = []
    k = np.arange(500)
    line = np.stack([k * 3 + 5, k * 2 + 1], axis=1)
    ident = FR.identity_matches(500)
    cases.append(("collinear", line, line + 10, ident, 500, 500, False))
    few = np.array([[10, 10], [200, 15], [180, 300], [40, 90], [500, 7], [33, 600], [250, 250]])[rng.integers(0, 7, 500)]
    cases.append(("seven locations", few, few * 2, ident, 500, 500, False))
    same = np.tile([[77, 88]], (500, 1))
    cases.append(("one location", same, same, ident, 500, 500, False))
    q0, t0, _, _ = FR.scene(rng, 2000, 0.3)
    q, t, m = FR.shuffled_matches(rng, q0, t0, q_extra=9, t_extra=4)
    bad = m.copy()
    sel = rng.random(2000) < 0.1
    bad[sel, 0] = rng.choice([-1, -(1 << 31), len(q), len(q) + 5, 1 << 30], sel.sum())
    sel2 = rng.random(2000) < 0.08
    bad[sel2, 1] = rng.choice([-7, len(t), (1 << 31) - 1], sel2.sum())
    cases.append(("out of range", q, t, bad, 2000, 2000, True))
    cases.append(("count above capacity", q, t, m, 2000, 10 ** 6, True))
    cases.append(("negative count", q, t, m, 2000, -3, True))
    cases.append(("count below capacity", q, t, m, 2000, 1234, True))
    allbad = m.copy()
    allbad[:, 1] = len(t) + 1
    cases.append(("every row out of range", q, t, allbad, 2000, 2000, True))
    pq, pt, pm = HR.synth_matches(rng, 2000, 0.3, HR.true_homography(rng))
    cases.append(("planar scene", pq, pt, pm, 2000, 2000, False))
    th = 0.03
    Rz = np.array([[np.cos(th), -np.sin(th), 960 - 960 * np.cos(th) + 540 * np.sin(th)],
                   [np.sin(th), np.cos(th), 540 - 960 * np.sin(th) - 540 * np.cos(th)], [0, 0, 1.0]])
    rq, rt, rm = HR.synth_matches(rng, 2000, 0.2, Rz)
    cases.append(("pure rotation", rq, rt, rm, 2000, 2000, False))
    for name, qq, tt, mm, cap, n, determined in cases:
        kq, kt, dm, hm = _upload(torch_mod, qq, tt, mm, cap=cap, seed=len(name))
        ref = FR.ransac(qq, tt, hm, n, cap, seed=3, hyps=512)
        rows = _rows(qq, tt, hm, n, cap) if determined else None
        for refine in (False, True):
            _compare(mt.findFundamental(kq, kt, dm, _cnt(torch_mod, n), hypotheses=512, seed=3, refine=refine), ref, refine, name, rows)
        if name in ("seven locations", "one location", "every row out of range", "negative count"):
            assert ref["hypothesis"] == -1 and ref["valid_hypotheses"] == 0, name
        if name == "collinear":
            # a rank-deficient system is rejected where the elimination meets an exact zero; rounding can leave a few samples a
            # tiny pivot, and their model still contains every point of the two lines
            assert ref["ninliers"] in (0, 500), (name, ref["valid_hypotheses"], ref["ninliers"])
        if name in ("planar scene", "pure rotation"):
            assert ref["hypothesis"] >= 0 and ref["ninliers"] > 500, name
        if name == "out of range":
            assert 0 < ref["valid_hypotheses"] < 512 and ref["hypothesis"] >= 0, name


@pytest.mark.parametrize("npairs", [1, 2, 16, 17, 33])
def test_fundamental_batch_equals_single_calls(cef, torch_mod, npairs):
    """FundamentalBatch over npairs pairs (several chains for 17 and 33) with mixed device counts equals single calls bit for bit,
    the refit included, and the reference."""
    rng = np.random.default_rng(1830 + npairs)
    mt, single = cef.BFMatcher.create(), cef.BFMatcher.create()
    cap, qcap, tcap = 3000, 3100, 3050
    data = []
    for i in range(npairs):
        n = [0, 7, 8, 50, 999, 3000, 2500][i % 7]
        q0, t0, _, _ = FR.scene(rng, n, [0.1, 0.5, 0.8][i % 3])
        q, t, m = FR.shuffled_matches(rng, q0, t0, q_extra=qcap - n, t_extra=tcap - n)
        kq, kt, dm, hm = _upload(torch_mod, q, t, m, cap=cap, seed=i)
        data.append((q, t, hm, kq, kt, dm, _cnt(torch_mod, n), n))
    b = cef.FundamentalBatch(mt, [d[3] for d in data], [d[4] for d in data], [d[5] for d in data], [d[6] for d in data],
                             hypotheses=700, seed=11)
    b.run()
    torch_mod.cuda.synchronize()
    for i, (q, t, hm, kq, kt, dm, c, n) in enumerate(data):
        F, info, mask = single.findFundamental(kq, kt, dm, c, hypotheses=700, seed=11)
        assert torch_mod.equal(b.F[i].view(torch_mod.int64), F.view(torch_mod.int64)), (npairs, i, n)
        assert torch_mod.equal(b.info[i], info) and torch_mod.equal(b.mask[i], mask), (npairs, i, n)
        if i < 8:
            _compare((b.F[i], b.info[i], b.mask[i]), FR.ransac(q, t, hm, n, cap, seed=11, hyps=700), True, (npairs, i),
                     _rows(q, t, hm, n, cap))
    lists = mt.findFundamentalBatch([d[3] for d in data], [d[4] for d in data], [d[5] for d in data], [d[6] for d in data],
                                    hypotheses=700, seed=11)
    for i in range(npairs):
        assert torch_mod.equal(lists[0][i].view(torch_mod.int64), b.F[i].view(torch_mod.int64)) and torch_mod.equal(lists[2][i], b.mask[i])


def test_fundamental_queued_calls_share_the_scratch(cef, torch_mod):
    """Calls queued behind each other on one matcher and stream with changing capacities and budgets, interleaved with homography,
    mutual and guided calls (the RANSAC scratch block is shared with the homography chains and regrows on the way): every result
    equals a fresh call on a fresh matcher, bit for bit."""
    torch = torch_mod
    rng = np.random.default_rng(1840)
    from tests import mutual_reference as MR
    sets = []
    for n, cap in [(800, 900), (5000, 6000), (300, 300), (20000, 20000)]:
        q0, t0, _, _ = FR.scene(rng, n, 0.5)
        q, t, m = FR.shuffled_matches(rng, q0, t0)
        sets.append(_upload(torch, q, t, m, cap=cap, seed=n) + (_cnt(torch, n),))
    nd = 6000
    dq = torch.from_numpy(MR.random_set(rng, nd, 32)).cuda()
    dt = torch.from_numpy(MR.random_set(rng, nd, 32)).cuda()
    gq = torch.from_numpy(FR.pack_location(np.stack([rng.integers(0, 1920, nd), rng.integers(0, 1080, nd)], axis=1))).cuda()
    gt = torch.from_numpy(FR.pack_location(np.stack([rng.integers(0, 1920, nd), rng.integers(0, 1080, nd)], axis=1))).cuda()
    args = [dict(hypotheses=256, seed=1, threshold=2.0), dict(hypotheses=4096, seed=2, threshold=4.5), dict(hypotheses=64, seed=9),
            dict(hypotheses=1000, seed=3)]

    def sequence(m):
        outs = []
        for i in (0, 1):
            kq, kt, dm, _, c = sets[i]
            outs.append(m.findFundamental(kq, kt, dm, c, **args[i]))
            outs.append(m.findHomography(kq, kt, dm, c, **args[i]))
        outs.append(m.matchMutual(dq, dt, 0.9))
        kq, kt, dm, _, c = sets[2]
        outs.append(m.findFundamental(kq, kt, dm, c, **args[2]))
        outs.append(m.matchGuided(dq, gq, dt, gt, prior=outs[1][0], radius=300.0))
        kq, kt, dm, _, c = sets[3]
        outs.append(m.findHomography(kq, kt, dm, c, **args[3]))
        outs.append(m.findFundamental(kq, kt, dm, c, **args[3]))
        outs.append(m.findFundamental(kq, kt, dm, c, refine=False, **args[3]))
        return outs

    queued = sequence(cef.BFMatcher.create())
    torch.cuda.synchronize()
    for k, (o, f) in enumerate(zip(queued, sequence_one_by_one(cef, torch, sets, args, dq, dt, gq, gt))):
        if len(o) == 2:                                    # (matches, nmatches)
            n = int(o[1].item())
            assert n == int(f[1].item()) and torch.equal(o[0][:n], f[0][:n]), k
        else:
            assert torch.equal(o[0].view(torch.int64), f[0].view(torch.int64)) and torch.equal(o[1], f[1]) and torch.equal(o[2], f[2]), k


def sequence_one_by_one(cef, torch, sets, args, dq, dt, gq, gt):
    """the calls of the queued sequence, each on a fresh matcher with a synchronisation behind it"""
    def fresh():
        return cef.BFMatcher.create()
    outs = []
    for i in (0, 1):
        kq, kt, dm, _, c = sets[i]
        outs.append(fresh().findFundamental(kq, kt, dm, c, **args[i]))
        torch.cuda.synchronize()
        outs.append(fresh().findHomography(kq, kt, dm, c, **args[i]))
        torch.cuda.synchronize()
    outs.append(fresh().matchMutual(dq, dt, 0.9))
    torch.cuda.synchronize()
    kq, kt, dm, _, c = sets[2]
    outs.append(fresh().findFundamental(kq, kt, dm, c, **args[2]))
    torch.cuda.synchronize()
    outs.append(fresh().matchGuided(dq, gq, dt, gt, prior=outs[1][0], radius=300.0))
    torch.cuda.synchronize()
    kq, kt, dm, _, c = sets[3]
    outs.append(fresh().findHomography(kq, kt, dm, c, **args[3]))
    torch.cuda.synchronize()
    outs.append(fresh().findFundamental(kq, kt, dm, c, **args[3]))
    torch.cuda.synchronize()
    outs.append(fresh().findFundamental(kq, kt, dm, c, refine=False, **args[3]))
    torch.cuda.synchronize()
    return outs


def parallax_frames(nf, rows=1080, cols=1920, split=0.45, far_shift=6, near_shift=30):
    """nf frames of a sideways camera over two texture layers: the upper `split` of the frame shows the far layer, the rest the near
    one; from frame to frame the layers move by far_shift / near_shift pixels along x"""
    from tools import synth
    wide = cols + near_shift * nf
    far, near = synth.synth_frame(rows, wide, seed=1851), synth.synth_frame(rows, wide, seed=1852)
    cut = int(round(split * rows))
    return [np.ascontiguousarray(np.concatenate([far[:cut, f * far_shift:f * far_shift + cols],
                                                 near[cut:, f * near_shift:f * near_shift + cols]])) for f in range(nf)], cut


def test_fundamental_sequence_end_to_end(cef, torch_mod):
    """Consecutive frames with parallax -> Batch detectAndCompute -> MutualBatch -> HomographyBatch and FundamentalBatch on the same
    device match lists, one synchronisation.  A homography explains at most one layer (at most 60 % of the true matches), the
    epipolar model both (expected ratio >= 1.67); 1.3 leaves room for the layers' unequal texture."""
    torch = torch_mod
    rows, cols, nf, cap = 1080, 1920, 6, 5000
    frames, cut = parallax_frames(nf, rows, cols)
    imgs = [torch.from_numpy(f).cuda() for f in frames]
    det = cef.EfficientFeatures.create(cap, dtype=cef.EfficientFeatures.BAD_256)
    nbytes = det.descriptorSize()
    st = torch.cuda.Stream()
    kps = [torch.empty((5, cap), dtype=torch.float32, device="cuda") for _ in range(nf)]
    desc = [torch.empty((cap, nbytes), dtype=torch.uint8, device="cuda") for _ in range(nf)]
    cnt = [torch.full((1,), -1, dtype=torch.int32, device="cuda") for _ in range(nf)]
    torch.cuda.synchronize()
    m = cef.BFMatcher.create()
    with torch.cuda.stream(st):
        cef.Batch([det], [st], imgs, kps, desc, cnt, cap).run()
        mb = cef.MutualBatch(m, desc[:-1], desc[1:], 0.9, cnt[:-1], cnt[1:], st)
        mb.run()
        hb = cef.HomographyBatch(m, kps[:-1], kps[1:], mb.matches, mb.nmatches, stream=st)
        hb.run()
        fb = cef.FundamentalBatch(m, kps[:-1], kps[1:], mb.matches, mb.nmatches, stream=st)
        fb.run()
    torch.cuda.synchronize()
    y, x = np.mgrid[20:rows:40, 60:cols:60]
    gq = np.stack([x.ravel(), y.ravel()], axis=1)
    gt = gq - np.stack([np.where(gq[:, 1] < cut, 6, 30), np.zeros(len(gq), dtype=np.int64)], axis=1)
    for i in range(nf - 1):
        _, hi, _ = _info((hb.H[i], hb.info[i], hb.mask[i]))
        F, fi, mask = _info((fb.F[i], fb.info[i], fb.mask[i]))
        k = int(mb.nmatches[i].item())
        print("pair %d: %d matches, homography %d inliers, fundamental %d inliers" % (i, k, hi["ninliers"], fi["ninliers"]))
        assert k > 300 and hi["hypothesis"] >= 0 and fi["hypothesis"] >= 0 and fi["refined"] == 1, (i, k, hi, fi)
        assert int(mask.sum()) == fi["ninliers"] and not mask[k:].any()
        assert fi["ninliers"] >= 1.3 * hi["ninliers"], (i, fi, hi)
        assert np.abs(FR.sampson(F, gq, gt)).max() < 1.0, i          # the true motion of both layers lies on the epipolar lines
        # the reference on the downloaded inputs
        ku, kv = cef.unpack_keypoints(kps[i].cpu().numpy()), cef.unpack_keypoints(kps[i + 1].cpu().numpy())
        q = np.stack([ku["x"], ku["y"]], axis=1).astype(np.int64)
        t = np.stack([kv["x"], kv["y"]], axis=1).astype(np.int64)
        hm = mb.matches[i].cpu().numpy()
        _compare((fb.F[i], fb.info[i], fb.mask[i]), FR.ransac(q, t, hm, k, cap), True, ("sequence", i), _rows(q, t, hm, k, cap))
    # an F is no prior for guided matching: the record has the layout of a homography but predicts a line
    with pytest.raises(cef.EfxError):
        m.matchGuided(desc[0], kps[0], desc[1], kps[1], prior=fb.F[0], nq=cnt[0], nt=cnt[1])
    F1 = m.findFundamental(kps[0], kps[1], mb.matches[0], mb.nmatches[0])[0]
    with pytest.raises(cef.EfxError):
        m.matchGuided(desc[0], kps[0], desc[1], kps[1], prior=F1, nq=cnt[0], nt=cnt[1])
    assert torch.equal(F1.view(torch.int64), fb.F[0].view(torch.int64))
    m.matchGuided(desc[0], kps[0], desc[1], kps[1], prior=hb.H[0], nq=cnt[0], nt=cnt[1])          # a homography still is
    torch.cuda.synchronize()


def test_fundamental_parameter_errors_with_a_matcher(cef):
    """With a matcher every bad parameter, capacity and NULL pointer returns EFX_ERR_BAD_ARG; npairs = 0 returns EFX_OK."""
    lib = cef.lib()
    m = cef.BFMatcher.create()
    P = ctypes.c_void_p
    good = cef.RansacParams()
    lib.efx_default_ransac_params(ctypes.byref(good))

    def call(p=good, kq=P(64), cap=10, qcap=10, res=P(64), pitch=4000):
        return lib.efx_match_fundamental_async(m._h, kq, pitch, qcap, P(64), 4000, 10, P(64), None, cap, ctypes.byref(p) if p else None,
                                               res, P(64), None)
    for hyps, thr in [(0, 3.0), (65537, 3.0), (-1, 3.0), (2048, 0.0), (2048, -1.0), (2048, float("inf")), (2048, float("nan"))]:
        p = cef.RansacParams()
        p.hypotheses, p.threshold, p.seed, p.refine = hyps, thr, 0, 1
        assert call(p=p) == -1, (hyps, thr)
    assert call(cap=-1) == -1 and call(qcap=-1) == -1 and call(kq=None) == -1 and call(res=None) == -1 and call(p=None) == -1
    assert call(pitch=8) == -1 and call(res=P(68)) == -1 and call(kq=P(66)) == -1
    assert lib.efx_match_fundamental_batch_async(m._h, 0, None, 0, 0, None, 0, 0, None, None, 0, ctypes.byref(good), None, None, None) == 0
    assert lib.efx_match_fundamental_batch_async(m._h, -1, None, 0, 0, None, 0, 0, None, None, 0, ctypes.byref(good), None, None, None) == -1


def test_fundamental_check_sample(cef):
    """samples/fundamental_check.cpp (built by build()): detect, mutual match, homography and fundamental batches through the C++
    facade with one host sync; the epipolar model keeps at least 1.3 x the homography's inliers on every pair."""
    exe = os.path.join(ROOT, "cuda-efficient-features_amd", "efx_fundamental_check")
    assert os.path.exists(exe), "build() did not build the fundamental sample"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "fundamental ok" in r.stdout, r.stdout + r.stderr
