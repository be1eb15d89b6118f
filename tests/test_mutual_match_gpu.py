"""GPU tier of mutual ratio-test matching (efx_match_mutual_async / efx_match_mutual_batch_async): every case is
compared exactly with the numpy reference (tests/mutual_reference.py, itself checked against the sample's loop in the CPU
tier).  Row counts come from device ints; rows past a count hold random bytes."""
import os
import subprocess

import numpy as np
import pytest

from tests import mutual_reference as MR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cnt(torch, n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def _knn(q, t):
    from oracle import matcher_oracle as MO
    if len(q) == 0 or len(t) == 0:
        return MO.knn2(q, t)
    return MO.knn2_c(q, t)


def _ref(q, t, ratios):
    i12, d12 = _knn(q, t)
    i21, d21 = _knn(t, q)
    return {r: MR.from_knn(i12, d12, i21, d21, r) for r in ratios}


def _got(matches, n):
    k = int(n.item())
    return matches[:k].cpu().numpy()


SIZES = [0, 1, 2, 127, 128, 129, 1000]
RATIOS = [0.7, 0.9, 1.0]


@pytest.mark.parametrize("nbytes", [32, 64])
def test_mutual_random_sets(cef, torch_mod, nbytes):
    """All (nq, nt) of {0, 1, 2, 127, 128, 129, 1000} (both sides of the popcount / matrix-core switch at 128) and the large
    sets around 40 000, at three ratios."""
    rng = np.random.default_rng(1500 + nbytes)
    m = cef.BFMatcher.create()
    cases = [(a, b) for a in SIZES for b in SIZES] + [(40000, 40000), (40000, 1000), (1000, 40000), (129, 40000), (40000, 2)]
    for nq, nt in cases:
        q, t = MR.random_set(rng, nq, nbytes), MR.random_set(rng, nt, nbytes)
        dq, dt = _dev(torch_mod, q.reshape(nq, nbytes)), _dev(torch_mod, t.reshape(nt, nbytes))
        want = _ref(q, t, RATIOS)
        for r in RATIOS:
            got = _got(*m.matchMutual(dq, dt, r))
            assert np.array_equal(got, want[r]), (nbytes, nq, nt, r, got.shape, want[r].shape)


@pytest.mark.parametrize("distinct", [3, 17, 200])
def test_mutual_tie_heavy_sets(cef, torch_mod, distinct):
    """Few distinct descriptors: every distance ties many times over; ties go to the lower index in both directions."""
    rng = np.random.default_rng(1600 + distinct)
    m = cef.BFMatcher.create()
    for nbytes in (32, 64):
        for nq, nt in [(129, 127), (1000, 1000), (5000, 3000), (100, 1000)]:
            q, t = MR.random_set(rng, nq, nbytes, distinct), MR.random_set(rng, nt, nbytes, distinct)
            want = _ref(q, t, RATIOS)
            for r in RATIOS:
                got = _got(*m.matchMutual(_dev(torch_mod, q), _dev(torch_mod, t), r))
                assert np.array_equal(got, want[r]), (nbytes, nq, nt, r, distinct)


def test_mutual_ratio_one_is_crosscheck(cef, torch_mod):
    """ratio = 1: exactly the kept pairs of efx_match_crosscheck_async, compacted."""
    rng = np.random.default_rng(1700)
    m = cef.BFMatcher.create()
    mc = cef.BFMatcher.create(cef.BFMatcher.NORM_HAMMING, True)
    for nbytes, nq, nt, distinct in [(32, 40000, 40000, None), (64, 3000, 5000, None), (32, 1000, 900, 50), (64, 100, 60, None)]:
        dq = _dev(torch_mod, MR.random_set(rng, nq, nbytes, distinct))
        dt = _dev(torch_mod, MR.random_set(rng, nt, nbytes, distinct))
        cm, cd = mc.match(dq, dt)
        cm, cd = cm.cpu().numpy(), cd.cpu().numpy()
        keep = np.nonzero(cm >= 0)[0]
        want = np.stack([keep, cm[keep], cd[keep]], axis=1).astype(np.int32).reshape(-1, 3)
        assert np.array_equal(_got(*m.matchMutual(dq, dt, 1.0)), want), (nbytes, nq, nt)


def test_mutual_device_counts_below_capacity(cef, torch_mod):
    """Counts on the device below the capacity, random bytes past them: the result equals the call on the sliced tensors (and
    the reference); a negative count reads as 0, one above the capacity as the capacity."""
    rng = np.random.default_rng(1800)
    m = cef.BFMatcher.create()
    for nbytes, qcap, tcap, nq, nt in [(32, 1000, 1000, 700, 300), (64, 40000, 40000, 30000, 25000), (32, 300, 5000, 120, 4000),
                                       (64, 2000, 100, 1999, 1), (32, 2000, 2000, 0, 1500), (32, 256, 256, 256, 255)]:
        q, t = MR.random_set(rng, qcap, nbytes), MR.random_set(rng, tcap, nbytes)
        dq, dt = _dev(torch_mod, q), _dev(torch_mod, t)
        want = _ref(q[:nq], t[:nt], [0.9])[0.9]
        got = _got(*m.matchMutual(dq, dt, 0.9, nq=_cnt(torch_mod, nq), nt=_cnt(torch_mod, nt)))
        sliced = _got(*m.matchMutual(dq[:nq].contiguous() if nq else dq[:1], dt[:nt].contiguous() if nt else dt[:1], 0.9,
                                     nq=None if nq else _cnt(torch_mod, 0), nt=None if nt else _cnt(torch_mod, 0)))
        assert np.array_equal(got, want), (nbytes, qcap, tcap, nq, nt)
        assert np.array_equal(sliced, want), (nbytes, qcap, tcap, nq, nt)
    q, t = MR.random_set(rng, 500, 32), MR.random_set(rng, 400, 32)
    dq, dt = _dev(torch_mod, q), _dev(torch_mod, t)
    assert int(m.matchMutual(dq, dt, 0.9, nq=_cnt(torch_mod, -5))[1].item()) == 0
    got = _got(*m.matchMutual(dq, dt, 0.9, nq=_cnt(torch_mod, 10 ** 6), nt=_cnt(torch_mod, 10 ** 6)))
    assert np.array_equal(got, _ref(q, t, [0.9])[0.9])


def test_mutual_variant_knobs_agree(cef, torch_mod, monkeypatch):
    """EFX_MATCH_NO_MFMA (popcount kernel) and EFX_MATCH_NO_FP4 (int8 matrix cores), read when a matcher is created, give the
    default (FP4) path's output."""
    rng = np.random.default_rng(1900)
    m_fp4 = cef.BFMatcher.create()
    monkeypatch.setenv("EFX_MATCH_NO_FP4", "1")
    m_i8 = cef.BFMatcher.create()
    monkeypatch.delenv("EFX_MATCH_NO_FP4")
    monkeypatch.setenv("EFX_MATCH_NO_MFMA", "1")
    m_pop = cef.BFMatcher.create()
    monkeypatch.delenv("EFX_MATCH_NO_MFMA")
    for nbytes, nq, nt, distinct in [(32, 5000, 6000, None), (64, 5000, 4000, None), (32, 3000, 3000, 20), (64, 129, 1000, None)]:
        q, t = MR.random_set(rng, nq, nbytes, distinct), MR.random_set(rng, nt, nbytes, distinct)
        dq, dt = _dev(torch_mod, q), _dev(torch_mod, t)
        cq, ct = _cnt(torch_mod, nq - 7), _cnt(torch_mod, nt - 3)
        outs = [_got(*mm.matchMutual(dq, dt, 0.9, nq=cq, nt=ct)) for mm in (m_fp4, m_i8, m_pop)]
        want = _ref(q[:nq - 7], t[:nt - 3], [0.9])[0.9]
        for o in outs:
            assert np.array_equal(o, want), (nbytes, nq, nt, distinct)


def test_mutual_queued_calls_growing_capacities(cef, torch_mod):
    """Calls queued on one matcher and one stream with growing capacities and no host sync between them: every input is uploaded
    first, the device is kept busy, then the six calls go back to back, so each regrow of the matcher's scratch happens while the
    calls before it are still queued or running.  Every result is right (a regrow waits for that work before the old block is
    released)."""
    rng = np.random.default_rng(2000)
    m = cef.BFMatcher.create()
    cases = []
    for nbytes, n in [(32, 50), (32, 300), (64, 2000), (32, 8000), (64, 20000), (32, 40000)]:
        q, t = MR.random_set(rng, n, nbytes), MR.random_set(rng, n + 17, nbytes)
        cases.append((q, t, _dev(torch_mod, q), _dev(torch_mod, t), _cnt(torch_mod, n - 1)))
    torch_mod.cuda.synchronize()
    torch_mod.cuda._sleep(int(100e6))                     # the calls below are queued behind this
    outs = [m.matchMutual(dq, dt, 0.8, nq=cq) for _, _, dq, dt, cq in cases]
    torch_mod.cuda.synchronize()
    for (q, t, _, _, _), (mt, nm) in zip(cases, outs):
        assert np.array_equal(_got(mt, nm), _ref(q[:len(q) - 1], t, [0.8])[0.8]), len(q)


def test_mutual_call_does_not_wait_for_the_stream(cef, torch_mod):
    """A call with capacities the matcher has seen returns while its stream is still busy (no host sync inside)."""
    import time
    rng = np.random.default_rng(2100)
    m = cef.BFMatcher.create()
    dq, dt = _dev(torch_mod, MR.random_set(rng, 5000, 32)), _dev(torch_mod, MR.random_set(rng, 5000, 32))
    cq = _cnt(torch_mod, 4000)
    m.matchMutual(dq, dt, 0.9, nq=cq)
    torch_mod.cuda.synchronize()
    torch_mod.cuda._sleep(int(500e6))                     # a few hundred ms of device time, queued before the call
    t0 = time.perf_counter()
    m.matchMutual(dq, dt, 0.9, nq=cq)
    host = time.perf_counter() - t0
    t1 = time.perf_counter()
    torch_mod.cuda.synchronize()
    rest = time.perf_counter() - t1
    assert rest > 0.03 and host < rest / 2, (host, rest)


def test_mutual_batch_on_detected_frames(cef, torch_mod):
    """The sequence loop without host sync: a Batch detectAndCompute of 19 FHD frames (two launch chains), then matchMutualBatch
    on the pairs (i, i + 1) straight from the device counts (18 pairs: two chains of the matcher too); downloaded at the end.
    Every pair equals the reference on the downloaded descriptors and counts, and the single-pair call, bit for bit."""
    from tools import synth
    torch = torch_mod
    nf, cap = 19, 5000
    imgs = [_dev(torch, synth.synth_frame(1080, 1920, seed=3000 + i // 2 * 2)) for i in range(nf)]   # pairs of equal frames too
    det = cef.EfficientFeatures.create(cap, dtype=cef.EfficientFeatures.BAD_256)
    nbytes = det.descriptorSize()
    st = torch.cuda.Stream()
    kps = [torch.empty((5, cap), dtype=torch.float32, device="cuda") for _ in range(nf)]
    desc = [torch.randint(0, 256, (cap, nbytes), dtype=torch.uint8, device="cuda") for _ in range(nf)]   # garbage past the counts
    cnt = [torch.full((1,), -1, dtype=torch.int32, device="cuda") for _ in range(nf)]
    torch.cuda.synchronize()
    m = cef.BFMatcher.create()
    with torch.cuda.stream(st):
        cef.Batch([det], [st], imgs, kps, desc, cnt, cap).run()
        mb = cef.MutualBatch(m, desc[:-1], desc[1:], 0.9, cnt[:-1], cnt[1:], st)
        mb.run()
    torch.cuda.synchronize()
    ns = [int(c.item()) for c in cnt]
    assert min(ns) > 500, ns
    hd = [d.cpu().numpy() for d in desc]
    single = cef.BFMatcher.create()
    for i in range(nf - 1):
        want = _ref(hd[i][:ns[i]], hd[i + 1][:ns[i + 1]], [0.9])[0.9]
        got = _got(mb.matches[i], mb.nmatches[i])
        assert np.array_equal(got, want), i
        one = _got(*single.matchMutual(desc[i], desc[i + 1], 0.9, nq=cnt[i], nt=cnt[i + 1]))
        assert np.array_equal(one, got), i
        if i % 2 == 0:
            assert len(got) > ns[i] // 2                      # equal frames: most keypoints match themselves


def test_mutual_batch_mixed_pairs(cef, torch_mod):
    """matchMutualBatch over pairs that share matrices in both roles, with and without counts, popcount-sized and large."""
    rng = np.random.default_rng(2200)
    m = cef.BFMatcher.create()
    for nbytes, cap in [(32, 100), (64, 3000)]:
        hs = [MR.random_set(rng, cap, nbytes, 40 if k % 3 == 0 else None) for k in range(6)]
        ds = [_dev(torch_mod, h) for h in hs]
        ns = [cap - 13 * k for k in range(6)]
        cs = [_cnt(torch_mod, n) for n in ns]
        pairs = [(0, 1), (1, 2), (2, 0), (3, 3), (4, 5), (5, 4), (1, 2)]
        outs, nouts = m.matchMutualBatch([ds[a] for a, _ in pairs], [ds[b] for _, b in pairs], 0.85,
                                         [cs[a] for a, _ in pairs], [cs[b] for _, b in pairs])
        for (a, b), mt, nm in zip(pairs, outs, nouts):
            assert np.array_equal(_got(mt, nm), _ref(hs[a][:ns[a]], hs[b][:ns[b]], [0.85])[0.85]), (nbytes, a, b)


def test_mutual_batch_many_chains_reuses_and_refills_slots(cef, torch_mod):
    """40 pairs (three chains of the matcher) over 41 matrices: a sequence (k, k + 1), so the shared frame of two chains is
    carried over in its expansion slot and every other slot is refilled chain after chain, then pairs whose matrices come back
    after a chain without them, and a matrix against itself; counts on the device.  Every pair equals the reference and the
    single-pair call."""
    rng = np.random.default_rng(2300)
    m = cef.BFMatcher.create()
    single = cef.BFMatcher.create()
    for nbytes, cap in [(32, 300), (64, 130)]:
        hs = [MR.random_set(rng, cap, nbytes, 60 if k % 4 == 0 else None) for k in range(41)]
        ds = [_dev(torch_mod, h) for h in hs]
        ns = [cap - (7 * k) % 100 for k in range(41)]
        cs = [_cnt(torch_mod, n) for n in ns]
        pairs = [(k, k + 1) for k in range(36)] + [(0, 40), (40, 2), (5, 5), (33, 20)]
        outs, nouts = m.matchMutualBatch([ds[a] for a, _ in pairs], [ds[b] for _, b in pairs], 0.9,
                                         [cs[a] for a, _ in pairs], [cs[b] for _, b in pairs])
        for (a, b), mt, nm in zip(pairs, outs, nouts):
            got = _got(mt, nm)
            assert np.array_equal(got, _ref(hs[a][:ns[a]], hs[b][:ns[b]], [0.9])[0.9]), (nbytes, a, b)
            assert np.array_equal(got, _got(*single.matchMutual(ds[a], ds[b], 0.9, nq=cs[a], nt=cs[b]))), (nbytes, a, b)


def test_sequence_check_sample(cef):
    """samples/sequence_check.cpp (built by build()): batched detectAndCompute -> mutual matches of consecutive frames with no
    host sync until the end, checked against a host-side filter of knnMatch results."""
    exe = os.path.join(ROOT, "cuda-efficient-features_amd", "efx_sequence_check")
    assert os.path.exists(exe), "build() did not build the sequence sample"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sequence ok" in r.stdout, r.stdout + r.stderr
