"""Guided (spatially gated) mutual matching (efx_match_guided_batch_async): ms per call from device events
after warm-up, against the brute-force mutual match (efx_match_mutual_batch_async) on identical inputs in the same process,
alternated twice.  (1) One pair of 40 000 x 40 000 descriptors at 256 and 512 bit, locations uniform over 7680 x 4320 (trains =
the queries moved by up to 3 px), radius 16, no prior, with and without the frame size hint.  (2) The 15 consecutive FHD pairs of
DESIGN section 5c (16 synthetic frames detected and described as one batch: BAD256, capacity 5000, device counts), radius 16, no
prior.  (3) 15 pairs of 16 FHD frames rendered from one scene through known homographies: radius 16 without a prior, and radius 8
with the homographies of a first brute-force pass as priors, straight from the device.  Reports the candidates per query (numpy
reference, tests/guided_reference.py) and the rows kept.  Prints one JSON line; --out FILE writes it too."""
import argparse
import json
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

import cef_loader
from tests import guided_reference as GR
from tests import homography_reference as HR


def timed(fn, reps):
    fn(); fn(); torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(r, mutual, guided, reps):
    """{name: batch} for the guided variants: the brute-force call and every variant, twice in turn (the spread shows)"""
    for _ in range(2):
        r.setdefault("mutual_ms", []).append(round(timed(mutual.run, reps), 4))
        for name, g in guided.items():
            r.setdefault(name + "_ms", []).append(round(timed(g.run, reps), 4))
    for name, g in guided.items():
        r[name + "_speedup"] = round(min(r["mutual_ms"]) / min(r[name + "_ms"]), 2)


def unpack(cef, kps, n):
    u = cef.unpack_keypoints(kps.cpu().numpy())
    return np.stack([u["x"][:n], u["y"][:n]], axis=1).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cef = cef_loader.load()
    res = {}
    m = cef.BFMatcher.create()
    # (1) one large pair
    n = 40000
    for nbytes in (32, 64):
        rng = np.random.default_rng(17 + nbytes)
        q = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
        t = q.copy()
        flips = rng.integers(0, nbytes * 8, (n, 24))
        for k in range(24):
            t[np.arange(n), flips[:, k] >> 3] ^= (1 << (flips[:, k] & 7)).astype(np.uint8)
        lq = np.stack([rng.integers(0, 7680, n), rng.integers(0, 4320, n)], axis=1)
        perm = rng.permutation(n)
        t, lt = t[perm], np.clip(lq + rng.integers(-3, 4, (n, 2)), 0, [7679, 4319])[perm]
        dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
        kq, kt = torch.from_numpy(GR.pack_keypoints(lq)).cuda(), torch.from_numpy(GR.pack_keypoints(lt)).cuda()
        mutual = cef.MutualBatch(m, [dq], [dt], 0.9)
        guided = {"guided_hint": cef.GuidedBatch(m, [dq], [kq], [dt], [kt], None, radius=16.0, width=7680, height=4320),
                  "guided_nohint": cef.GuidedBatch(m, [dq], [kq], [dt], [kt], None, radius=16.0)}
        r = {}
        alternate(r, mutual, guided, args.reps)
        torch.cuda.synchronize()
        r["mutual_rows"] = int(mutual.nmatches[0].item())
        r["guided_rows"] = int(guided["guided_hint"].nmatches[0].item())
        r["candidates_per_query"] = round(len(GR.candidates(lq, lt, None, None, None, 16.0, -1)[0]) / n, 2)
        res[f"pair_40k_{nbytes * 8}bit_8k_uniform_r16"] = r
    # (2) the 15 FHD pairs of section 5c, (3) 15 pairs of one scene
    from tools import synth
    cap = 5000
    det = cef.EfficientFeatures.create(cap, dtype=cef.EfficientFeatures.BAD_256)
    kps = [torch.empty((5, cap), dtype=torch.float32, device="cuda") for _ in range(16)]
    frames = [torch.empty((cap, 32), dtype=torch.uint8, device="cuda") for _ in range(16)]
    counts = [torch.empty((1,), dtype=torch.int32, device="cuda") for _ in range(16)]
    st = torch.cuda.current_stream()
    mutual = cef.MutualBatch(m, frames[:-1], frames[1:], 0.9, counts[:-1], counts[1:])
    hom = cef.HomographyBatch(m, kps[:-1], kps[1:], mutual.matches, mutual.nmatches, hypotheses=2048)
    ident = cef.GuidedBatch(m, frames[:-1], kps[:-1], frames[1:], kps[1:], None, radius=16.0, width=1920, height=1080,
                            nqs=counts[:-1], nts=counts[1:])
    prior = cef.GuidedBatch(m, frames[:-1], kps[:-1], frames[1:], kps[1:], hom.H, radius=8.0, width=1920, height=1080,
                            nqs=counts[:-1], nts=counts[1:])
    rng = np.random.default_rng(16)
    base = synth.synth_frame(1500, 2500, seed=4321)
    G = HR.frame_homographies(rng, 16)
    sets = {"fhd_15_pairs_cap5000_bad256": [synth.synth_frame(1080, 1920, seed=4000 + i) for i in range(16)],
            "fhd_15_warped_pairs_cap5000_bad256": [HR.warp_frame(base, g, 1080, 1920) for g in G]}
    for name, imgs in sets.items():
        cef.Batch([det], [st], [torch.from_numpy(i).cuda() for i in imgs], kps, frames, counts, cap).run()
        mutual.run(); hom.run()
        torch.cuda.synchronize()
        warped = "warped" in name
        r = {}
        alternate(r, mutual, {"guided_r16_identity": ident, "guided_r8_prior": prior} if warped else {"guided_r16_identity": ident},
                  args.reps)
        torch.cuda.synchronize()
        cnt = [int(c.item()) for c in counts]
        r["keypoints"] = cnt
        r["mutual_rows"] = [int(x.item()) for x in mutual.nmatches]
        r["guided_r16_identity_rows"] = [int(x.item()) for x in ident.nmatches]
        loc = [unpack(cef, kps[i], cnt[i]) for i in range(16)]
        r["candidates_per_query_r16_identity"] = round(
            sum(len(GR.candidates(loc[i], loc[i + 1], None, None, None, 16.0, -1)[0]) for i in range(15)) / max(sum(cnt[:-1]), 1), 2)
        if warped:
            r["guided_r8_prior_rows"] = [int(x.item()) for x in prior.nmatches]
            within = [[], []]
            for i in range(15):
                truth = G[i + 1] @ np.linalg.inv(G[i])
                for k, b in enumerate((mutual, prior)):
                    rows = b.matches[i][:int(b.nmatches[i].item())].cpu().numpy()
                    e = HR.project(truth, loc[i][rows[:, 0]].astype(np.float64)) - loc[i + 1][rows[:, 1]]
                    within[k].append(int((np.hypot(e[:, 0], e[:, 1]) <= 3.0).sum()))
            r["mutual_rows_within_3px_of_truth"] = within[0]
            r["guided_r8_prior_rows_within_3px_of_truth"] = within[1]
            r["candidates_per_query_r8_prior"] = round(
                sum(len(GR.candidates(loc[i], loc[i + 1], None, None, (hom.H[i].cpu().numpy(), int(hom.info[i][1].item())), 8.0, -1)[0])
                    for i in range(15)) / max(sum(cnt[:-1]), 1), 2)
        res[name] = r
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
