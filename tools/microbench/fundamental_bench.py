"""RANSAC fundamental-matrix verification (efx_match_fundamental_batch_async): ms per call from device
events after warm-up, the homography call (S16) and the new call alternated in one process, two passes.  The three workloads of
section 5d: (1) the 15 consecutive FHD pairs of independent synthetic scenes (BAD256, capacity 5000, device counts), detected and
mutual-matched as one batch, then both batched verifiers on those matches at 2048 hypotheses, against the batched mutual match;
(2) the same loop on 16 frames rendered from one scene through known homographies (a planar scene: F is undetermined there, the
timing is what counts); (3) one pair of 40 000 synthetic correspondences of a camera moving through a 3-D scene with 50 % outliers
at 512, 2048 and 8192 hypotheses.  --kernels-only runs workload (1)'s and (3)'s new calls a few times for a kernel trace.  Prints
one JSON line; --out FILE writes it too."""
import argparse
import json
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

import cef_loader
from tests import fundamental_reference as FR
from tests import homography_reference as HR


def timed(fn, reps):
    fn(); fn(); torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="a short run of the new calls for a kernel trace")
    args = ap.parse_args()
    cef = cef_loader.load()
    res = {}
    from tools import synth
    cap = 5000
    det = cef.EfficientFeatures.create(cap, dtype=cef.EfficientFeatures.BAD_256)
    imgs = [torch.from_numpy(synth.synth_frame(1080, 1920, seed=4000 + i)).cuda() for i in range(16)]
    kps = [torch.empty((5, cap), dtype=torch.float32, device="cuda") for _ in imgs]
    frames = [torch.empty((cap, 32), dtype=torch.uint8, device="cuda") for _ in imgs]
    counts = [torch.empty((1,), dtype=torch.int32, device="cuda") for _ in imgs]
    st = torch.cuda.current_stream()
    cef.Batch([det], [st], imgs, kps, frames, counts, cap).run()
    torch.cuda.synchronize()
    m = cef.BFMatcher.create()
    mutual = cef.MutualBatch(m, frames[:-1], frames[1:], 0.9, counts[:-1], counts[1:])
    mutual.run()
    hom = cef.HomographyBatch(m, kps[:-1], kps[1:], mutual.matches, mutual.nmatches, hypotheses=2048)
    fun = cef.FundamentalBatch(m, kps[:-1], kps[1:], mutual.matches, mutual.nmatches, hypotheses=2048)

    def three(r):
        for _ in range(2):                                  # alternate twice: the spread shows in the two figures
            r.setdefault("mutual_batch_ms", []).append(round(timed(mutual.run, args.reps), 4))
            r.setdefault("homography_batch_ms", []).append(round(timed(hom.run, args.reps), 4))
            r.setdefault("fundamental_batch_ms", []).append(round(timed(fun.run, args.reps), 4))
        hom.run(); fun.run(); torch.cuda.synchronize()
        r["matches"] = [int(n.item()) for n in mutual.nmatches]
        r["homography_inliers"] = [int(i[0].item()) for i in hom.info]
        r["fundamental_inliers"] = [int(i[0].item()) for i in fun.info]
        r["fundamental_to_homography"] = round(min(r["fundamental_batch_ms"]) / min(r["homography_batch_ms"]), 3)
        return r

    if args.kernels_only:
        for _ in range(5):
            fun.run()
        torch.cuda.synchronize()
    else:
        res["fhd_15_pairs_cap5000_bad256_2048hyp"] = three({})
        rng = np.random.default_rng(16)
        base = synth.synth_frame(1500, 2500, seed=4321)
        G = HR.frame_homographies(rng, 16)
        wimgs = [torch.from_numpy(HR.warp_frame(base, g, 1080, 1920)).cuda() for g in G]
        cef.Batch([det], [st], wimgs, kps, frames, counts, cap).run()
        torch.cuda.synchronize()
        res["fhd_15_warped_pairs_cap5000_bad256_2048hyp"] = three({})
    # one pair of 40 000 correspondences of a 3-D scene, half of them outliers
    rng = np.random.default_rng(5)
    q, t, good, _ = FR.scene(rng, 40000, 0.5)
    mt = FR.identity_matches(40000)
    kq = torch.from_numpy(FR.pack_location(q)).cuda()
    kt = torch.from_numpy(FR.pack_location(t)).cuda()
    dm = torch.from_numpy(mt).cuda()
    for hyps in (512, 2048, 8192):
        bh = cef.HomographyBatch(m, [kq], [kt], [dm], None, hypotheses=hyps)
        bf = cef.FundamentalBatch(m, [kq], [kt], [dm], None, hypotheses=hyps)
        if args.kernels_only:
            for _ in range(5):
                bf.run()
            torch.cuda.synchronize()
            continue
        rr = {"homography_ms": [], "fundamental_ms": []}
        for _ in range(2):
            rr["homography_ms"].append(round(timed(bh.run, args.reps), 4))
            rr["fundamental_ms"].append(round(timed(bf.run, args.reps), 4))
        bf.run(); torch.cuda.synchronize()
        mask = bf.mask[0].cpu().numpy().astype(bool)
        rr["inliers"] = int(bf.info[0][0].item())
        rr["recall"] = round(float((mask & good).sum() / good.sum()), 4)
        rr["precision"] = round(float((mask & good).sum() / max(mask.sum(), 1)), 4)
        rr["fundamental_to_homography"] = round(min(rr["fundamental_ms"]) / min(rr["homography_ms"]), 3)
        res[f"pair_40k_50pct_{hyps}hyp"] = rr
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
