"""RANSAC homography verification (efx_match_homography_batch_async): ms per call from device events after
warm-up.  (1) The 15 consecutive FHD pairs of DESIGN section 5c (16 synthetic frames detected and described as one batch: BAD256,
capacity 5000, device counts), mutual-matched as one batch, then the batched homography call on those matches at 2048 hypotheses,
against the batched mutual match in the same process.  Those frames are independent scenes, so their matches are mostly
random; the same loop then runs on 16 frames rendered from one scene through known homographies, where most matches are
inliers; (2) one pair of 40 000 synthetic correspondences with 50 % outliers at 512, 2048 and 8192 hypotheses; (3) the numpy reference (tests/homography_reference.py) on that pair at 2048 hypotheses, a CPU
reference only.  Prints one JSON line; --out FILE writes it too."""
import argparse
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

import cef_loader
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
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy reference timing")
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
    r = {}
    for _ in range(2):                                      # alternate twice: the spread shows in the two figures
        r.setdefault("mutual_batch_ms", []).append(round(timed(mutual.run, args.reps), 4))
        r.setdefault("homography_batch_ms", []).append(round(timed(hom.run, args.reps), 4))
    hom.run(); torch.cuda.synchronize()
    r["matches"] = [int(n.item()) for n in mutual.nmatches]
    r["inliers"] = [int(i[0].item()) for i in hom.info]
    res["fhd_15_pairs_cap5000_bad256_2048hyp"] = r
    # the same loop on 16 FHD frames rendered from ONE scene through known homographies (consecutive frames overlap, as in a video):
    # the realistic case -- most mutual matches are inliers and the refit runs on them
    rng = np.random.default_rng(16)
    base = synth.synth_frame(1500, 2500, seed=4321)
    G = HR.frame_homographies(rng, 16)
    wimgs = [torch.from_numpy(HR.warp_frame(base, g, 1080, 1920)).cuda() for g in G]
    cef.Batch([det], [st], wimgs, kps, frames, counts, cap).run()
    torch.cuda.synchronize()
    r = {}
    for _ in range(2):
        r.setdefault("mutual_batch_ms", []).append(round(timed(mutual.run, args.reps), 4))
        r.setdefault("homography_batch_ms", []).append(round(timed(hom.run, args.reps), 4))
    hom.run(); torch.cuda.synchronize()
    r["matches"] = [int(n.item()) for n in mutual.nmatches]
    r["inliers"] = [int(i[0].item()) for i in hom.info]
    r["worst_corner_err_px"] = round(max(float(np.abs(HR.project(hom.H[i].cpu().numpy(), HR.corners())
                                                      - HR.project(G[i + 1] @ np.linalg.inv(G[i]), HR.corners())).max())
                                         for i in range(15)), 4)
    res["fhd_15_warped_pairs_cap5000_bad256_2048hyp"] = r
    # one pair of 40 000 correspondences, half of them outliers
    rng = np.random.default_rng(5)
    H = HR.true_homography(rng)
    q, t, mt = HR.synth_matches(rng, 40000, 0.5, H)
    kq = torch.from_numpy(HR.pack_location(q)).cuda()
    kt = torch.from_numpy(HR.pack_location(t)).cuda()
    dm = torch.from_numpy(mt).cuda()
    for hyps in (512, 2048, 8192):
        b = cef.HomographyBatch(m, [kq], [kt], [dm], None, hypotheses=hyps)
        rr = {"ms": [round(timed(b.run, args.reps), 4) for _ in range(2)]}
        b.run(); torch.cuda.synchronize()
        rr["inliers"] = int(b.info[0][0].item())
        rr["corner_err_px"] = round(float(np.abs(HR.project(b.H[0].cpu().numpy(), HR.corners()) - HR.project(H, HR.corners())).max()), 4)
        res[f"pair_40k_50pct_{hyps}hyp"] = rr
    if not args.no_cpu:
        t0 = time.perf_counter()
        HR.ransac(q, t, mt, None, len(mt), hyps=2048)
        res["cpu_numpy_reference_40k_2048hyp_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
