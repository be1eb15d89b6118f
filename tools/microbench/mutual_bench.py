"""Mutual ratio-test matching (efx_match_mutual_async / efx_match_mutual_batch_async): ms per call from device events after
warm-up.  (1) 40 000 x 40 000 random descriptors at 512 and 256 bits: matchMutual against the host-count calls it replaces
(knnMatch in both directions, and the cross check); (2) 15 pairs of consecutive FHD frames (synthetic, detected and described
as one batch: BAD256, capacity 5000, device counts): one batched call against 15 single-pair calls.  Prints one JSON line; --out FILE writes it too."""
import argparse
import json
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

import cef_loader


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
    args = ap.parse_args()
    cef = cef_loader.load()
    rng = np.random.default_rng(1)
    res = {}
    for nbytes in (64, 32):
        q = torch.from_numpy(rng.integers(0, 256, size=(40000, nbytes), dtype=np.uint8)).cuda()
        t = torch.from_numpy(rng.integers(0, 256, size=(40000, nbytes), dtype=np.uint8)).cuda()
        m = cef.BFMatcher.create()
        mc = cef.BFMatcher.create(cef.BFMatcher.NORM_HAMMING, True)
        r = {}
        for _ in range(2):                                  # alternate the variants twice: the spread shows in the two figures
            r.setdefault("mutual_ms", []).append(timed(lambda: m.matchMutual(q, t, 0.9), args.reps))
            r.setdefault("knn2_ms", []).append(timed(lambda: m.knnMatch(q, t, 2), args.reps))
            r.setdefault("knn2_x2_ms", []).append(timed(lambda: (m.knnMatch(q, t, 2), m.knnMatch(t, q, 2)), args.reps))
            r.setdefault("crosscheck_ms", []).append(timed(lambda: mc.match(q, t), args.reps))
        res[f"{nbytes * 8}bit_40k"] = {k: [round(x, 4) for x in v] for k, v in r.items()}
    # 15 pairs of consecutive FHD frames: 16 synthetic 1920 x 1080 frames through one batched detectAndCompute (BAD256, capacity
    # 5000), their descriptors and DEVICE counts straight into the matcher
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
    batch = cef.MutualBatch(m, frames[:-1], frames[1:], 0.9, counts[:-1], counts[1:])
    singles = lambda: [m.matchMutual(frames[i], frames[i + 1], 0.9, nq=counts[i], nt=counts[i + 1]) for i in range(15)]
    r = {"keypoints": [int(c.item()) for c in counts]}
    for _ in range(2):
        r.setdefault("batched_ms", []).append(timed(batch.run, args.reps))
        r.setdefault("singles_ms", []).append(timed(singles, args.reps))
    batch.run(); torch.cuda.synchronize()
    r["matches"] = [int(n.item()) for n in batch.nmatches]
    res["fhd_15_pairs_cap5000_bad256"] = {k: [round(x, 4) for x in v] for k, v in r.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
