"""Numpy reference of the mutual ratio-test filter (efx_match_mutual_async) and a literal O(nq nt) restatement
of the loop of samples/sample_image_sequence.cpp:114-137 that checks it (test infrastructure only)."""
import numpy as np

from oracle import matcher_oracle as MO


def mutual(query, train, ratio, knn2=MO.knn2):
    """knn2 in both directions, then the sample's three checks: (queryIdx, trainIdx, distance) rows in ascending queryIdx.
    A missing second neighbour passes its ratio test (S15); a count of 0 on either side gives no rows."""
    query = np.asarray(query, np.uint8)
    train = np.asarray(train, np.uint8)
    if len(query) == 0 or len(train) == 0:
        return np.zeros((0, 3), np.int32)
    i12, d12 = knn2(query, train)
    i21, d21 = knn2(train, query)
    return from_knn(i12, d12, i21, d21, ratio)


def from_knn(i12, d12, i21, d21, ratio):
    """The filter on knn2 results of both directions (nq x 2 and nt x 2 index / distance arrays, -1 where missing)."""
    if len(i12) == 0 or len(i21) == 0:
        return np.zeros((0, 3), np.int32)
    j = i12[:, 0]
    keep = j >= 0
    js = np.where(keep, j, 0)
    r12 = (i12[:, 1] < 0) | ~(d12[:, 0].astype(np.float64) > ratio * d12[:, 1].astype(np.float64))
    r21 = (i21[js, 1] < 0) | ~(d21[js, 0].astype(np.float64) > ratio * d21[js, 1].astype(np.float64))
    keep &= r12 & r21 & (i21[js, 0] == np.arange(len(i12)))
    q = np.nonzero(keep)[0]
    return np.stack([q, j[q], d12[q, 0]], axis=1).astype(np.int32).reshape(-1, 3)


def sample_loop(query, train, ratio):
    """The sample's loop, transliterated: knnMatch(k = 2) by a sequential scan with a strict `<` in both directions, then
    for m12 in matches12: m21 = matches21[m12[0].trainIdx]; the two uniqueness checks and the cross check, in double."""
    query = [bytes(np.asarray(r, np.uint8)) for r in query]
    train = [bytes(np.asarray(r, np.uint8)) for r in train]

    def dist(a, b):
        return sum(bin(x ^ y).count("1") for x, y in zip(a, b))

    def knn_match(qs, ts):
        out = []
        for qi, q in enumerate(qs):
            best = []                                   # [(distance, trainIdx)], at most two, nearest first
            for ti, t in enumerate(ts):
                d = dist(q, t)
                if not best or d < best[0][0]:
                    best = [(d, ti)] + best[:1]
                elif len(best) < 2 or d < best[1][0]:
                    best = best[:1] + [(d, ti)]
            out.append([(qi, ti, float(d)) for d, ti in best])     # DMatch(queryIdx, trainIdx, distance as float)
        return out

    if not query or not train:
        return np.zeros((0, 3), np.int32)
    matches12, matches21 = knn_match(query, train), knn_match(train, query)
    uniqueness = float(ratio)
    rows = []
    for m12 in matches12:
        m21 = matches21[m12[0][1]]
        if len(m12) > 1 and m12[0][2] > uniqueness * m12[1][2]:
            continue
        if len(m21) > 1 and m21[0][2] > uniqueness * m21[1][2]:
            continue
        if m21[0][1] != m12[0][0]:
            continue
        rows.append((m12[0][0], m12[0][1], int(m12[0][2])))
    return np.array(rows, np.int32).reshape(-1, 3)


def random_set(rng, n, nbytes, distinct=None):
    """n random descriptors; with `distinct`, drawn from that many distinct rows (tie-heavy)."""
    if distinct is None:
        return rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
    pool = rng.integers(0, 256, (max(distinct, 1), nbytes), dtype=np.uint8)
    return pool[rng.integers(0, len(pool), n)]
