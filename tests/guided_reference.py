"""Numpy restatement of guided (spatially gated) mutual matching (efx_match_guided_async) and a literal per-pair
loop that checks it (test infrastructure only).  The gate is a dense boolean matrix, evaluated in blocks of query rows so that
40 000 x 40 000 fits in memory; nothing here knows about cells or grids."""
import math

import numpy as np

from tests import mutual_reference as MR


def predict(loc_q, prior):
    """S17 step 2: (px, py, valid) per query, or None when the prior holds no model.  prior: None (identity) or (H, hypothesis)."""
    x = np.asarray(loc_q, np.int64).reshape(-1, 2)[:, 0].astype(np.float64)
    y = np.asarray(loc_q, np.int64).reshape(-1, 2)[:, 1].astype(np.float64)
    if prior is None:
        return x, y, np.ones(len(x), bool)
    H, hyp = prior
    if hyp < 0:
        return None
    H = np.asarray(H, np.float64).reshape(9)
    with np.errstate(all="ignore"):
        X = (H[0] * x + H[1] * y) + H[2]
        Y = (H[3] * x + H[4] * y) + H[5]
        W = (H[6] * x + H[7] * y) + H[8]
        px, py = X / W, Y / W
        valid = (W > 0) & np.isfinite(px) & np.isfinite(py)
    return px, py, valid


def gate_block(px, py, valid, loc_t, oct_q, oct_t, radius, max_octave_diff):
    """S17 step 3 for the queries given: a len(px) x nt boolean matrix"""
    R = float(np.float32(radius))
    xt = loc_t[:, 0].astype(np.float64)
    yt = loc_t[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        g = (np.abs(xt[None, :] - px[:, None]) <= R) & (np.abs(yt[None, :] - py[:, None]) <= R) & valid[:, None]
        if max_octave_diff >= 0:
            g &= np.abs(oct_q.astype(np.int32)[:, None] - oct_t.astype(np.int32)[None, :]) <= np.int32(max_octave_diff)
    return g


def candidates(loc_q, loc_t, oct_q, oct_t, prior, radius, max_octave_diff, block=None):
    """The candidate set C as index arrays (i, j), in ascending (i, j)"""
    loc_q = np.asarray(loc_q, np.int64).reshape(-1, 2)
    loc_t = np.asarray(loc_t, np.int64).reshape(-1, 2)
    nq, nt = len(loc_q), len(loc_t)
    pr = predict(loc_q, prior)
    if pr is None or nq == 0 or nt == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    px, py, valid = pr
    oct_q = np.zeros(nq, np.int32) if oct_q is None else np.asarray(oct_q, np.int32)
    oct_t = np.zeros(nt, np.int32) if oct_t is None else np.asarray(oct_t, np.int32)
    # The dense gate, one block of query rows at a time.  To keep 40 000 x 40 000 affordable the rows are visited in the order of
    # their predicted x and a block looks only at the trains whose x lies within the block's range widened by radius + 1 (every
    # other train fails the x comparison of the gate); inside that slice the gate is evaluated exactly, pair by pair.
    R = float(np.float32(radius))
    block = block or 512
    rows_all = np.argsort(np.where(valid, px, np.inf), kind="stable")[:int(valid.sum())]
    xt = loc_t[:, 0].astype(np.float64)
    t_order = np.argsort(xt, kind="stable")
    xts = xt[t_order]
    ii, jj = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for a0 in range(0, len(rows_all), block):
        rows = rows_all[a0:a0 + block]
        c0 = np.searchsorted(xts, px[rows[0]] - R - 1.0, "left")
        c1 = np.searchsorted(xts, px[rows[-1]] + R + 1.0, "right")
        cols = t_order[c0:c1]
        a, b = np.nonzero(gate_block(px[rows], py[rows], valid[rows], loc_t[cols], oct_q[rows], oct_t[cols], radius, max_octave_diff))
        ii.append(rows[a])
        jj.append(cols[b])
    ii, jj = np.concatenate(ii), np.concatenate(jj)
    order = np.lexsort((jj, ii))
    return ii[order], jj[order]


def _best2(owner, other, dist, n):
    """per owner row: the best two (dist, other) pairs among its candidates, ties to the lower index; -1 where missing"""
    idx = np.full((n, 2), -1, np.int32)
    dd = np.full((n, 2), -1, np.int32)
    if len(owner) == 0:
        return idx, dd
    order = np.lexsort((other, dist, owner))
    o, t, d = owner[order], other[order], dist[order]
    first = np.concatenate([[True], o[1:] != o[:-1]])
    pos = np.arange(len(o)) - np.maximum.accumulate(np.where(first, np.arange(len(o)), 0))
    for k in (0, 1):
        sel = pos == k
        idx[o[sel], k] = t[sel]
        dd[o[sel], k] = d[sel]
    return idx, dd


def hamming_pairs(query, train, ii, jj):
    q = np.ascontiguousarray(query, np.uint8)
    t = np.ascontiguousarray(train, np.uint8)
    out = np.zeros(len(ii), np.int64)
    step = 1 << 20
    for a in range(0, len(ii), step):
        x = np.bitwise_xor(q[ii[a:a + step]], t[jj[a:a + step]])
        out[a:a + step] = np.bitwise_count(x).sum(axis=1)
    return out


def guided(query, train, loc_q, loc_t, oct_q=None, oct_t=None, prior=None, radius=16.0, max_octave_diff=-1, ratio=0.9):
    """S17: (queryIdx, trainIdx, distance) rows in ascending queryIdx.  query / train: n x 32|64 uint8 (the rows below the counts),
    loc_*: n x 2 integer locations, oct_*: n octaves (read only with the octave gate), prior: None or (H, hypothesis)."""
    query = np.asarray(query, np.uint8)
    train = np.asarray(train, np.uint8)
    nq, nt = len(query), len(train)
    if nq == 0 or nt == 0:
        return np.zeros((0, 3), np.int32)
    ii, jj = candidates(loc_q, loc_t, oct_q, oct_t, prior, radius, max_octave_diff)
    d = hamming_pairs(query, train, ii, jj)
    i12, d12 = _best2(ii, jj, d, nq)
    i21, d21 = _best2(jj, ii, d, nt)
    return MR.from_knn(i12, d12, i21, d21, ratio)


def within_gate(rows, loc_q, loc_t, oct_q, oct_t, prior, radius, max_octave_diff):
    """the rows (i, j, d) whose pair passes the gate (consequence (b) of S17)"""
    rows = np.asarray(rows, np.int32).reshape(-1, 3)
    loc_q = np.asarray(loc_q, np.int64).reshape(-1, 2)
    loc_t = np.asarray(loc_t, np.int64).reshape(-1, 2)
    pr = predict(loc_q, prior)
    if pr is None or len(rows) == 0:
        return rows[:0]
    px, py, valid = pr
    i, j = rows[:, 0], rows[:, 1]
    R = float(np.float32(radius))
    with np.errstate(all="ignore"):
        ok = valid[i] & (np.abs(loc_t[j, 0].astype(np.float64) - px[i]) <= R) & (np.abs(loc_t[j, 1].astype(np.float64) - py[i]) <= R)
    if max_octave_diff >= 0:
        ok &= np.abs(np.asarray(oct_q, np.int32)[i] - np.asarray(oct_t, np.int32)[j]) <= np.int32(max_octave_diff)
    return rows[ok]


def literal(query, train, loc_q, loc_t, oct_q, oct_t, prior, radius, max_octave_diff, ratio):
    """S17 step by step in plain Python floats (IEEE doubles, no fused operations), one pair at a time"""
    query = [bytes(np.asarray(r, np.uint8)) for r in query]
    train = [bytes(np.asarray(r, np.uint8)) for r in train]
    nq, nt = len(query), len(train)
    R = float(np.float32(radius))
    if nq == 0 or nt == 0:
        return np.zeros((0, 3), np.int32)
    if prior is not None and prior[1] < 0:
        return np.zeros((0, 3), np.int32)
    H = None if prior is None else [float(v) for v in np.asarray(prior[0], np.float64).reshape(9)]

    def div(a, b):
        try:
            return a / b
        except ZeroDivisionError:
            return math.nan if a == 0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)

    C = set()
    for i in range(nq):
        x, y = float(int(loc_q[i][0])), float(int(loc_q[i][1]))
        if H is None:
            px, py = x, y
        else:
            X = (H[0] * x + H[1] * y) + H[2]
            Y = (H[3] * x + H[4] * y) + H[5]
            W = (H[6] * x + H[7] * y) + H[8]
            px, py = div(X, W), div(Y, W)
            if not (W > 0) or not math.isfinite(px) or not math.isfinite(py):
                continue
        for j in range(nt):
            if not (abs(float(int(loc_t[j][0])) - px) <= R and abs(float(int(loc_t[j][1])) - py) <= R):
                continue
            if max_octave_diff >= 0 and not (abs(int(oct_q[i]) - int(oct_t[j])) <= max_octave_diff):
                continue
            C.add((i, j))

    def dist(a, b):
        return sum(bin(u ^ v).count("1") for u, v in zip(a, b))

    def best2(n, cands):
        out = []
        for a in range(n):
            best = sorted(cands(a))[:2]                 # (distance, index): ties to the lower index
            out.append(best)
        return out
    m12 = best2(nq, lambda i: [(dist(query[i], train[j]), j) for j in range(nt) if (i, j) in C])
    m21 = best2(nt, lambda j: [(dist(query[i], train[j]), i) for i in range(nq) if (i, j) in C])
    rows = []
    for i in range(nq):
        a = m12[i]
        if not a:
            continue
        b = m21[a[0][1]]
        if len(a) > 1 and float(a[0][0]) > ratio * float(a[1][0]):
            continue
        if len(b) > 1 and float(b[0][0]) > ratio * float(b[1][0]):
            continue
        if b[0][1] != i:
            continue
        rows.append((i, a[0][1], a[0][0]))
    return np.array(rows, np.int32).reshape(-1, 3)


def pack_keypoints(xy, octave=None, capacity=None, seed=0):
    """5 x capacity float32 keypoint matrix: LOCATION = xy as short2 bits, OCTAVE = octave (int32 bits), everything else -- the
    other rows and every column at or beyond len(xy) -- poison"""
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    cap = len(xy) if capacity is None else capacity
    k = np.random.default_rng(seed).integers(0, 1 << 32, (5, max(cap, 1)), dtype=np.uint32)[:, :cap].copy()
    k[0, :len(xy)] = xy[:, 0].astype(np.uint16).astype(np.uint32) | (xy[:, 1].astype(np.uint16).astype(np.uint32) << np.uint32(16))
    if octave is not None:
        k[3, :len(xy)] = np.asarray(octave, np.int32).view(np.uint32)
    return k.view(np.float32)
