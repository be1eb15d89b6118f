"""numpy restatement of DESIGN.md spec S18 (RANSAC fundamental-matrix verification of matches, efx_match_fundamental_async),
vectorised over hypotheses.  Every step but the refit is written with the operations, types and order of the spec, so the GPU tests
compare with it bit for bit: int64 for the exact parts, float64 for the eight-point model, float32 for the score.  The refit
restates the device's algorithm (Hartley normalisation, A^T A, cyclic Jacobi with the device's round order, rank-2 projection) and
is compared by tolerance: the device adds its sums in another order.

ransac() takes the inputs of one pair as the device reads them and returns a dict with F (3 x 3 float64), ninliers, hypothesis,
valid_hypotheses, refined, mask (uint8[capacity]) and eight_point (the winner's minimal model)."""
import numpy as np

from tests import homography_reference as HR

splitmix64 = HR.splitmix64
gather = HR.gather
pack_location = HR.pack_location
SWEEPS9, SWEEPS3 = 8, 6       # Jacobi sweeps of the 9 x 9 and of the 3 x 3 solve


def sample(n, seed, hyps, first=0):
    """S18 step 2: the eight row indices of hypotheses first .. first + hyps - 1 (hyps x 8 int64), n >= 8"""
    h = np.arange(first, first + hyps, dtype=np.uint64)
    idx = np.zeros((hyps, 8), dtype=np.int64)
    with np.errstate(over="ignore"):
        for j in range(8):
            r = splitmix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + np.uint64(8) * h + np.uint64(j))
            v = ((r >> np.uint64(32)) * np.uint64(n - j) >> np.uint64(32)).astype(np.int64)
            earlier = np.sort(idx[:, :j], axis=1)
            for k in range(j):
                v = v + (v >= earlier[:, k])
            idx[:, j] = v
    return idx


def sample_ok(s, d):
    """S18 step 3: s, d (..., 8, 2) int64 -> bool (...): no two rows share a query location or a train location"""
    ok = np.ones(s.shape[:-2], dtype=bool)
    for i in range(8):
        for j in range(i + 1, 8):
            ok &= ~np.all(s[..., i, :] == s[..., j, :], axis=-1) & ~np.all(d[..., i, :] == d[..., j, :], axis=-1)
    return ok


def first_largest(F):
    """the entry of largest magnitude of each row (the first of equals), signed"""
    k = np.argmax(np.abs(F), axis=-1)
    return np.take_along_axis(F, k[..., None], axis=-1)[..., 0]


def eight_point(s, d):
    """S18 step 4: s, d (hyps x 8 x 2) int64 -> (hyps x 9 float64 models, validity)"""
    Hn = len(s)
    ar = np.arange(Hn)
    D = np.concatenate([s, d], axis=2)
    o = D[:, 0, :]
    R = D[:, 1:, :] - o[:, None, :]
    x, y, u, v = (R[:, :, k] for k in range(4))
    A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y], axis=2).astype(np.float64)          # exact integers below 2^34
    perm = np.tile(np.arange(8), (Hn, 1))
    ok = np.ones(Hn, dtype=bool)
    with np.errstate(all="ignore"):
        for c in range(7):
            sub = np.abs(A[:, c:, c:]).reshape(Hn, -1)
            k = np.argmax(sub, axis=1)                                                     # the first largest, row-major
            pr, pc = c + k // (8 - c), c + k % (8 - c)
            ok &= sub[ar, k] > 0
            t = A[ar, c, :].copy(); A[ar, c, :] = A[ar, pr, :]; A[ar, pr, :] = t
            t = A[ar, :, c].copy(); A[ar, :, c] = A[ar, :, pc]; A[ar, :, pc] = t
            t = perm[ar, c].copy(); perm[ar, c] = perm[ar, pc]; perm[ar, pc] = t
            f = A[:, c + 1:, c] / A[:, c, c][:, None]
            A[:, c + 1:, c:] = A[:, c + 1:, c:] - f[:, :, None] * A[:, c, c:][:, None, :]
        z = np.zeros((Hn, 8))
        z[:, 7] = 1.0
        for r in range(6, -1, -1):
            acc = np.zeros(Hn)
            for j in range(r + 1, 8):
                acc = acc + A[:, r, j] * z[:, j]
            z[:, r] = (0.0 - acc) / A[:, r, r]
        fv = np.zeros((Hn, 8))
        fv[ar[:, None], perm] = z
        f0, f1, f2, f3, f4, f5, f6, f7 = (fv[:, k] for k in range(8))
        ox, oy, ou, ov = (o[:, k].astype(np.float64) for k in range(4))
        g2 = f2 - (f0 * ox + f1 * oy)
        g5 = f5 - (f3 * ox + f4 * oy)
        g8 = 0.0 - (f6 * ox + f7 * oy)
        r6 = f6 - (ou * f0 + ov * f3)
        r7 = f7 - (ou * f1 + ov * f4)
        r8 = g8 - (ou * g2 + ov * g5)
        F = np.stack([f0, f1, g2, f3, f4, g5, r6, r7, r8], axis=1)
        dv = first_largest(F)
        F = F / dv[:, None]
        ok &= (dv != 0) & np.all(np.isfinite(F), axis=1)
    return F, ok


def inliers(c, x, y, u, v, t):
    """S18 step 5: c (k x 9 float32), points float32 -> bool (k x n); the operations in exactly the spec's order"""
    f = np.float32
    t2 = f(t) * f(t)
    c = c.astype(f)
    x, y, u, v = (w.astype(f)[None, :] for w in (x, y, u, v))
    col = lambda i: c[:, i:i + 1]
    with np.errstate(all="ignore"):
        a = (col(0) * x + col(1) * y) + col(2)
        b = (col(3) * x + col(4) * y) + col(5)
        cc = (col(6) * x + col(7) * y) + col(8)
        a2 = (col(0) * u + col(3) * v) + col(6)
        b2 = (col(1) * u + col(4) * v) + col(7)
        r = (a * u + b * v) + cc
        g = (a * a + b * b) + (a2 * a2 + b2 * b2)
        return (g > 0) & (r * r <= t2 * g)


def hypotheses(src, dst, ok, seed, hyps):
    """S18 steps 2-4 for every hypothesis: (hyps x 9 float64 models, validity)"""
    n = len(src)
    if n < 8:
        return np.zeros((hyps, 9)), np.zeros(hyps, dtype=bool)
    idx = sample(n, seed, hyps)
    s, d = src[idx], dst[idx]
    valid = np.all(ok[idx], axis=1) & sample_ok(s, d)
    F, fin = eight_point(s, d)
    return F, valid & fin


def jacobi(M, sweeps=SWEEPS9):
    """Cyclic Jacobi as the device runs it: `sweeps` sweeps of n rounds; round r rotates the disjoint pairs {i, (r - i) mod n} at
    once, M <- J^T M J, V <- V J.  Returns (diagonal, V)."""
    M = np.array(M, dtype=np.float64)
    n = len(M)
    V = np.eye(n)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for r in range(n):
                c, g = np.ones(n), np.zeros(n)
                part = (r - np.arange(n)) % n
                for p in range(n):
                    q = int(part[p])
                    if p < q and M[p, q] != 0:
                        a, b = M[q, q] - M[p, p], 2.0 * M[p, q]
                        h = np.sqrt(a * a + b * b)
                        t = b / (a + (h if a >= 0 else 0.0 - h))
                        cc = 1.0 / np.sqrt(t * t + 1.0)
                        s = t * cc
                        c[p], g[p], c[q], g[q] = cc, 0.0 - s, cc, s
                M = c[None, :] * M + g[None, :] * M[:, part]
                V = c[None, :] * V + g[None, :] * V[:, part]
                M = c[:, None] * M + g[:, None] * M[part, :]
    return np.diag(M).copy(), V


def hartley_cs(p):
    """centroid (integer sums / k) and scale sqrt(2) / mean distance, S16 step 7"""
    k = len(p)
    c = p.sum(axis=0).astype(np.float64) / k
    q = p.astype(np.float64) - c
    return c, np.sqrt(2.0) / (np.sqrt((q * q).sum(axis=1)).sum() / k)


def normalise(F):
    """divide by the first entry of largest magnitude; None when that is 0 or an entry is not finite"""
    with np.errstate(all="ignore"):
        F = np.asarray(F, dtype=np.float64).reshape(9)
        d = first_largest(F[None])[0]
        F = F / d
    return F.reshape(3, 3) if d != 0 and np.all(np.isfinite(F)) else None


def refit(src, dst):
    """S18 step 7: the normalised eight-point fit of rank 2 on integer correspondences (k >= 8) or None"""
    with np.errstate(all="ignore"):
        (cs, ss), (cd, sd) = hartley_cs(src), hartley_cs(dst)
        q = ss * (src.astype(np.float64) - cs)
        t = sd * (dst.astype(np.float64) - cd)
        u, v, U, V = q[:, 0], q[:, 1], t[:, 0], t[:, 1]
        A = np.stack([U * u, U * v, U, V * u, V * v, V, u, v, np.ones(len(u))], axis=1)
        w, E = jacobi(A.T @ A)
        Fn = E[:, int(np.argmin(w))].reshape(3, 3)
        w3, E3 = jacobi(Fn.T @ Fn, SWEEPS3)
        v3 = E3[:, int(np.argmin(w3))]
        Fn = Fn - np.outer(Fn @ v3, v3)
        Ts = np.array([[ss, 0, -ss * cs[0]], [0, ss, -ss * cs[1]], [0, 0, 1.0]])
        Td = np.array([[sd, 0, -sd * cd[0]], [0, sd, -sd * cd[1]], [0, 0, 1.0]])
        return normalise(Td.T @ Fn @ Ts)


def ransac(q_xy, t_xy, matches, nmatches, capacity, seed=0, hyps=2048, threshold=3.0, refine=True, block=64):
    src, dst, ok = gather(q_xy, t_xy, matches, nmatches, capacity)
    n = len(src)
    out = dict(F=np.zeros((3, 3)), ninliers=0, hypothesis=-1, valid_hypotheses=0, refined=0, mask=np.zeros(capacity, dtype=np.uint8),
               eight_point=np.zeros((3, 3)))
    F, valid = hypotheses(src, dst, ok, seed, hyps)
    if not valid.any():
        return out
    c32 = F.astype(np.float32)
    f = [w.astype(np.float32) for w in (src[:, 0], src[:, 1], dst[:, 0], dst[:, 1])]
    counts = np.full(hyps, -1, dtype=np.int64)
    for h0 in range(0, hyps, block):
        sel = np.nonzero(valid[h0:h0 + block])[0] + h0
        if len(sel):
            counts[sel] = (inliers(c32[sel], *f, threshold) & ok[None, :]).sum(axis=1)
    w = int(np.argmax(counts))                                   # the first maximum: ties go to the lowest index
    mask = inliers(c32[w:w + 1], *f, threshold)[0] & ok
    out.update(ninliers=int(counts[w]), hypothesis=w, valid_hypotheses=int(valid.sum()), eight_point=F[w].reshape(3, 3).copy())
    out["mask"][:n] = mask
    out["F"] = F[w].reshape(3, 3).copy()
    if refine and counts[w] >= 8:
        R = refit(src[mask], dst[mask])
        if R is not None:
            out.update(F=R, refined=1)
    return out


def sampson(F, q, t):
    """signed Sampson distance of the correspondences q -> t (k x 2) under F, in double"""
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    a = np.concatenate([np.asarray(q, np.float64), np.ones((len(q), 1))], axis=1)
    b = np.concatenate([np.asarray(t, np.float64), np.ones((len(t), 1))], axis=1)
    Fa, Fb = a @ F.T, b @ F
    with np.errstate(all="ignore"):
        return (b * Fa).sum(axis=1) / np.sqrt(Fa[:, 0] ** 2 + Fa[:, 1] ** 2 + Fb[:, 0] ** 2 + Fb[:, 1] ** 2)


def textbook_fit(src, dst):
    """the normalised eight-point algorithm with library solvers (eigh, svd): the second opinion on refit()"""
    def T(p):
        c = p.mean(axis=0)
        s = np.sqrt(2) / np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    T1, T2 = T(src), T(dst)
    a = np.concatenate([src, np.ones((len(src), 1))], axis=1) @ T1.T
    b = np.concatenate([dst, np.ones((len(dst), 1))], axis=1) @ T2.T
    A = np.stack([b[:, 0] * a[:, 0], b[:, 0] * a[:, 1], b[:, 0], b[:, 1] * a[:, 0], b[:, 1] * a[:, 1], b[:, 1], a[:, 0], a[:, 1],
                  np.ones(len(a))], axis=1)
    _, E = np.linalg.eigh(A.T @ A)
    U, s, Vt = np.linalg.svd(E[:, 0].reshape(3, 3))
    s[2] = 0
    return T2.T @ (U @ np.diag(s) @ Vt) @ T1


def scene(rng, n, outliers, w=1920, h=1080):
    """A camera moving through a 3-D scene: focal length 0.9 w, depths uniform in [4, 20], rotation up to 0.05 rad per axis,
    baseline 0.5, locations rounded to integers; a share `outliers` of the train locations is replaced by uniformly random ones.
    Returns (query xy, train xy (n x 2 int64, row i matches row i), good (n bool), the true F)."""
    f = 0.9 * w
    K = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]])
    Ki = np.linalg.inv(K)
    a = rng.uniform(-0.05, 0.05, 3)
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
         @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    t = rng.uniform(-1, 1, 3)
    t = t / np.linalg.norm(t) * 0.5
    q, tt = np.zeros((n, 2)), np.zeros((n, 2))
    k = 0
    while k < n:
        x, y, z = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(4, 20)
        X2 = R @ (Ki @ np.array([x, y, 1.0]) * z) + t
        p = K @ X2
        p = p[:2] / p[2]
        if 0 <= p[0] < w and 0 <= p[1] < h and X2[2] > 0:
            q[k], tt[k] = (x, y), p
            k += 1
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ft = Ki.T @ tx @ R @ Ki
    good = np.ones(n, dtype=bool)
    no = int(round(outliers * n))
    bad = rng.permutation(n)[:no]
    tt[bad] = np.stack([rng.uniform(0, w, no), rng.uniform(0, h, no)], axis=1)
    good[bad] = False
    return np.floor(q + 0.5).astype(np.int64), np.floor(tt + 0.5).astype(np.int64), good, Ft


def shuffled_matches(rng, q, t, q_extra=0, t_extra=0, w=1920, h=1080):
    """row-aligned correspondences -> shuffled keypoint lists padded by unused keypoints, and the n x 3 match rows"""
    n = len(q)
    q = np.concatenate([q, np.stack([rng.integers(0, w, q_extra), rng.integers(0, h, q_extra)], axis=1)]) if q_extra else q
    t = np.concatenate([t, np.stack([rng.integers(0, w, t_extra), rng.integers(0, h, t_extra)], axis=1)]) if t_extra else t
    qp, tp = rng.permutation(len(q)), rng.permutation(len(t))
    qinv, tinv = np.argsort(qp), np.argsort(tp)
    m = np.zeros((n, 3), dtype=np.int32)
    m[:, 0] = qinv[:n]
    m[:, 1] = tinv[:n]
    m[:, 2] = rng.integers(0, 64, n)
    return q[qp], t[tp], m


def identity_matches(n):
    k = np.arange(n)
    return np.stack([k, k, np.zeros_like(k)], axis=1).astype(np.int32)
