"""numpy restatement of DESIGN.md spec S16 (RANSAC homography verification of matches, efx_match_homography_async), vectorised
over hypotheses.  Every step but the refit is written with the operations, types and order of the spec, so the GPU tests compare
with it bit for bit: int64 for the exact parts, float64 for the four-point model, float32 for the score.

ransac() takes the inputs of one pair as the device reads them (the LOCATION coordinates of both keypoint matrices, the match rows,
the device count and the capacities) and returns a dict with H (3 x 3 float64), ninliers, hypothesis, valid_hypotheses, refined and
mask (uint8[capacity]).  Helpers build the synthetic keypoint matrices the tests upload."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))


def splitmix64(x):
    """splitmix64 of a uint64 array (wrap-around arithmetic)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sample(n, seed, hyps, first=0):
    """S16 step 2: the four row indices of hypotheses first .. first + hyps - 1 (hyps x 4 int64), n >= 4"""
    h = np.arange(first, first + hyps, dtype=np.uint64)
    idx = np.zeros((hyps, 4), dtype=np.int64)
    with np.errstate(over="ignore"):
        for j in range(4):
            r = splitmix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + np.uint64(4) * h + np.uint64(j))
            v = ((r >> np.uint64(32)) * np.uint64(n - j) >> np.uint64(32)).astype(np.int64)
            earlier = np.sort(idx[:, :j], axis=1)
            for k in range(j):
                v = v + (v >= earlier[:, k])
            idx[:, j] = v
    return idx


def cross(a, b, c):
    """z of (b - a) x (c - a), int64 (... x 2 arrays)"""
    return (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])


def subset_ok(s, d):
    """S16 step 3: s, d: (..., 4, 2) int64 sample points -> bool (...)"""
    ok = np.ones(s.shape[:-2], dtype=bool)
    flips = np.zeros(s.shape[:-2], dtype=np.int64)
    for i, j, k in TRIPLES:
        cs, cd = cross(s[..., i, :], s[..., j, :], s[..., k, :]), cross(d[..., i, :], d[..., j, :], d[..., k, :])
        ok &= (cs != 0) & (cd != 0)
        flips += (cs > 0) != (cd > 0)
    return ok & ((flips == 0) | (flips == 4))


def quad(p):
    """S16 step 4: Q(p0..p3) of (..., 4, 2) int64 points -> a, b, c, d, e, f, g, h (float64 arrays)"""
    x0, x1, x2, x3 = (p[..., i, 0] for i in range(4))
    y0, y1, y2, y3 = (p[..., i, 1] for i in range(4))
    sx, sy = x0 - x1 + x2 - x3, y0 - y1 + y2 - y3
    dx1, dx2, dy1, dy2 = x1 - x2, x3 - x2, y1 - y2, y3 - y2
    den = dx1 * dy2 - dx2 * dy1
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (sx * dy2 - dx2 * sy).astype(np.float64) / den.astype(np.float64)
        h = (dx1 * sy - sx * dy1).astype(np.float64) / den.astype(np.float64)
    f64 = lambda v: v.astype(np.float64)
    a = f64(x1 - x0) + g * f64(x1)
    b = f64(x3 - x0) + h * f64(x3)
    d = f64(y1 - y0) + g * f64(y1)
    e = f64(y3 - y0) + h * f64(y3)
    return a, b, f64(x0), d, e, f64(y0), g, h


def four_point(s, d):
    """S16 step 4: H = Q_dst adj(Q_src) / H22 -> (..., 9) float64 and validity (H22 != 0, every entry finite)"""
    with np.errstate(all="ignore"):
        a, b, c, dd, e, f, g, h = quad(s)
        A = [e - f * h, c * h - b, b * f - c * e,
             f * g - dd, a - c * g, c * dd - a * f,
             dd * h - e * g, b * g - a * h, a * e - b * dd]
        Da, Db, Dc, Dd, De, Df, Dg, Dh = quad(d)
        rows = ((Da, Db, Dc), (Dd, De, Df), (Dg, Dh, np.ones_like(Dg)))
        H = np.stack([(rows[i][0] * A[j] + rows[i][1] * A[3 + j]) + rows[i][2] * A[6 + j] for i in range(3) for j in range(3)], axis=-1)
        h22 = H[..., 8].copy()
        H = H / h22[..., None]
        ok = (h22 != 0) & np.all(np.isfinite(H), axis=-1)
    return H, ok


def inliers(c, x, y, xd, yd, t):
    """S16 step 5: c (k x 9 float32), points float32 -> bool (k x n); the operations in exactly the spec's order"""
    f = np.float32
    t2 = f(t) * f(t)
    c = c.astype(f)
    x, y, xd, yd = (v.astype(f)[None, :] for v in (x, y, xd, yd))
    col = lambda i: c[:, i:i + 1]
    with np.errstate(all="ignore"):
        X = (col(0) * x + col(1) * y) + col(2)
        Y = (col(3) * x + col(4) * y) + col(5)
        W = (col(6) * x + col(7) * y) + col(8)
        ex = X - xd * W
        ey = Y - yd * W
        return (W != 0) & (ex * ex + ey * ey <= t2 * (W * W))


def gather(q_xy, t_xy, matches, nmatches, capacity):
    """S16 step 1: src / dst int64 (n x 2) and the row validity, n = the clamped count (None: capacity)"""
    n = capacity if nmatches is None else min(max(int(nmatches), 0), capacity)
    m = np.asarray(matches, dtype=np.int64).reshape(-1, 3)[:n]
    qi, ti = m[:, 0], m[:, 1]
    ok = (qi >= 0) & (qi < len(q_xy)) & (ti >= 0) & (ti < len(t_xy))
    src = np.zeros((n, 2), dtype=np.int64)
    dst = np.zeros((n, 2), dtype=np.int64)
    src[ok] = np.asarray(q_xy, dtype=np.int64)[qi[ok]]
    dst[ok] = np.asarray(t_xy, dtype=np.int64)[ti[ok]]
    return src, dst, ok


def hypotheses(src, dst, ok, seed, hyps):
    """S16 steps 2-4 for every hypothesis: (hyps x 9 float64 models, validity)"""
    n = len(src)
    if n < 4:
        return np.zeros((hyps, 9)), np.zeros(hyps, dtype=bool)
    idx = sample(n, seed, hyps)
    s, d = src[idx], dst[idx]
    valid = np.all(ok[idx], axis=1) & subset_ok(s, d)
    H, fin = four_point(s, d)
    valid &= fin
    return H, valid


def solve_pivot(A, b):
    """Gaussian elimination with partial pivoting (the first largest |pivot|), as the device solves the 8 x 8 system; None on a
    zero pivot"""
    M = np.concatenate([np.array(A, dtype=np.float64), np.array(b, dtype=np.float64).reshape(-1, 1)], axis=1)
    n = len(M)
    for col in range(n):
        piv = col + int(np.argmax(np.abs(M[col:, col])))
        if M[piv, col] == 0:
            return None
        M[[col, piv]] = M[[piv, col]]
        for r in range(col + 1, n):
            M[r, col:] -= M[r, col] / M[col, col] * M[col, col:]
    x = np.zeros(n)
    for r in range(n - 1, -1, -1):
        x[r] = (M[r, n] - M[r, r + 1:n] @ x[r + 1:]) / M[r, r]
    return x


def dlt_system(src, dst):
    """the 2k x 8 rows of the h22 = 1 DLT: [x y 1 0 0 0 -x x' -y x'] = x', [0 0 0 x y 1 -x y' -y y'] = y'"""
    x, y, u, v = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
    z, o = np.zeros_like(x), np.ones_like(x)
    A = np.concatenate([np.stack([x, y, o, z, z, z, -x * u, -y * u], 1), np.stack([z, z, z, x, y, o, -x * v, -y * v], 1)])
    return A, np.concatenate([u, v])


def hartley(p):
    """T = [[s 0 -s cx] [0 s -s cy] [0 0 1]]: centroid c, mean distance to it -> sqrt(2)"""
    k = len(p)
    c = p.sum(axis=0).astype(np.float64) / k
    q = p.astype(np.float64) - c
    s = np.sqrt(2.0) / (np.sqrt((q * q).sum(axis=1)).sum() / k)
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def refit(src, dst):
    """S16 step 7: least-squares homography of integer correspondences (k >= 4) or None"""
    with np.errstate(all="ignore"):
        Ts, Td = hartley(src), hartley(dst)
        hs = lambda p, T: (p.astype(np.float64) @ T[:2, :2].T) + T[:2, 2]
        A, b = dlt_system(hs(src, Ts), hs(dst, Td))
        h = solve_pivot(A.T @ A, A.T @ b)
        if h is None:
            return None
        Hn = np.append(h, 1.0).reshape(3, 3)
        H = np.linalg.inv(Td) @ Hn @ Ts
        if H[2, 2] == 0:
            return None
        H = H / H[2, 2]
    return H if np.all(np.isfinite(H)) else None


def ransac(q_xy, t_xy, matches, nmatches, capacity, seed=0, hyps=2048, threshold=3.0, refine=True, block=64):
    src, dst, ok = gather(q_xy, t_xy, matches, nmatches, capacity)
    n = len(src)
    out = dict(H=np.zeros((3, 3)), ninliers=0, hypothesis=-1, valid_hypotheses=0, refined=0, mask=np.zeros(capacity, dtype=np.uint8),
               four_point=np.zeros((3, 3)))
    H, valid = hypotheses(src, dst, ok, seed, hyps)
    if not valid.any():
        return out
    c32 = H.astype(np.float32)
    f = [v.astype(np.float32) for v in (src[:, 0], src[:, 1], dst[:, 0], dst[:, 1])]
    counts = np.full(hyps, -1, dtype=np.int64)
    for h0 in range(0, hyps, block):
        sel = np.nonzero(valid[h0:h0 + block])[0] + h0
        if len(sel):
            counts[sel] = (inliers(c32[sel], *f, threshold) & ok[None, :]).sum(axis=1)
    w = int(np.argmax(counts))                                   # the first maximum: ties go to the lowest index
    mask = inliers(c32[w:w + 1], *f, threshold)[0] & ok
    out.update(ninliers=int(counts[w]), hypothesis=w, valid_hypotheses=int(valid.sum()), four_point=H[w].reshape(3, 3))
    out["mask"][:n] = mask
    out["H"] = H[w].reshape(3, 3).copy()
    if refine and counts[w] >= 4:
        R = refit(src[mask], dst[mask])
        if R is not None:
            out.update(H=R, refined=1)
    return out


def project(H, pts):
    """pts (k x 2) through H"""
    p = np.concatenate([pts, np.ones((len(pts), 1))], axis=1) @ np.asarray(H, dtype=np.float64).T
    return p[:, :2] / p[:, 2:3]


def corners(w=1920, h=1080):
    return np.array([[0, 0], [w, 0], [w, h], [0, h]], dtype=np.float64)


def true_homography(rng, w=1920, h=1080, rot=0.2, scale=0.1, persp=2e-5, shift=40.0):
    """a random frame-to-frame homography about the frame centre: rotation, scale, mild perspective, shift"""
    th = rng.uniform(-rot, rot)
    s = 1.0 + rng.uniform(-scale, scale)
    c, si = np.cos(th), np.sin(th)
    A = np.array([[s * c, -s * si, rng.uniform(-shift, shift)], [s * si, s * c, rng.uniform(-shift, shift)],
                  [rng.uniform(-persp, persp), rng.uniform(-persp, persp), 1.0]])
    T = np.array([[1, 0, w / 2], [0, 1, h / 2], [0, 0, 1.0]])
    Ti = np.array([[1, 0, -w / 2], [0, 1, -h / 2], [0, 0, 1.0]])
    H = T @ A @ Ti
    return H / H[2, 2]


def synth_matches(rng, n, outliers, H, w=1920, h=1080, q_extra=0, t_extra=0):
    """n correspondences, a fraction `outliers` of them random: (query xy, train xy, matches n x 3).  Inlier train points are the
    rounded projections of distinct integer query points; the query / train keypoint lists are shuffled and padded by extra
    keypoints that no match uses."""
    q = np.stack([rng.integers(0, w, n + q_extra), rng.integers(0, h, n + q_extra)], axis=1).astype(np.int64)
    t = np.rint(project(H, q[:n].astype(np.float64))).astype(np.int64) if n else np.zeros((0, 2), np.int64)
    bad = rng.random(n) < outliers
    t[bad] = np.stack([rng.integers(0, w, bad.sum()), rng.integers(0, h, bad.sum())], axis=1)
    t = np.clip(t, -32768, 32767)
    t = np.concatenate([t, np.stack([rng.integers(0, w, t_extra), rng.integers(0, h, t_extra)], axis=1)]) if t_extra else t
    qp, tp = rng.permutation(len(q)), rng.permutation(len(t))
    qinv, tinv = np.argsort(qp), np.argsort(tp)
    m = np.zeros((n, 3), dtype=np.int32)
    m[:, 0] = qinv[:n]
    m[:, 1] = tinv[:n]
    m[:, 2] = rng.integers(0, 64, n)
    return q[qp], t[tp], m


def pack_location(xy, capacity=None):
    """5 x capacity float32 keypoint matrix whose LOCATION row holds xy as short2 bits (other rows: garbage)"""
    xy = np.asarray(xy, dtype=np.int64)
    cap = len(xy) if capacity is None else capacity
    k = np.random.default_rng(len(xy)).random((5, max(cap, 1)), dtype=np.float32)[:, :cap].copy()
    loc = (xy[:, 0].astype(np.uint16).astype(np.uint32)) | (xy[:, 1].astype(np.uint16).astype(np.uint32) << np.uint32(16))
    k[0, :len(xy)] = loc.view(np.float32)
    return k


def warp_frame(base, G, rows, cols):
    """frame = base sampled bilinearly at G^-1 (u, v)"""
    Gi = np.linalg.inv(G)
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    p = np.stack([u.ravel(), v.ravel(), np.ones(u.size)])
    s = Gi @ p
    sx, sy = s[0] / s[2], s[1] / s[2]
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    ok = (x0 >= 0) & (y0 >= 0) & (x0 + 1 < base.shape[1]) & (y0 + 1 < base.shape[0])
    x0c, y0c = np.clip(x0, 0, base.shape[1] - 2), np.clip(y0, 0, base.shape[0] - 2)
    fx, fy = sx - x0c, sy - y0c
    b = base.astype(np.float64)
    val = (1 - fy) * ((1 - fx) * b[y0c, x0c] + fx * b[y0c, x0c + 1]) + fy * ((1 - fx) * b[y0c + 1, x0c] + fx * b[y0c + 1, x0c + 1])
    val = np.where(ok, val, 128.0)
    return np.clip(np.rint(val), 0, 255).astype(np.uint8).reshape(rows, cols)


def frame_homographies(rng, nf, rows=1080, cols=1920, base_rows=1500, base_cols=2500):
    """nf scene -> frame homographies G (rotation up to 0.03 rad, scale within 4 %, shift up to 20 px, mild perspective), mapping
    the centre of a base_rows x base_cols scene to the frame centre; frame i + 1 relates to frame i by G[i + 1] G[i]^-1"""
    G = []
    for _ in range(nf):
        th, s = 0.03 * rng.uniform(-1, 1), 1.0 + 0.04 * rng.uniform(-1, 1)
        A = np.array([[s * np.cos(th), -s * np.sin(th), rng.uniform(-20, 20)], [s * np.sin(th), s * np.cos(th), rng.uniform(-20, 20)],
                      [rng.uniform(-1e-5, 1e-5), rng.uniform(-1e-5, 1e-5), 1.0]])
        G.append(np.array([[1, 0, cols / 2], [0, 1, rows / 2], [0, 0, 1.0]]) @ A
                 @ np.array([[1, 0, -base_cols / 2], [0, 1, -base_rows / 2], [0, 0, 1.0]]))
    return G
