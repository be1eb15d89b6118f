"""Calls queued on one stream behind each other, with the context's geometry changing in between.  include/efx.h promises one
context per (thread, stream, device), so stream order is all a caller relies on: a setter, a new frame size, a new batch size
or another entry point between two queued calls must not change what the earlier call computes.

Every transition A -> B runs the same protocol on one context and one stream:
  1. A runs once and the device is synchronised (A's geometry is built and every buffer is warm);
  2. a calibrated delay (torch.cuda._sleep) is armed on the stream and A is enqueued again behind it;
  3. the stream is asserted busy, the change is applied (setters), and -- unless the change is a describer switch, which waits for
     the context's streams by design -- the stream is asserted busy again: B's host-side rebuild runs while A is provably pending;
  4. B is enqueued, the device is synchronised, and A's and B's outputs are compared, frame by frame, with a single-frame call on
     a fresh context (bit for bit: keypoint rows, N, descriptor bytes -- HashSIFT included, HIP against HIP is deterministic);
     at 640x480 and 1280x720 one frame of B is also checked against the oracle.
Outputs are preallocated and poisoned before the delay is armed, so no allocation or EFX_POISON fill drains it.

A second class asserts that some changes cost no host wait at all: once a geometry has been used with a batch size, calls of any
batch size, and changes of the FAST threshold or the NMS radius (kernel arguments), enqueue behind a pending stream."""
import itertools
import os

import numpy as np
import pytest

from tools import synth

pytestmark = pytest.mark.gpu

BAD_256, BAD_512, HASH_SIFT_256, HASH_SIFT_512 = 0, 1, 2, 3
UHD, FHD, HD, VGA = (2160, 3840), (1080, 1920), (720, 1280), (480, 640)
ANCHORED = (HD, VGA)                 # sizes at which one frame of every B is also checked against the oracle
DELAY_MS = 50.0                      # per pair; A's enqueue and the setters take a few ms of host time at most
BASE = dict(nfeatures=3000, scale_factor=1.2, nlevels=8, first_level=0, fast_threshold=20, nonmax_radius=15, dtype=BAD_256)
FIELDS = ("nfeatures", "scale_factor", "nlevels", "first_level", "fast_threshold", "nonmax_radius", "dtype")


def cfg(**kw):
    c = dict(BASE)
    c.update(kw)
    return c


def call(kind, size, frames, c):
    """kind: batch | dc (detectAndComputeAsync) | detect | masked | provided (useProvidedKeypoints) | compute (computeAsync);
    frames: image keys (kind, seed), one per frame."""
    return (kind, size, tuple(frames), tuple(sorted(c.items())))


def frames(n, kind="synth", seed0=0):
    return [(kind, seed0 + i) for i in range(n)]


def _name(c):
    return f"{c[0]} {c[1][0]}x{c[1][1]} x{len(c[2])} {dict(c[3])}"


class Env:
    """Images, poisoned outputs, references (fresh contexts) and the delay, shared by the whole module."""

    def __init__(self, cef, torch, oracle):
        self.cef, self.torch, self.oracle = cef, torch, oracle
        self._img, self._ref, self._orc, self._kin = {}, {}, {}, {}
        self.delayed_ms = 0.0
        # calibrate torch.cuda._sleep once: cycles per millisecond on this device
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        best = None
        for _ in range(2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record()
                torch.cuda._sleep(2_000_000)
                e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        assert best > 0.05, f"torch.cuda._sleep(2e6) took {best} ms: cannot calibrate a delay"
        self.cycles_per_ms = 2_000_000 / best

    def delay(self, stream, ms=DELAY_MS):
        assert ms <= 200.0
        self.delayed_ms += ms
        with self.torch.cuda.stream(stream):
            self.torch.cuda._sleep(int(self.cycles_per_ms * ms))

    def image(self, size, key):
        k = (size, key)
        if k not in self._img:
            rows, cols = size
            kind, seed = key
            if kind == "synth":
                im = synth.synth_frame(rows, cols, seed=3000 + seed)
            elif kind == "dense":
                im = synth.powerlaw_frame(rows, cols, seed=4000 + seed, beta=1.0)
            elif kind == "const":
                im = np.full((rows, cols), 90 + 7 * seed, np.uint8)
            else:
                raise ValueError(kind)
            self._img[k] = (im, self.torch.from_numpy(np.ascontiguousarray(im)).cuda())
        return self._img[k]

    def mask(self, size):
        k = (size, "mask")
        if k not in self._img:
            rows, cols = size
            m = np.zeros((rows, cols), np.uint8)
            m[rows // 8: rows - rows // 5, cols // 6: cols - cols // 9] = 255
            self._img[k] = (m, self.torch.from_numpy(m).cuda())
        return self._img[k][1]

    def input_keypoints(self, size, key):
        """Keypoints a provided-keypoints / compute call describes: a detect of the frame at the base parameters."""
        k = (size, key)
        if k not in self._kin:
            det = self.cef.EfficientFeatures.create(BASE["nfeatures"], dtype=BAD_256)
            kps, cnt = det.detectAsync(self.image(size, key)[1])
            self.torch.cuda.synchronize()
            n = int(cnt.item())
            self._kin[k] = kps[:, :n].cpu().numpy().copy()
            del det
        return self._kin[k]

    def make(self, detector, stream, c):
        return Prepared(self, detector, stream, c)

    def reference(self, c, i):
        """Frame i of call c as a single-frame call of the same kind on a fresh context, synchronised."""
        kind, size, fr, items = c
        single = "dc" if kind == "batch" else kind
        k = (single, size, fr[i], items)
        if k not in self._ref:
            p = dict(items)
            det = self.cef.EfficientFeatures.create(p["nfeatures"], p["scale_factor"], p["nlevels"], p["first_level"],
                                                    p["fast_threshold"], p["nonmax_radius"], p["dtype"])
            s = self.torch.cuda.current_stream()
            pr = Prepared(self, det, s, (single, size, (fr[i],), items))
            pr.run()
            self.torch.cuda.synchronize()
            self._ref[k] = pr.results()[0]
            del pr, det
        return self._ref[k]

    def oracle_result(self, c, i):
        kind, size, fr, items = c
        p = dict(items)
        bad = p["dtype"] in (BAD_256, BAD_512) and kind in ("batch", "dc")
        k = (size, fr[i], items if bad else tuple(x for x in items if x[0] != "dtype"))
        if k not in self._orc:
            r = self.oracle.detect_and_compute(self.image(size, fr[i])[0], nfeatures=p["nfeatures"], scale_factor=p["scale_factor"],
                                               nlevels=p["nlevels"], first_level=p["first_level"],
                                               fast_threshold=p["fast_threshold"], nonmax_radius=p["nonmax_radius"],
                                               desc_type=p["dtype"] if bad else -1)
            self._orc[k] = (r["n"], r["kps"].view(np.uint32), r["desc"] if bad else None)
        return self._orc[k]

    def check(self, pr, c, what):
        got = pr.results()
        for i in range(len(c[2])):
            _same(got[i], self.reference(c, i), f"{what}: frame {i} against a fresh single-frame call")
        if c[1] in ANCHORED and c[0] in ("batch", "dc", "detect"):
            o = self.oracle_result(c, 0)
            g = got[0]
            _same((g[0], g[1], g[2] if o[2] is not None else None), o, f"{what}: frame 0 against the oracle")


class Prepared:
    """One call with its outputs allocated (poisoned) up front; run() only enqueues."""

    def __init__(self, env, detector, stream, c):
        torch = env.torch
        self.env, self.det, self.stream, self.c = env, detector, stream, c
        kind, size, fr, items = c
        p = dict(items)
        cap = p["nfeatures"]
        nbytes = 64 if p["dtype"] in (BAD_512, HASH_SIFT_512) else 32
        self.imgs = [env.image(size, f)[1] for f in fr]
        self.mask = env.mask(size) if kind == "masked" else None
        self.kin = None
        if kind in ("provided", "compute"):
            assert len(fr) == 1
            k = env.input_keypoints(size, fr[0])
            self.n_in = k.shape[1]
            self.kin = torch.from_numpy(k).cuda()
            self.kps, self.cnt = None, None
            self.desc = [torch.full((max(self.n_in, 1), nbytes), 0xA5, dtype=torch.uint8, device="cuda")]
        else:
            self.kps = [torch.full((5, cap), -7.0, dtype=torch.float32, device="cuda") for _ in fr]
            self.cnt = [torch.full((1,), -1, dtype=torch.int32, device="cuda") for _ in fr]
            self.desc = None if kind == "detect" else [torch.full((cap, nbytes), 0xA5, dtype=torch.uint8, device="cuda") for _ in fr]
        self.batch = env.cef.Batch([detector], [stream], self.imgs, self.kps, self.desc, self.cnt, cap) if kind == "batch" else None
        self.cap = cap

    def run(self):
        kind = self.c[0]
        d, s = self.det, self.stream
        if kind == "batch":
            self.batch.run()
        elif kind == "dc":
            d.detectAndComputeAsync(self.imgs[0], keypoints=self.kps[0], descriptors=self.desc[0], count=self.cnt[0], stream=s)
        elif kind == "detect":
            d.detectAsync(self.imgs[0], keypoints=self.kps[0], count=self.cnt[0], stream=s)
        elif kind == "masked":
            d.detectAndComputeAsync(self.imgs[0], keypoints=self.kps[0], descriptors=self.desc[0], count=self.cnt[0], stream=s,
                                    mask=self.mask)
        elif kind == "provided":
            d.detectAndComputeAsync(self.imgs[0], keypoints=self.kin, descriptors=self.desc[0], useProvidedKeypoints=True,
                                    n=self.n_in, stream=s)
        elif kind == "compute":
            d.computeAsync(self.imgs[0], self.kin, n=self.n_in, descriptors=self.desc[0], stream=s)
        else:
            raise ValueError(kind)

    def results(self):
        """Per frame (N, keypoint rows as uint32, descriptor bytes or None); read after a synchronisation."""
        if self.kin is not None:
            return [(self.n_in, None, self.desc[0][:self.n_in].cpu().numpy())]
        out = []
        for i in range(len(self.imgs)):
            n = int(self.cnt[i].item())
            assert 0 <= n <= self.cap, f"count {n} outside 0 .. {self.cap}: the call did not write it"
            out.append((n, self.kps[i][:, :n].cpu().numpy().view(np.uint32), None if self.desc is None else self.desc[i][:n].cpu().numpy()))
        return out


def _same(a, b, what):
    assert a[0] == b[0], f"{what}: N {a[0]} != {b[0]}"
    if a[1] is not None:
        assert np.array_equal(a[1], b[1]), f"{what}: keypoint rows differ"
    if a[2] is not None or b[2] is not None:
        assert a[2] is not None and b[2] is not None and np.array_equal(a[2], b[2]), f"{what}: descriptor bytes differ"


class Context:
    """The one context and stream a test drives, with the parameters it currently holds."""

    def __init__(self, env, c=None):
        c = dict(BASE if c is None else c)
        self.env = env
        self.det = env.cef.EfficientFeatures.create(c["nfeatures"], c["scale_factor"], c["nlevels"], c["first_level"],
                                                    c["fast_threshold"], c["nonmax_radius"], c["dtype"])
        self.stream = env.torch.cuda.Stream()
        self.p = c

    def apply(self, p):
        """Setters for every field that differs; True if the describer was switched."""
        d = self.det
        setters = dict(nfeatures=d.setMaxFeatures, scale_factor=d.setScaleFactor, nlevels=d.setNLevels, first_level=d.setFirstLevel,
                       fast_threshold=d.setFastThreshold, nonmax_radius=d.setNonmaxRadius, dtype=d.setDescriptorType)
        for f in FIELDS:
            if p[f] != self.p[f]:
                setters[f](p[f])
        switched = p["dtype"] != self.p["dtype"]
        self.p = dict(p)
        return switched

    def pair(self, A, B, label):
        env, torch = self.env, self.env.torch
        what = f"{label}: {_name(A)} -> {_name(B)}"
        self.apply(dict(A[3]))
        env.make(self.det, self.stream, A).run()
        torch.cuda.synchronize()
        pa = env.make(self.det, self.stream, A)
        pb = env.make(self.det, self.stream, B)
        torch.cuda.synchronize()
        env.delay(self.stream)
        pa.run()
        assert not self.stream.query(), f"{what}: the stream drained while A was enqueued (delay too short for the host)"
        switched = self.apply(dict(B[3]))
        if not switched:
            assert not self.stream.query(), f"{what}: a setter waited for the stream"
        pb.run()
        torch.cuda.synchronize()
        env.check(pa, A, what + " [A]")
        env.check(pb, B, what + " [B]")

    def chain(self, calls, label):
        for A, B in zip(calls, calls[1:]):
            self.pair(A, B, label)


@pytest.fixture(scope="module")
def env(oracle):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cef_loader
    e = Env(cef_loader.load(), torch, oracle)
    yield e
    print(f"\nqueued-call delays: {e.delayed_ms / 1000:.2f} s in all")


# ---- batch size ----

@pytest.mark.parametrize("sizes", [(20, 3), (3, 20), (16, 1), (1, 16), (5, 16)], ids=lambda s: f"{s[0]}to{s[1]}")
def test_batch_size_change_fhd(env, sizes):
    """FHD batches of 3 or more frames take the row-walking pyramid chain, whose chunk tables depend on the frames per launch
    (20 frames: a launch of 16 and one of 4)."""
    ctx = Context(env)
    a, b = sizes
    ctx.pair(call("batch", FHD, frames(a), BASE), call("batch", FHD, frames(b, seed0=20), BASE), f"FHD batch {a} -> {b}")


def test_batch_of_20_alone_fhd(env):
    """One call of 20 frames queued behind itself: the 16 + 4 split inside one call, twice in a row."""
    ctx = Context(env)
    c = call("batch", FHD, frames(20, seed0=40), cfg(dtype=HASH_SIFT_256))
    ctx.pair(c, c, "FHD batch 20 -> 20")


def test_batch_size_change_4k(env):
    """4K: every frame takes the row-walking chain.  3 -> 1 -> 2 frames."""
    ctx = Context(env, cfg(nfeatures=8000))
    c = cfg(nfeatures=8000)
    ctx.chain([call("batch", UHD, frames(3), c), call("batch", UHD, frames(1, seed0=3), c), call("batch", UHD, frames(2, seed0=4), c)],
              "4K batch 3 -> 1 -> 2")


# ---- frame size ----

def test_frame_size_shrinks_and_grows(env):
    """4K -> FHD -> 1280x720 -> 640x480 -> FHD on one context: the level table and the resize plans are rewritten in place while
    the previous size's call is still queued."""
    ctx = Context(env)
    ctx.chain([call("dc", UHD, frames(1), BASE), call("batch", FHD, frames(3), BASE), call("dc", HD, frames(1), BASE),
               call("batch", VGA, frames(2), BASE), call("batch", FHD, frames(3, seed0=5), BASE)], "frame size")


# ---- setters ----

SETTER_STEPS = [
    ("setNLevels 8 -> 4", dict(nlevels=8), dict(nlevels=4)),
    ("setNLevels 4 -> 8", dict(nlevels=4), dict(nlevels=8)),
    ("setScaleFactor 1.2 -> 1.35", dict(scale_factor=1.2), dict(scale_factor=1.35)),
    ("setScaleFactor 1.35 -> 1.2", dict(scale_factor=1.35), dict(scale_factor=1.2)),
    ("setFirstLevel 0 -> 1", dict(first_level=0), dict(first_level=1)),
    ("setFirstLevel 1 -> 0", dict(first_level=1), dict(first_level=0)),
    ("setNonmaxRadius 15 -> 4", dict(nonmax_radius=15), dict(nonmax_radius=4)),
    ("setMaxFeatures 3000 -> 1200", dict(nfeatures=3000), dict(nfeatures=1200)),
    ("setMaxFeatures 1200 -> 3000", dict(nfeatures=1200), dict(nfeatures=3000)),
    ("setFastThreshold 20 -> 35", dict(fast_threshold=20), dict(fast_threshold=35)),
]


@pytest.mark.parametrize("where", ["fhd_batch3", "vga_dc"])
def test_setters(env, where):
    ctx = Context(env)
    for label, a, b in SETTER_STEPS:
        if where == "fhd_batch3":
            A, B = call("batch", FHD, frames(3), cfg(**a)), call("batch", FHD, frames(3, seed0=3), cfg(**b))
        else:
            A, B = call("dc", VGA, frames(1), cfg(**a)), call("dc", VGA, frames(1, seed0=1), cfg(**b))
        ctx.pair(A, B, f"{where} {label}")


# ---- describer ----

def test_descriptor_type_every_ordered_pair(env):
    """Every ordered pair of the four describers, detectAndComputeAsync on both sides: setDescriptorType rewrites the BAD boxes /
    HashSIFT weights of a block that may still be read by the queued call (BAD512 -> BAD256, HashSIFT -> BAD, HashSIFT512 ->
    256 fit the block)."""
    ctx = Context(env)
    for a, b in itertools.permutations([BAD_256, BAD_512, HASH_SIFT_256, HASH_SIFT_512], 2):
        ctx.pair(call("dc", HD, frames(1), cfg(dtype=a)), call("dc", HD, frames(1, seed0=1), cfg(dtype=b)), f"describer {a} -> {b}")


# ---- entry points ----

@pytest.mark.parametrize("size", [FHD, VGA], ids=["fhd", "vga"])
def test_entry_points(env, size):
    """batched -> detectAndComputeAsync -> masked -> provided keypoints -> computeAsync -> detectAsync; all but the first build
    the geometry for one frame per launch."""
    ctx = Context(env)
    ctx.chain([call("batch", size, frames(3), BASE), call("dc", size, frames(1, seed0=3), BASE), call("masked", size, frames(1), BASE),
               call("provided", size, frames(1, seed0=1), BASE), call("compute", size, frames(1, seed0=2), BASE),
               call("detect", size, frames(1, seed0=4), BASE), call("batch", size, frames(3, seed0=5), BASE)], "entry points")


# ---- frame content ----

def test_dense_sparse_constant_alternation(env):
    """The sparse / dense form of harris_kernel is chosen from a host-mapped word the previous frame left: with frames queued it is
    a frame stale, which must not change any result."""
    ctx = Context(env)
    ctx.chain([call("batch", FHD, frames(3, "dense"), BASE), call("batch", FHD, frames(3, "synth"), BASE),
               call("batch", FHD, frames(3, "const"), BASE), call("batch", FHD, frames(3, "dense", 3), BASE),
               call("dc", UHD, frames(1, "dense"), BASE), call("dc", UHD, frames(1, "const"), BASE),
               call("dc", UHD, frames(1, "synth"), BASE)], "content")


# ---- changes that cost no host wait ----

def _enqueue_busy(ctx, preps, changes, what):
    """Arms one delay, then enqueues every prepared call (after its setters), asserting the stream busy after each step."""
    env = ctx.env
    env.torch.cuda.synchronize()
    env.delay(ctx.stream, 150.0)
    for i, (pr, ch) in enumerate(zip(preps, changes)):
        if ch:
            ctx.apply(ch)
            assert not ctx.stream.query(), f"{what}: step {i}: a setter waited for the stream"
        pr.run()
        assert not ctx.stream.query(), f"{what}: step {i} ({_name(pr.c)}) waited for the stream"
    env.torch.cuda.synchronize()
    for i, pr in enumerate(preps):
        env.check(pr, pr.c, f"{what}: step {i}")


def test_batch_size_changes_do_not_wait(env):
    """Once a geometry has been used with a batch size, calls of other batch sizes on it enqueue without a host wait: 20 (16 + 4)
    twice, 3, 16, 1 at FHD behind one delay."""
    ctx = Context(env)
    for n in (20, 3, 1):
        env.make(ctx.det, ctx.stream, call("batch", FHD, frames(n), BASE)).run()
    env.torch.cuda.synchronize()
    seq = [call("batch", FHD, frames(20), BASE), call("batch", FHD, frames(20, seed0=1), BASE), call("batch", FHD, frames(3, seed0=2), BASE),
           call("batch", FHD, frames(16, seed0=3), BASE), call("batch", FHD, frames(1, seed0=4), BASE)]
    preps = [env.make(ctx.det, ctx.stream, c) for c in seq]
    _enqueue_busy(ctx, preps, [None] * len(seq), "batch sizes without a wait")


def test_kernel_argument_setters_do_not_wait(env):
    """setFastThreshold and setNonmaxRadius change kernel arguments, not the device tables: no host wait, at any batch size."""
    ctx = Context(env)
    for n in (16, 1):
        env.make(ctx.det, ctx.stream, call("batch", FHD, frames(n), BASE)).run()
    env.torch.cuda.synchronize()
    steps = [cfg(), cfg(fast_threshold=30), cfg(fast_threshold=30, nonmax_radius=5), cfg(fast_threshold=12, nonmax_radius=5), cfg()]
    # 1, 5, 1, 5, 1 frames; each step's setters bring the context to that step's parameters
    seq = [call("batch", FHD, frames(1 + 4 * (i % 2), seed0=i), c) for i, c in enumerate(steps)]
    preps = [env.make(ctx.det, ctx.stream, c) for c in seq]
    _enqueue_busy(ctx, preps, [dict(c[3]) if i else None for i, c in enumerate(seq)], "threshold / radius without a wait")


# ---- seeded fuzz ----

FUZZ_SIZES = [VGA, HD, FHD, (544, 968), (1088, 1936)]
FUZZ_KINDS = ["batch", "batch", "batch", "dc", "detect", "masked", "provided", "compute"]


def _fuzz_call(rng, p):
    kind = FUZZ_KINDS[int(rng.integers(0, len(FUZZ_KINDS)))]
    size = FUZZ_SIZES[int(rng.integers(0, len(FUZZ_SIZES)))]
    n = int(rng.integers(1, 21)) if kind == "batch" else 1
    content = ["synth", "synth", "dense", "const"][int(rng.integers(0, 4))]
    return call(kind, size, frames(n, content, int(rng.integers(0, 4))), p)


def _fuzz_params(rng, p):
    p = dict(p)
    for _ in range(int(rng.integers(0, 3))):
        f = FIELDS[int(rng.integers(0, len(FIELDS)))]
        p[f] = {"nfeatures": lambda: int(rng.choice([500, 1500, 3000])),
                "scale_factor": lambda: float(rng.choice([1.2, 1.35, 1.5])),
                "nlevels": lambda: int(rng.integers(2, 9)),
                "first_level": lambda: int(rng.integers(0, 2)),
                "fast_threshold": lambda: int(rng.choice([10, 20, 35])),
                "nonmax_radius": lambda: int(rng.choice([0, 4, 15])),
                "dtype": lambda: int(rng.integers(0, 4))}[f]()
    if p["first_level"] >= p["nlevels"]:
        p["first_level"] = 0
    return p


@pytest.mark.parametrize("seed", range(int(os.environ.get("EFX_QUEUE_FUZZ", "12"))))
def test_queued_fuzz(env, seed):
    """Random sequences of transitions on one context: sizes, batch sizes 1..20, entry points, setters and describers."""
    rng = np.random.default_rng(7100 + seed)
    p = dict(BASE)
    calls = []
    for _ in range(4):
        calls.append(_fuzz_call(rng, p))
        p = _fuzz_params(rng, p)
    ctx = Context(env, dict(calls[0][3]))
    ctx.chain(calls, f"fuzz seed {seed}")
