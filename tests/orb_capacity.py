"""ORB capacity predicate and hard-input generators (test helper: no pytest import, no GPU).

The ORB path keeps fixed-capacity device lists (mono_slam_framework_amd/csrc/orb_plan.h sizes them).  A frame whose result does not fit them comes back loud
(n_out = -1 / MSF_ERR_CAPACITY); any other frame must come back bit-exact, whatever else is in the call.  `capacity()`
decides from the CPU oracle (oracle/orb.py) which case a frame is, and the generators below build inputs that sit on either
side of that line.  tests/test_orb_capacity.py pins what every generator is for, tests/test_orb_capacity_gpu.py holds
the GPU to it.
"""
import numpy as np

from oracle import orb as oracle_orb

# The capacities, as mono_slam_framework_amd/csrc/orb_plan.h documents them (plan_orb sizes the lists;
# tests/test_orb_plan_host.py compares these restatements with the compiled plan):
KP_CAP = 2048          # kKpCap: final key points of a frame
S1_CAP = 8192          # kS1Cap: key points of a level kept by retainBest(2N) on the FAST score (ties included)


def _align16(n):
    return (n + 15) & ~15


def full_list(w, h):
    """Entries of a level's FULL candidate list (a dense call lists every strict FAST maximum at fastThreshold there):
    w h / 8, at least 4096."""
    return _align16(max(w * h // 8, 4096))


def primary_list(w, h):
    """Entries of a level's PRIMARY candidate list (a streaming call): w h / 64, at least kS1Cap; a level whose full list
    is at most 16 K entries keeps the full list."""
    cap = full_list(w, h)
    p = _align16(max(w * h // 64, S1_CAP))
    return cap if (p > cap or cap <= 16384) else p


def stage1_cap(w, h):
    """Stage-1 key points a level may keep in every call form: min(kS1Cap, full list)."""
    return min(S1_CAP, full_list(w, h))


class Capacity:
    """What the oracle's counts say about one frame.  `maxima[l]`: strict 3x3 FAST maxima at fastThreshold inside the
    31-px border (the kernels count after the border reject, as fast_level does); `stage1[l]`: retainBest(2N) survivors
    of level l; `kp`: final key points.

    `loud` lists the caps a frame exceeds that make EVERY call form return n_out = -1 (a stage-1 list, the key-point
    list).  `dense_only` lists the one that only a dense call (fewer than eight frames, MSF_FLAG_FAST_DENSE) meets: more
    maxima than the full list (a streaming call lists only the level's stage-1 candidates).  `over` = either."""

    def __init__(self, sizes, maxima, stage1, kp):
        self.sizes, self.maxima, self.stage1, self.kp = sizes, maxima, stage1, kp
        self.loud, self.dense_only = [], []
        for l, ((w, h), m, s) in enumerate(zip(sizes, maxima, stage1)):
            if s > stage1_cap(w, h):
                self.loud.append("L%d stage 1 %d > %d" % (l, s, stage1_cap(w, h)))
            if m > full_list(w, h):
                self.dense_only.append("L%d maxima %d > full list %d" % (l, m, full_list(w, h)))
        if kp > KP_CAP:
            self.loud.append("key points %d > %d" % (kp, KP_CAP))
        self.over = bool(self.loud or self.dense_only)
        # levels whose maxima do not fit the primary list: a streaming call that sends such a level through the dense
        # pass must still list its stage 1 exactly (the case the old shared pool of full-size lists served)
        self.primary_overflow = [l for l, ((w, h), m) in enumerate(zip(sizes, maxima)) if m > primary_list(w, h)]

    def __repr__(self):
        return "Capacity(maxima=%s, stage1=%s, kp=%d, loud=%s, dense_only=%s)" % (
            self.maxima, self.stage1, self.kp, self.loud, self.dense_only)


_oracles = {}


def _oracle(w, h):
    if (w, h) not in _oracles:
        _oracles[(w, h)] = oracle_orb.OrbOracle(w, h)
    return _oracles[(w, h)]


def capacity(img):
    """Run the oracle on one frame (cv::ORB::create() defaults) and return its Capacity."""
    h, w = img.shape
    o = _oracle(w, h)
    kps, _ = o.extract(np.ascontiguousarray(img))
    s1 = o.stage1_keypoints()
    sizes = [o.level_size(l) for l in range(o.nlevels)]
    maxima = [len(o.fast_candidates(l)) for l in range(o.nlevels)]
    stage1 = [int((s1["octave"] == l).sum()) for l in range(o.nlevels)]
    return Capacity(sizes, maxima, stage1, len(kps))


class OracleMatcher:
    """FeatureMatcherOracle.MatchFrames with each frame's features extracted once (frames repeat across batches)."""

    def __init__(self, ratio):
        self.ratio = ratio
        self._feat = {}

    def features(self, img):
        key = (img.shape, img.tobytes())
        if key not in self._feat:
            h, w = img.shape
            self._feat[key] = _oracle(w, h).extract(np.ascontiguousarray(img))
        return self._feat[key]

    def match(self, a, b):
        (k1, d1), (k2, d2) = self.features(a), self.features(b)
        return oracle_orb.knn_match(k1, d1, k2, d2, self.ratio)


# ---------------------------------------------------------------------------------------------------- generators
# Every generator is deterministic (fixed seed) and cheap; the oracle runs through a 1280 x 720 frame of any of them in
# well under a second.

def noise(w, h, sigma, seed=0):
    """Gaussian noise around 128: tens of thousands of FAST maxima per level, few hundred stage-1 key points."""
    rng = np.random.default_rng(1000 + seed * 97 + int(sigma))
    return np.clip(np.rint(rng.normal(128.0, sigma, (h, w))), 0, 255).astype(np.uint8)


def weak_dots(w, h, seed=0):
    """Isolated single-pixel dots, 3 to 5 px apart, on a background with +-1 of noise; contrast 21..24, so their FAST
    scores sit at 20..23 (the background noise moves them and breaks Harris ties), and one dot in 64 strong (contrast
    40..90).  Many corners just above fastThreshold, few strong ones: a first threshold taken from the strong tail
    overshoots and the level goes through the dense pass, whose maxima do not fit the primary list."""
    rng = np.random.default_rng(2000 + seed)
    img = (100 + rng.integers(-1, 2, (h, w))).astype(np.int16)
    for y in range(4, h - 4, 4):
        xs = np.arange(4 + (y // 4) % 2 * 2, w - 4, 4)
        jit = rng.integers(-1, 2, xs.size)
        c = rng.integers(21, 25, xs.size)
        strong = rng.random(xs.size) < 1.0 / 64
        c[strong] = rng.integers(40, 91, int(strong.sum()))
        sign = np.where(rng.random(xs.size) < 0.5, 1, -1)
        img[y + jit, xs] = 100 + sign * c
    return np.clip(img, 0, 255).astype(np.uint8)


def adversarial(w, h):
    """The three pathological textures of tests/test_orb_gpu.py."""
    y, x = np.mgrid[0:h, 0:w]
    chk = (((x // 2) + (y // 2)) % 2 * 200 + 20).astype(np.uint8)             # 2x2 checkerboard: dense corners
    dots = np.full((h, w), 30, np.uint8)
    dots[::4, ::4] = 250                                                       # isolated bright dots every 4 px
    rng = np.random.default_rng(5)
    salt = (rng.random((h, w)) < 0.08).astype(np.uint8) * 220 + 10             # salt noise
    return [("checker2", chk), ("dots4", dots), ("salt", salt)]


def flat(w, h):
    """Frames with no corner on some or all levels: constant, 0/255 saturation, a shallow gradient."""
    y, x = np.mgrid[0:h, 0:w]
    sat = np.where(((x // 97) + (y // 61)) % 2 == 0, 0, 255).astype(np.uint8)  # large saturated blocks
    grad = (x * 64 // w + y * 32 // h + 80).astype(np.uint8)                  # at most one grey level per 10+ px
    return [("constant", np.full((h, w), 77, np.uint8)), ("saturated", sat), ("gradient", grad)]


# name -> (builder(w, h), expected class): "within" frames must come back bit-exact in every call form, "over" frames
# loud in every call form
GENERATORS = {
    "noise16": (lambda w, h: noise(w, h, 16), "within"),
    "noise20": (lambda w, h: noise(w, h, 20), "within"),
    "noise30": (lambda w, h: noise(w, h, 30), "within"),
    "noise45": (lambda w, h: noise(w, h, 45), "within"),
    "weak_dots": (weak_dots, "within"),
    "checker2": (lambda w, h: adversarial(w, h)[0][1], "within"),
    "dots4": (lambda w, h: adversarial(w, h)[1][1], "over"),
    "salt": (lambda w, h: adversarial(w, h)[2][1], "over"),
    "constant": (lambda w, h: flat(w, h)[0][1], "flat"),
    "saturated": (lambda w, h: flat(w, h)[1][1], "flat"),
    "gradient": (lambda w, h: flat(w, h)[2][1], "flat"),
}
# generators whose frames send levels through the dense pass with more maxima than the primary list holds
DENSE_PASS = ("noise16", "noise20", "noise30", "noise45", "weak_dots")


def frame(name, w, h):
    return GENERATORS[name][0](w, h)


def kind(name):
    return GENERATORS[name][1]
