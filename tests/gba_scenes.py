"""The scenes of the global bundle adjustment tests (CPU and GPU): tests/ba_ref.make_scene above the old cap of 64 free
cameras, at the tile edges of the device Cholesky, and one whose entry estimates lie further off, so that the
Levenberg-Marquardt loop rejects trials.  tests/test_gba_scenes.py asserts on the CPU what the GPU tests rely on."""
import numpy as np

from tests import ba_ref as br

GLOBAL_BA = (1, (10, 0), (0, 0))                      # Optimizer.cc:62-69: BundleAdjustment(10 iterations), not robust
# The bars scene.  BundleAdjustment's schedule has no Huber kernel, and with make_scene's 5 % of gross outliers no draw
# of the (80 + 2) x 400 scene meets ba_ref.scene_conditions under it (seeds 1 .. 60: no free pose ends nearer the truth).
# The scene for the float64 bars is therefore drawn with outliers = 0; G80_CLEAN_SEED is the first draw that meets them.
G80_CLEAN_SEED = 1
# twice the (80 + 2) x 400 scene's own spread under ba_ref.measure_bars (profiles/gba_bars.txt), never above STEP_BAR
G80_STEP_SPREAD = 1.0125233984581428e-13
REJECTED_TRIALS = [1, 2, 3, 1, 1, 1, 4, 1, 1, 1]      # what the host build runs on "rejected"

_SPECS = {
    "s65": ((65, 1, 260, None, 1), br.LOCAL_BA),
    "g80": ((80, 2, 400, None, 1), GLOBAL_BA),
    "g80_clean": ((80, 2, 400, None, G80_CLEAN_SEED, 0.0), GLOBAL_BA),
    "s130": ((130, 1, 520, None, 1), (1, (3, 0), (0, 0))),
    "larger": ((90, 1, 360, None, 2), (1, (2, 0), (0, 0))),
}
_CACHE = {}


def far_off(sc, seed, rotation=0.1, shift=0.2, points=0.1):
    """the scene with every free camera rotated by `rotation` rad and shifted by about `shift` more, the points moved by
    up to `points` of their coordinates"""
    rng = np.random.default_rng(seed)
    out = dict(sc)
    T = sc["cam_Tcw"].reshape(-1, 3, 4).astype(np.float64)
    for c in range(len(T)):
        if sc["cam_fixed"][c]:
            continue
        a = rng.normal(size=3)
        dR = br._rotation(a / np.linalg.norm(a) * rotation)
        T[c, :, :3] = dR @ T[c, :, :3]
        T[c, :, 3] = dR @ T[c, :, 3] + rng.normal(size=3) * shift
    out["cam_Tcw"] = T.reshape(-1, 12).astype(np.float32)
    out["points"] = (sc["points"] * (1 + rng.uniform(-points, points, sc["points"].shape))).astype(np.float32)
    return out


def tile_edge_sizes(tile):
    """for k = 1, 2, 3 the largest n_free with 6 n_free <= k tile, and the next one"""
    return [n for k in (1, 2, 3) for n in (k * tile // 6, k * tile // 6 + 1)]


def scene(name):
    """-> (scene, schedule)"""
    if name not in _CACHE:
        if name in _SPECS:
            args, schedule = _SPECS[name]
            _CACHE[name] = (br.make_scene(*args), schedule)
        elif name == "rejected":
            _CACHE[name] = (far_off(br.make_scene(70, 2, 300, None, 1), 1), GLOBAL_BA)
        elif name == "nan":
            sc = dict(br.make_scene(20, 2, 80, None, 1))
            sc["edge_obs"] = sc["edge_obs"].copy()
            sc["edge_obs"][17, 1] = np.nan
            _CACHE[name] = (sc, GLOBAL_BA)
        elif name.startswith("t"):                    # "t<n_free>": two fixed cameras, 4 n_free points
            n = int(name[1:])
            _CACHE[name] = (br.make_scene(n, 2, 4 * n, None, 1), (1, (4, 0), (0, 0)))
        elif name == "lonely":
            # camera 0 is free and has no edge; every camera of point 0 is fixed
            sc = dict(br.make_scene(12, 3, 60, None, 1))
            fixed = np.flatnonzero(sc["cam_fixed"])
            free = np.flatnonzero(sc["cam_fixed"] == 0)
            ec = sc["edge_cam"].copy()
            ec[ec == free[0]] = free[1]
            first = np.flatnonzero(sc["edge_point"] == 0)
            ec[first] = fixed[np.arange(len(first)) % len(fixed)]
            sc["edge_cam"] = ec
            _CACHE[name] = (sc, br.LOCAL_BA)
        else:
            raise KeyError(name)
    return _CACHE[name]


def n_free(sc):
    return int((np.asarray(sc["cam_fixed"]) == 0).sum())


def first_usable_g80_seed(limit=20, outliers=0.0):
    for seed in range(1, limit):
        sc = br.make_scene(80, 2, 400, None, seed, outliers)
        if not br.scene_conditions(sc, GLOBAL_BA, br.run(sc, GLOBAL_BA)):
            return seed
    return None


def measure_g80(log=print):
    """ba_ref.measure_bars on the (80 + 2) x 400 scene alone -> (step spread, final spread, chaotic)"""
    br.SCENES["g80_clean"] = _SPECS["g80_clean"][0][:5] + (GLOBAL_BA,)
    br._SCENES["g80_clean"] = scene("g80_clean")[0]
    try:
        return br.measure_bars(["g80_clean"], log=log)
    finally:
        del br.SCENES["g80_clean"]
        br._SCENES.pop("g80_clean", None)
        br._RUNS.pop("g80_clean", None)


if __name__ == "__main__":
    print("first usable seed of the (80 + 2) x 400 scene, 5 %% gross outliers: %r" % first_usable_g80_seed(limit=61, outliers=0.05))
    print("first usable seed of the (80 + 2) x 400 scene, no gross outliers: %r" % first_usable_g80_seed())
    s, f, c = measure_g80()
    print("G80_STEP_SPREAD = %r\nfinal spread = %r\nchaotic = %r" % (s, f, tuple(c)))
