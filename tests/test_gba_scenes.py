"""CPU: what the GPU tests of the global bundle adjustment take for granted about their scenes (tests/gba_scenes.py) --
the seed of the float64-bars scene is the first usable draw, its step bar is no wider than ba_ref.STEP_BAR, the
"rejected" scene makes the host build reject trials and the "nan" scene makes it reject every trial and end."""
import numpy as np
import pytest

from tests import ba_host, ba_ref as br, gba_scenes as gs


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return ba_host.build(tmp_path_factory.mktemp("gba_scenes"))


def test_the_bars_scene_is_the_first_usable_draw():
    assert gs.first_usable_g80_seed(limit=gs.G80_CLEAN_SEED + 1) == gs.G80_CLEAN_SEED
    sc, schedule = gs.scene("g80_clean")
    assert gs.n_free(sc) == 80 and len(sc["cam_Tcw"]) == 82 and len(sc["points"]) == 400 and schedule == gs.GLOBAL_BA
    # with make_scene's gross outliers the first draw is not usable under a schedule without a Huber kernel
    noisy, _ = gs.scene("g80")
    assert br.scene_conditions(noisy, schedule, br.run(noisy, schedule)) != []
    assert 0 < 2 * gs.G80_STEP_SPREAD <= br.STEP_BAR


def test_the_rejected_and_nan_scenes_do_what_their_names_say(L):
    sc, schedule = gs.scene("rejected")
    assert gs.n_free(sc) <= 80
    r = ba_host.run(L, sc, schedule, max_free=gs.n_free(sc))
    trials = r["it_trials"][r["it_trials"] > 0].tolist()
    assert trials == gs.REJECTED_TRIALS and max(trials) >= 2 and r["status"] == 1
    sc, schedule = gs.scene("nan")
    r = ba_host.run(L, sc, schedule, max_free=gs.n_free(sc))
    assert r["it_trials"][r["it_trials"] > 0].tolist() == [10] and r["round_iterations"].tolist() == [1, 0]
    assert r["status"] == 1 and r["it_cam_out"][0].tobytes() == r["it_cam_in"][0].tobytes()   # nothing moved


def test_tile_edge_sizes():
    assert gs.tile_edge_sizes(64) == [10, 11, 21, 22, 32, 33]
    for n in gs.tile_edge_sizes(64):
        sc, _ = gs.scene("t%d" % n)
        assert gs.n_free(sc) == n and len(sc["points"]) == 4 * n and int(sc["cam_fixed"].sum()) == 2
