"""CPU: the host build of csrc/ba_solve.h (tests/cpp/ba_solve_host.cpp: g++ -ffp-contract=off, one thread) against the
float64 reference of tests/ba_ref.py, with the bars the device is held to in tests/test_ba_gpu.py."""
import numpy as np
import pytest

from tests import ba_host
from tests import ba_ref as br


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ba_host.build(tmp_path_factory.mktemp("ba_host"))


@pytest.mark.parametrize("name", list(br.SCENES))
def test_scenes_meet_the_float64_bars(host, name):
    got = ba_host.run(host, br.scene(name), br.schedule_of(name))
    clear, run, step, final = br.check_result(got, name, "host " + name)
    print("%s: %d clear iterations of %d, worst step %.3g and final %.3g of their bars" % (name, clear, run, step, final))


def test_stop_word_preset(host):
    sc = br.scene("p64")
    got = ba_host.run(host, sc, br.LOCAL_BA, stop=1)
    ref = br.run(sc, br.LOCAL_BA, stop=True)
    assert got["status"] == 0 and (got["it_trials"] == 0).all() and (got["round_iterations"] == 0).all()
    assert got["cam_Tcw"].tobytes() == sc["cam_Tcw"].tobytes() and got["points"].tobytes() == sc["points"].tobytes()
    assert (got["outliers"] == ref["outliers"]).all()
    assert ba_host.run(host, sc, br.LOCAL_BA, stop=0)["status"] == 2


def test_malformed_problems_get_minus_one_and_nothing_else(host):
    sc = dict(br.scene("p63"))
    for what in ("cam", "point", "order", "free"):
        bad = dict(sc)
        bad["edge_cam"], bad["edge_point"] = sc["edge_cam"].copy(), sc["edge_point"].copy()
        max_free = 64
        if what == "cam":
            bad["edge_cam"][17] = len(sc["cam_Tcw"])
        elif what == "point":
            bad["edge_point"][-1] = len(sc["points"])
        elif what == "order":
            bad["edge_point"][[3, 200]] = bad["edge_point"][[200, 3]]
        else:
            max_free = 2
        got = ba_host.run(host, bad, br.LOCAL_BA, max_free=max_free)
        assert got["status"] == -1, what
        for k, v in got.items():
            if k != "status":
                assert not np.asarray(v).any(), (what, k)


def test_one_round_of_bundle_adjustment_without_a_kernel(host):
    sc = br.scene("p65")
    schedule = (1, (8, 0), (0, 0))
    got = ba_host.run(host, sc, schedule)
    br.check_result(got, None, "host BundleAdjustment", sc=sc, schedule=schedule, final=False)


def test_another_huber_delta(host):
    sc = br.scene("p63")
    schedule = (1, (4, 0), (1, 0))
    got = ba_host.run(host, sc, schedule, huber_delta2=5.99)
    ref = br.run(sc, schedule, huber_delta2=5.99)
    assert (got["it_trials"] == ref["it_trials"]).all()
    assert np.allclose(got["it_cost_in"], ref["it_cost_in"], rtol=1e-12, atol=0)
    base = ba_host.run(host, sc, schedule)
    assert not np.array_equal(base["it_cost_in"], got["it_cost_in"])
