"""Human-driven vehicles on the MI355X (csrc/hdv_kernel.hip): pdmpc_hdv_traffic against its host twin bit for bit —
closest lists, rows, offsets, vertices, flags, adjacency — on the cases of tests/hdv_cases.py (the CPU half, against exact arithmetic,
is tests/test_hdv_host.py), and the capacity protocol."""
import numpy as np
import pytest

import hdv_cases as H
from pdmpc import backend, hdv
from pdmpc.backend import Handle
from pdmpc.config import Config, MpaType, ScenarioType

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

CASES = H.traffic_cases()


@pytest.fixture(scope="module")
def handle():
    h = Handle(Config(scenario_type=ScenarioType.commonroad, Hp=6, mpa_type=MpaType.single_speed, max_vehicles=8))
    yield h
    h.close()


def _upload(handle, case):
    handle.upload_hdv_map(case.hmap, case.sets)


def test_a_call_before_the_upload_is_refused():
    fresh = Handle(Config(scenario_type=ScenarioType.commonroad, Hp=6, mpa_type=MpaType.single_speed, max_vehicles=8))
    fresh.hdv_shape = (104, 6)  # (what upload_hdv_map would have noted: the wrapper sizes its arrays by it)
    with pytest.raises(backend.BackendError) as e:
        CASES[0].device(fresh)
    fresh.close()
    assert e.value.status == -1 and "before pdmpc_upload_hdv_map" in str(e.value)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_equals_host_twin(handle, case):
    _upload(handle, case)
    host, dev = case.host(), case.device(handle)
    H.assert_same(dev, host, case.name)
    assert handle.hdv_kernel_ms() > 0.0
    # the capacity protocol: one call with exactly the room needed gives the same; one vertex short is PDMPC_ERR_CAPACITY with the
    # count, and lists, rows, offsets and adjacency are there all the same (the sized second call is the default path above)
    total = int(host["set_offset"][-1])
    H.assert_same(case.device(handle, capacity=total), host, case.name)
    H.assert_same(case.device(handle, capacity=total + 1000), host, case.name)
    if total:
        with pytest.raises(backend.CapacityError) as e:
            case.device(handle, capacity=total - 1)
        assert e.value.count == total


def test_no_hdv_and_no_cav(handle):
    case = CASES[0]
    _upload(handle, case)
    none = H.Case("no HDV", case.hmap, case.sets, [], case.cavs)
    r = none.device(handle)
    assert r["closest"] == [] and r["row_hdv"] == [] and r["sets"] == [] and r["adjacency"].shape == (1, 0)
    alone = H.Case("no CAV", case.hmap, case.sets, case.hdvs, [])
    H.assert_same(alone.device(handle), alone.host(), "no CAV")


def test_invalid_and_oversized_calls(handle):
    case = CASES[0]
    _upload(handle, case)
    x, y, yaw, _, tile = case.hdvs[0]
    for trim in (0, len(case.sets) + 1):
        with pytest.raises(backend.BackendError) as e:
            H.Case("bad trim", case.hmap, case.sets, [(x, y, yaw, trim, tile)], case.cavs).device(handle)
        assert e.value.status == -1
    with pytest.raises(backend.BackendError) as e:
        H.Case("bad lanelet", case.hmap, case.sets, case.hdvs, [(0.0, 0.0, 105, tile)]).device(handle)
    assert e.value.status == -1
    # 17 lanelets on one spot: more closest lanelets than PDMPC_HDV_MAX_CHAINS
    sq = [(0.0, 0.5), (1.0, 0.5)], [(0.0, -0.5), (1.0, -0.5)]
    many = hdv.HdvMap([sq[0]] * 17, [sq[1]] * 17, [[]] * 17, np.zeros((17, 17), dtype=np.uint8))
    handle.upload_hdv_map(many, H.local_sets(6))
    with pytest.raises(backend.BackendError) as e:
        H.Case("17 lanelets", many, H.local_sets(6), [(0.5, 0.0, 0.0, 1, (0.0, 0.0))], []).device(handle)
    assert e.value.status == backend.ERR_CAPACITY
    # more HDVs than PDMPC_HDV_MAX_VEHICLES (config.max_vehicles, 8 here, is not a limit of this call: 9 HDVs and 9 CAVs are fine)
    _upload(handle, case)
    nine = H.Case("9 HDVs, 9 CAVs", case.hmap, case.sets, case.hdvs * 9, case.cavs * 9)
    H.assert_same(nine.device(handle), nine.host(), nine.name)
    with pytest.raises(backend.BackendError) as e:
        H.Case("65 HDVs", case.hmap, case.sets, case.hdvs * 65, []).device(handle)
    assert e.value.status == backend.ERR_CAPACITY


def test_two_regions_and_the_hand_made_graph(handle):
    """PDMPC_BOUND_MULTIPLE on the device, and the adjacency cases of the 3-lanelet graph in one call of 2 HDVs and 4 CAVs"""
    u = H.Case("two regions", H.u_map(), H.ngon_sets(12, 1, radius=1.0), [(0.5, 0.0, 0.0, 1, (0.0, 0.0))], [])
    _upload(handle, u)
    dev = u.device(handle)
    H.assert_same(dev, u.host(), u.name)
    assert int(dev["flags"][0, 0]) == 2
    hm = H.hand_map()
    g = H.Case("hand-made graph", hm, H.local_sets(6), [(0.5, 0.0, 0.0, 1, (0.0, 0.0)), (1.0, -0.5, 0.4636476090008061, 1, (0.0, 0.0))],
               [(1.5, 0.0, 1, (0.0, 0.0)), (0.2, 0.0, 1, (0.0, 0.0)), (3.0, 0.0, 2, (0.0, 0.0)), (1.5, 0.0, 1, (12.0, 0.0))])
    _upload(handle, g)
    dev = g.device(handle)
    H.assert_same(dev, g.host(), g.name)
    assert dev["adjacency"].tolist() == [[0, 0], [1, 1], [0, 0], [0, 0]]
