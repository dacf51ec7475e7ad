"""The grouped HDV traffic call on the MI355X (pdmpc_hdv_traffic_grouped, csrc/hdv_kernel.hip): every group's slices
against pdmpc_hdv_traffic_host for that group alone, bit for bit -- lists, rows, offsets, vertices, flags, adjacency --, with several
maps resident in the handle's map slots; the edges of the scan pass, the capacity protocol, the limits and the refusals."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import hdv_cases as H
from pdmpc import backend, hdv
from pdmpc.backend import Handle
from pdmpc.config import Config, MpaType, ScenarioType

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the slots of one tile of the scan pass (its workgroup's lanes), from the code: at Hp 1 an HDV has MAX_CHAINS slots
SCAN_TILE = int(re.search(r"#define PDMPC_HDV_SCAN_BLOCK (\d+)", open(os.path.join(ROOT, "p-dmpc_amd", "csrc", "pdmpc_device.h")).read()).group(1))
TILE_HDVS = SCAN_TILE // hdv.MAX_CHAINS
ZERO = (0.0, 0.0)
LAB, HAND = 0, 1  # the map slots of the module's handle


@pytest.fixture(scope="module")
def handle():
    h = Handle(Config(scenario_type=ScenarioType.commonroad, Hp=6, mpa_type=MpaType.single_speed, max_vehicles=8))
    yield h
    h.close()


def _maps():
    return {LAB: hdv.lab_hdv_map(), HAND: H.hand_map()}


def _upload(handle, Hp):
    for slot, m in _maps().items():
        handle.upload_hdv_map(m, H.local_sets(Hp), slot=slot)


def _lab_poses():
    """poses on the lab map by what they reach: the point with 8 closest lanelets, the fork, 1 m off the road (empty early steps), a straight"""
    lab = hdv.lab_hdv_map()
    xo, yo, yawo = H.along(lab, 64, 3)
    return [H.along(lab, 17, 10), H.along(lab, 3, 3), (xo - 1.0 * math.sin(yawo), yo + 1.0 * math.cos(yawo), yawo), H.along(lab, 64, 3)]


def _groups(Hp):
    """(slot, case) in the order slot 1, 0, 1, 0 with (HDVs, CAVs) = (2, 3), (0, 2), (1, 0), (3, 5): the hand-made graph with a tile
    offset (both HDVs and two of the CAVs on the copy 12 m away), CAVs without an HDV, an HDV without CAVs, and the lab map's fork,
    8-lanelet point and empty-intersection pose"""
    maps, sets = _maps(), H.local_sets(Hp)
    tile = (12.0, 0.0)
    p8, pf, po, _ = _lab_poses()
    return [
        (HAND, H.Case("hand-made graph on a tile", maps[HAND], sets, [(0.5 + 12.0, 0.0, 0.0, 1, tile), (1.0 + 12.0, -0.5, 0.4636476090008061, 1, tile)],
                      [(1.5 + 12.0, 0.0, 1, tile), (0.2 + 12.0, 0.0, 1, tile), (3.0, 0.0, 2, ZERO)])),
        (LAB, H.Case("no HDV", maps[LAB], sets, [], H._cavs(maps[LAB], [3, 5]))),
        (HAND, H.Case("no CAV", maps[HAND], sets, [(1.0, -0.5, 0.4636476090008061, 1, ZERO)], [])),
        (LAB, H.Case("8 lanelets, the fork, off the road", maps[LAB], sets, [p8 + (1, ZERO), pf + (1, ZERO), po + (1, ZERO)], H._cavs(maps[LAB], [17, 3, 5, 64, 66]))),
    ]


def _call(handle, groups, **kw):
    return handle.hdv_traffic_grouped([(slot,) + case.args() for slot, case in groups], **kw)


def _assert_groups(got, groups):
    assert len(got) == len(groups)
    for g, (r, (_, case)) in enumerate(zip(got, groups)):
        H.assert_same(r, case.host(), "group %d: %s" % (g, case.name))


@pytest.mark.parametrize("Hp", [1, 6])
def test_groups_equal_the_host_twin_group_by_group(handle, Hp):
    _upload(handle, Hp)
    groups = _groups(Hp)
    got = _call(handle, groups)
    _assert_groups(got, groups)
    assert handle.hdv_kernel_ms() > 0.0
    assert got[3]["adjacency"].shape == (5, 3) and got[1]["adjacency"].shape == (2, 0) and got[2]["adjacency"].shape == (0, 1)
    assert len(got[3]["closest"][0]) == 8
    # ... and the ungrouped device call with that map in slot 0 (the slot pdmpc_hdv_traffic reads): the same bytes
    handle.upload_hdv_map(groups[0][1].hmap, H.local_sets(Hp))
    H.assert_same(got[0], groups[0][1].device(handle), "group 0 against pdmpc_hdv_traffic")
    H.assert_same(got[2], groups[2][1].device(handle), "group 2 against pdmpc_hdv_traffic")
    _upload(handle, Hp)
    assert _call(handle, []) == []
    # several groups on one slot, and the same groups in another order
    again = [groups[3], groups[3], groups[0]]
    _assert_groups(_call(handle, again), again)


def _edge_groups(total):
    """`total` HDVs on the lab map at Hp 1 (MAX_CHAINS slots each), their poses cycling through _lab_poses, cut into groups after 1 HDV
    (inside a wavefront and a tile), at the wavefront's edge (64 slots), at the tile's edge and at twice the tile's, as far as there
    are HDVs; a CAV per group"""
    lab, sets, poses = hdv.lab_hdv_map(), H.local_sets(1), _lab_poses()
    cuts = sorted({0, total} | {c for c in (1, 64 // hdv.MAX_CHAINS, TILE_HDVS, 2 * TILE_HDVS) if c < total})
    return [(LAB, H.Case("HDVs %d..%d of %d" % (a, b, total), lab, sets, [poses[q % len(poses)] + (1, ZERO) for q in range(a, b)], H._cavs(lab, [3 + a % 3])))
            for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("total", [3, 4, 5, TILE_HDVS - 1, TILE_HDVS, TILE_HDVS + 1, 2 * TILE_HDVS + 1])
def test_the_scan_at_the_edges_of_a_wavefront_and_of_its_tile(handle, total):
    """The scan pass walks tiles of PDMPC_HDV_SCAN_BLOCK slots (TILE_HDVS HDVs at Hp 1) in wavefronts of 64: 48, 64 and 80 slots, one
    HDV below, at and above a tile, and above two tiles (the carry between tiles twice), with group boundaries inside a tile, at a
    wavefront's edge and exactly on the tile's edges."""
    assert SCAN_TILE == 256 and TILE_HDVS == 16
    handle.upload_hdv_map(hdv.lab_hdv_map(), H.local_sets(1), slot=LAB)
    groups = _edge_groups(total)
    _assert_groups(_call(handle, groups), groups)


@pytest.mark.parametrize("short_in", ["last", "first"])
def test_capacity_protocol(handle, short_in):
    """Exact room and more room give the result; one vertex short -- the missing vertex in the last group, then (the groups behind it
    without vertices) in the first -- is PDMPC_ERR_CAPACITY with every offset and set_base entry right and nothing written at or
    beyond the capacity in the caller's arrays (NaN guards behind the buffers).  The guards see the host's copies only: in the short
    case the call copies no vertex back.  The device's own bound (hdv_copy_slot stores nothing at or beyond the capacity: behind
    x's room stands y's in the workspace) cannot be seen through the call and is not tested here, as it is not for the ungrouped call."""
    _upload(handle, 6)
    groups = _groups(6)
    if short_in == "first":
        groups = [groups[3], groups[1], groups[1]]
    host = [case.host() for _, case in groups]
    totals = [int(r["set_offset"][-1]) for r in host]
    total = sum(totals)
    assert total > 0 and (totals[-1] > 0) == (short_in == "last")
    _assert_groups(_call(handle, groups, capacity=total), groups)
    _assert_groups(_call(handle, groups, capacity=total + 1000), groups)
    with pytest.raises(backend.CapacityError) as e:
        _call(handle, groups, capacity=total - 1)
    assert e.value.count == total
    raw = {}
    got = _call(handle, groups, capacity=total - 1, raw=raw, guard=64)
    assert raw["rc"] == backend.ERR_CAPACITY
    assert raw["set_base"].tolist() == np.concatenate([[0], np.cumsum(totals)]).tolist()
    for r, ref in zip(got, host):
        assert np.array_equal(r["set_offset"], ref["set_offset"]) and r["closest"] == ref["closest"] and r["row_hdv"] == ref["row_hdv"]
        assert np.array_equal(r["adjacency"], ref["adjacency"]) and np.array_equal(r["flags"], ref["flags"])
    assert np.isnan(raw["set_x"][total - 1:]).all() and np.isnan(raw["set_y"][total - 1:]).all()
    _assert_groups(_call(handle, groups), groups)  # (the sized second call)


def test_limits_and_refusals(handle):
    lab, tri = hdv.lab_hdv_map(), H.ngon_sets(3, 1)
    x, y, yaw = H.along(lab, 64, 3)
    handle.upload_hdv_map(lab, tri, slot=LAB)
    good = [(LAB, H.Case("1 HDV", lab, tri, [(x, y, yaw, 1, ZERO)], H._cavs(lab, [64])))]

    def refused(groups, status):
        with pytest.raises(backend.BackendError) as e:
            _call(handle, groups)
        assert e.value.status == status, str(e.value)
        _assert_groups(_call(handle, good), good)  # the handle works for the next call
        return str(e.value)

    full = [(LAB, H.Case("64 HDVs in a group", lab, tri, [(x, y, yaw, 1, ZERO)] * 64, []))]
    _assert_groups(_call(handle, full), full)
    refused([(LAB, H.Case("65 HDVs in a group", lab, tri, [(x, y, yaw, 1, ZERO)] * 65, []))], backend.ERR_CAPACITY)
    forty_three = (LAB, H.Case("43 HDVs", lab, tri, [(x, y, yaw, 1, ZERO)] * 43, []))
    refused([forty_three] * 3, backend.ERR_CAPACITY)  # 129 in the call
    assert "group 1" in refused([good[0], (7, good[0][1])], -1)  # a slot never uploaded
    refused([(8, good[0][1])], -1)
    with pytest.raises(backend.BackendError) as e:
        handle.upload_hdv_map(lab, tri, slot=8)
    assert e.value.status == -1
    handle.upload_hdv_map(H.hand_map(), H.local_sets(6), slot=HAND)  # Hp 6 beside Hp 1
    assert "Hp" in refused([good[0], (HAND, H.Case("on the Hp 6 slot", H.hand_map(), H.local_sets(6), [(0.5, 0.0, 0.0, 1, ZERO)], []))], -1)
    assert "group 1" in refused([good[0], (LAB, H.Case("bad trim", lab, tri, [(x, y, yaw, 2, ZERO)], []))], -1)
    assert "group 0" in refused([(LAB, H.Case("bad lanelet", lab, tri, [(x, y, yaw, 1, ZERO)], [(0.0, 0.0, 105, ZERO)]))], -1)


def test_one_group_runs_over_its_lists_and_the_others_come_back_whole(handle):
    """17 lanelets on one spot: an HDV there has more than PDMPC_HDV_MAX_CHAINS closest lanelets.  Its group gets n_rows -1 and the
    call PDMPC_ERR_CAPACITY; the groups in front of and behind it hold what they hold alone."""
    _upload(handle, 6)
    sq = [(0.0, 0.5), (1.0, 0.5)], [(0.0, -0.5), (1.0, -0.5)]
    many = hdv.HdvMap([sq[0]] * 17, [sq[1]] * 17, [[]] * 17, np.zeros((17, 17), dtype=np.uint8))
    handle.upload_hdv_map(many, H.local_sets(6), slot=2)
    groups = _groups(6)
    over = (2, H.Case("17 lanelets", many, H.local_sets(6), [(0.5, 0.0, 0.0, 1, ZERO)], [(0.5, 0.0, 1, ZERO)]))
    mixed = [groups[3], over, groups[0]]
    with pytest.raises(backend.BackendError) as e:
        _call(handle, mixed)
    assert e.value.status == backend.ERR_CAPACITY and "group 1" in str(e.value)
    raw = {}
    got = _call(handle, mixed, raw=raw)
    assert raw["rc"] == backend.ERR_CAPACITY and raw["n_rows"].tolist()[1] == -1 and got[1] is None
    H.assert_same(got[0], groups[3][1].host(), "the group in front")
    H.assert_same(got[2], groups[0][1].host(), "the group behind")


def test_slot_generations_and_the_content_check(handle):
    g0, n0 = handle.hdv_map_slot_state(5)
    assert g0 == 0 and hdv.hdv_map_slot_hp(handle, 5) == 0 and not handle.hdv_map_slot_holds(5, H.u_map(), H.local_sets(6))
    handle.upload_hdv_map(H.u_map(), H.local_sets(6), slot=5)
    g1, n1 = handle.hdv_map_slot_state(5)
    handle.upload_hdv_map(H.u_map(), H.local_sets(6), slot=5)
    g2, n2 = handle.hdv_map_slot_state(5)
    assert 0 < g1 < g2 and (n1, n2) == (n0 + 1, n0 + 2) and hdv.hdv_map_slot_hp(handle, 5) == 6
    # pdmpc_hdv_map_slot_holds on the handle: the map and the sets that were uploaded, and nothing that differs from them by a bit
    assert handle.hdv_map_slot_holds(5, H.u_map(), H.local_sets(6))
    assert not handle.hdv_map_slot_holds(5, H.u_map(), H.local_sets(1))  # another Hp
    assert not handle.hdv_map_slot_holds(5, H.hand_map(), H.local_sets(6))  # another map
    assert not handle.hdv_map_slot_holds(5, H.u_map(), H.ngon_sets(3, 6))  # other hulls
    moved = H.u_map()
    nudged = hdv.HdvMap([np.nextafter(np.asarray(b, dtype=np.float64), np.inf) for b in moved.left], moved.right, [[]], np.zeros((1, 1), dtype=np.uint8))
    assert not handle.hdv_map_slot_holds(5, nudged, H.local_sets(6))  # every left point one ulp away
    assert handle.hdv_map_slot_state(5) == (g2, n2)  # (asking uploads nothing)


def test_the_wrapper_sizes_its_arrays_by_the_slots_own_hp(handle):
    """The Python wrapper asks the handle for the Hp of the groups' slots: a map uploaded through the C ABI alone (as a controller's
    traffic stage does), or one that replaced a map of another Hp, is sliced by the Hp it has."""
    lab, sets = hdv.lab_hdv_map(), H.local_sets(6)
    handle.upload_hdv_map(lab, H.local_sets(1), slot=6)
    L = backend.load_library()
    args, keep = lab.arrays()
    ps, pkeep = backend.pack_local_sets(sets)
    assert L.pdmpc_upload_hdv_map_slot(handle.h, 6, *args, len(sets), 6, ctypes.byref(ps)) == 0  # (behind the wrapper's back: Hp 6 over Hp 1)
    del keep, pkeep
    x, y, yaw = H.along(lab, 3, 3)
    groups = [(6, H.Case("one HDV on slot 6", lab, sets, [(x, y, yaw, 1, ZERO)], H._cavs(lab, [3, 5])))]
    _assert_groups(_call(handle, groups), groups)
