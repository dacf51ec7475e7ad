"""The HDV driver model on the MI355X (pdmpc_hdv_drive_kernel, csrc/hdv_kernel.hip): pdmpc_hdv_drive_grouped against
pdmpc_hdv_drive_host group by group, bit for bit -- state, pose, cos and sin, speed, gap --, and pdmpc_hdv_drive_traffic_grouped (the
drive launch in front of the five of the grouped traffic call) against the host twins of both, against pdmpc_hdv_traffic_grouped where
no group drives, with the capacity protocol and the refusals."""
import math

import numpy as np
import pytest

import hdv_cases as H
import hdv_drive_cases as D
from pdmpc import backend, hdv
from pdmpc.backend import Handle
from pdmpc.config import Config, MpaType, ScenarioType

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

LAB, HAND = 0, 1  # the map slots of the module's handle
ZERO, TILE, FAR = (0.0, 0.0), (12.0, 24.0), (50.0, 0.0)


@pytest.fixture(scope="module")
def handle():
    h = Handle(Config(scenario_type=ScenarioType.commonroad, Hp=6, mpa_type=MpaType.single_speed, max_vehicles=8))
    yield h
    h.close()


def _upload(handle, Hp):
    handle.upload_hdv_map(D.lab(), H.local_sets(Hp), slot=LAB)
    handle.upload_hdv_map(D.hand_map(), H.local_sets(Hp), slot=HAND)


def _members():
    """(slot, member) on the slots 1, 0, 1, 0 with (HDVs, CAVs) = (2, 3), (0, 2), (1, 0), (3, 5).
    0: over the segment of length 0 and slowed; the capped window of 64 segments against 3 CAVs and the other HDV: 320 items, five rounds
       of the lanes' stride.
    1: CAVs without an HDV.
    2: the capped window and no other vehicle but the HDV itself: (0 CAVs + 1 HDV) x 64 segments = exactly 64 items, one per lane.
    3: stopped inside gap_min; the wrap of the closed route, slowed by a CAV behind the wrap; a step over a lanelet joint on a copy of
       the map 12 m away, with a CAV of that copy behind it; two CAVs ahead of all of them on another copy, which nobody sees."""
    L, Hm, R = D.lab(), D.hand_map(), D.loop_route()
    total = D.route_length(L, R)
    first = sum(hdv._route_segment(L, R[0], R[1], 0, j)[4] for j in range(hdv._route_segments(L, R[0], R[1], 0)))
    r12, r4 = ([1, 2], False), ([4], False)
    return [
        (HAND, D.Member("length 0 and the cap", Hm, [(r12, 0.95, ZERO, 2.0), (r4, 0.0, ZERO, 0.5)], [(1.75, 0.0, ZERO), (0.5, 5.0, ZERO), (0.8, 5.0, ZERO)])),
        (LAB, D.Member("no HDV", L, [], [D.at(L, R, 1.0) + (ZERO,), D.at(L, R, 2.0) + (ZERO,)])),
        (HAND, D.Member("exactly 64 items", Hm, [(r4, 0.0, ZERO, 0.5)], [])),
        (LAB, D.Member("stopped, wrap, joint, other tiles", L, [(R, 0.7, ZERO, 0.5), (R, total - 0.01, ZERO, 0.5), (R, first - 0.05, TILE, 3.0)],
                       [D.at(L, R, 0.9) + (ZERO,), D.at(L, R, 0.5) + (ZERO,), D.at(L, R, first - 0.5, TILE) + (TILE,), D.at(L, R, 1.0, FAR) + (FAR,), D.at(L, R, 0.75, FAR) + (FAR,)])),
    ]


def _assert_members(got, members):
    assert len(got) == len(members)
    out = []
    for g, (r, (_, m)) in enumerate(zip(got, members)):
        ref = m.host()
        D.assert_same(r, ref, "group %d: %s" % (g, m.name))
        out.append(ref)
    return out


def test_groups_equal_the_host_twin_group_by_group(handle):
    _upload(handle, 1)
    members = _members()
    got = hdv.drive_grouped_native(handle, [m.group(slot) for slot, m in members])
    ref = _assert_members(got, members)
    assert handle.hdv_kernel_ms() > 0.0
    # what the groups are there for
    assert 0.0 < ref[0]["speed"][0] < 2.0 and ref[0]["states"][0][:2] == (0, 2) and 0.0 < ref[0]["speed"][1] < 0.5  # over the length 0, slowed; the CAV within the cap
    assert ref[1]["states"] == [] and ref[2]["speed"] == [0.5] and ref[2]["gap"] == [math.inf]
    s3 = ref[3]
    assert s3["speed"][0] == 0.0 and 0.0 < s3["speed"][1] < 0.5 and s3["states"][1][0] == 0 and s3["speed"][2] == 3.0 and s3["states"][2][0] == 1
    assert s3["gap"][2] == math.inf and s3["x"][2] > TILE[0] and s3["y"][2] > TILE[1]
    # the step after it, from the states the device gave; several groups on one slot and another order
    nxt = [(slot, m.after(r, m.name + ", next step")) for (slot, m), r in zip(members, got)]
    again = [nxt[3], nxt[0], nxt[3], nxt[2]]
    _assert_members(hdv.drive_grouped_native(handle, [m.group(slot) for slot, m in again]), again)
    assert hdv.drive_grouped_native(handle, []) == []


def test_65_hdvs_in_one_call(handle):
    """64 HDVs in a group (the limit) follow one another about 0.5 m apart round the lab map's longest loop, and one more in a second
    group: 65 wavefronts, every HDV of the first group against 2 CAVs and 63 others."""
    handle.upload_hdv_map(D.lab(), H.local_sets(1), slot=LAB)
    L, R = D.lab(), hdv.route_from_loop(54)
    assert D.route_length(L, R) > 64 * 0.51 + 0.5
    cavs = [D.at(L, R, 3.1) + (ZERO,), D.at(L, R, 9.33) + (ZERO,)]
    members = [(LAB, D.Member("64 in a row", L, [(R, 0.45 * q + 0.02 * (q % 4), ZERO, 0.5) for q in range(64)], cavs)), (LAB, D.Member("one more", L, [(R, 5.0, ZERO, 0.5)], cavs[:1]))]
    ref = _assert_members(hdv.drive_grouped_native(handle, [m.group(slot) for slot, m in members]), members)
    assert len({round(v, 6) for v in ref[0]["speed"]}) > 3 and min(ref[0]["speed"]) >= 0.0 and max(ref[0]["speed"]) <= 0.5


def _traffic_group(slot, m, drives, trim=1):
    """a member as a group of the combined call; one that does not drive brings the poses its states stand for"""
    poses = [hdv.state_pose(m.hmap, r[0], r[1], s, t) for r, s, t in zip(m.routes, m.states, m.tiles)]
    return m.group(slot, drives=drives, trim=[trim] * len(m.states), cav_lanelet=[1] * len(m.cav_x), x=[p[0] for p in poses], y=[p[1] for p in poses],
                   yaw=[math.atan2(p[3], p[2]) for p in poses])


def _traffic_reference(m, Hp, drives):
    """pdmpc_hdv_drive_host, then pdmpc_hdv_traffic_host on the poses it gives -- or, for a group that does not drive, on the poses it
    brought -- for the group alone -> (driven, traffic)"""
    sets = H.local_sets(Hp)
    n = len(m.states)
    if drives:
        d = m.host()
        x, y, cs = d["x"], d["y"], (d["cos_yaw"], d["sin_yaw"])
    else:
        g = _traffic_group(0, m, False)
        d, x, y, cs = None, g["x"], g["y"], ([math.cos(a) for a in g["yaw"]], [math.sin(a) for a in g["yaw"]])
    t = hdv.hdv_traffic_native(m.hmap, sets, x, y, [0.0] * n, [1] * n, m.tiles, m.cav_x, m.cav_y, [1] * len(m.cav_x), m.cav_tile, cos_sin=cs)
    return d, t


def _assert_combined(got, members, flags, Hp):
    for g, ((driven, traffic), (_, m), f) in enumerate(zip(got, members, flags)):
        ref_d, ref_t = _traffic_reference(m, Hp, f)
        assert (driven is None) == (not f)
        if f:
            D.assert_same(driven, ref_d, "group %d: %s" % (g, m.name))
        H.assert_same(traffic, ref_t, "group %d: %s" % (g, m.name))


@pytest.mark.parametrize("Hp", [1, 6])
def test_combined_call_equals_drive_then_traffic_on_the_host(handle, Hp):
    _upload(handle, Hp)
    members = _members()
    flags = [True] * 4
    got = hdv.drive_traffic_grouped_native(handle, [_traffic_group(slot, m, f) for (slot, m), f in zip(members, flags)], capacity=1 << 16)
    _assert_combined(got, members, flags, Hp)
    assert handle.hdv_kernel_ms() > 0.0
    assert sum(len(t["row_hdv"]) for _, t in got) > 0 and sum(int(t["set_offset"][-1]) for _, t in got) > 0


def test_a_call_in_which_no_group_drives_is_the_grouped_traffic_call(handle):
    _upload(handle, 6)
    members = _members()
    groups = [_traffic_group(slot, m, False) for slot, m in members]
    raw, ref = {}, {}
    hdv.drive_traffic_grouped_native(handle, groups, capacity=1 << 16, raw=raw)
    plain = [(g["slot"], g["x"], g["y"], g["yaw"], g["trim"], g["tiles"], g["cav_x"], g["cav_y"], g["cav_lanelet"], g["cav_tile"]) for g in groups]
    handle.hdv_traffic_grouped(plain, capacity=1 << 16, raw=ref)
    assert raw["rc"] == ref["rc"] == 0
    for key in ("closest_offset", "closest_index", "n_rows", "row_hdv", "set_offset", "set_base", "set_x", "set_y", "set_flags", "adjacency"):
        assert np.asarray(raw[key]).tobytes() == np.asarray(ref[key]).tobytes(), key


def test_a_mixed_call_drives_groups_0_and_2_only(handle):
    _upload(handle, 6)
    members = _members()
    flags = [True, False, True, False]
    groups = [_traffic_group(slot, m, f) for (slot, m), f in zip(members, flags)]
    groups[3]["routes"] = None  # (a group that does not drive needs no routes)
    got = hdv.drive_traffic_grouped_native(handle, groups, capacity=1 << 16)
    _assert_combined(got, members, flags, 6)


def test_capacity_protocol_with_the_drive_pass_in_front(handle):
    _upload(handle, 6)
    members = _members()
    flags = [True] * 4
    groups = [_traffic_group(slot, m, f) for (slot, m), f in zip(members, flags)]
    totals = [int(_traffic_reference(m, 6, True)[1]["set_offset"][-1]) for _, m in members]
    total = sum(totals)
    assert total > 0 and totals[-1] > 0
    _assert_combined(hdv.drive_traffic_grouped_native(handle, groups, capacity=total), members, flags, 6)
    with pytest.raises(backend.CapacityError) as e:
        hdv.drive_traffic_grouped_native(handle, groups, capacity=total - 1)
    assert e.value.count == total
    raw = {}
    got = hdv.drive_traffic_grouped_native(handle, groups, capacity=total - 1, raw=raw, guard=64)
    assert raw["rc"] == backend.ERR_CAPACITY
    assert raw["set_base"].tolist() == np.concatenate([[0], np.cumsum(totals)]).tolist()
    for (driven, traffic), (_, m) in zip(got, members):
        ref_d, ref_t = _traffic_reference(m, 6, True)
        D.assert_same(driven, ref_d, m.name)  # (the driver outputs are there whatever the room)
        assert np.array_equal(traffic["set_offset"], ref_t["set_offset"]) and traffic["closest"] == ref_t["closest"] and np.array_equal(traffic["adjacency"], ref_t["adjacency"])
    assert np.isnan(raw["set_x"][total - 1:]).all() and np.isnan(raw["set_y"][total - 1:]).all()


def test_the_four_calls_take_turns_on_one_workspace(handle):
    """pdmpc_hdv_traffic, pdmpc_hdv_traffic_grouped, pdmpc_hdv_drive_grouped and pdmpc_hdv_drive_traffic_grouped stage into and read back
    from ONE workspace on the handle, under layouts of one function (csrc/hdv_call_host.hpp: hdv_ws) with other regions empty in each.
    Ungrouped, grouped traffic, drive alone, drive and traffic, ungrouped again: each equals its host twin bit for bit, whatever the
    call before it left in the workspace.  The lab map at Hp 1, two groups of (2 HDVs, 1 CAV) and (1 HDV, no CAV)."""
    sets = H.local_sets(1)
    handle.upload_hdv_map(D.lab(), sets, slot=LAB)
    L, R = D.lab(), D.loop_route()
    members = [(LAB, D.Member("two HDVs, a CAV ahead", L, [(R, 0.7, ZERO, 0.5), (R, 1.6, ZERO, 0.5)], [D.at(L, R, 1.3) + (ZERO,)])),
               (LAB, D.Member("one HDV, no CAV", L, [(R, 3.0, ZERO, 0.5)], []))]
    standing = [_traffic_reference(m, 1, False)[1] for _, m in members]  # the traffic at the poses the groups bring

    def ungrouped(what):
        g = _traffic_group(LAB, members[0][1], False)
        cs = ([math.cos(a) for a in g["yaw"]], [math.sin(a) for a in g["yaw"]])
        dev = hdv.hdv_traffic_native(L, sets, g["x"], g["y"], g["yaw"], g["trim"], g["tiles"], g["cav_x"], g["cav_y"], g["cav_lanelet"], g["cav_tile"], handle=handle, cos_sin=cs)
        H.assert_same(dev, standing[0], what)

    ungrouped("ungrouped, first")
    plain = [_traffic_group(slot, m, False) for slot, m in members]
    got = handle.hdv_traffic_grouped([(g["slot"], g["x"], g["y"], g["yaw"], g["trim"], g["tiles"], g["cav_x"], g["cav_y"], g["cav_lanelet"], g["cav_tile"]) for g in plain],
                                     capacity=1 << 16)
    for g, (t, ref) in enumerate(zip(got, standing)):
        H.assert_same(t, ref, "grouped traffic, group %d" % g)
    _assert_members(hdv.drive_grouped_native(handle, [m.group(slot) for slot, m in members]), members)
    flags = [True, True]
    _assert_combined(hdv.drive_traffic_grouped_native(handle, [_traffic_group(slot, m, f) for (slot, m), f in zip(members, flags)], capacity=1 << 16), members, flags, 1)
    ungrouped("ungrouped, after the grouped calls")
    assert sum(len(t["row_hdv"]) for t in standing) > 0 and int(standing[0]["adjacency"].size) == 2


def test_refusals_leave_the_handle_working(handle):
    _upload(handle, 1)
    members = _members()
    good = [members[3]]

    def works():
        _assert_members(hdv.drive_grouped_native(handle, [m.group(slot) for slot, m in good]), good)

    def refused(groups, text, combined=False):
        with pytest.raises(backend.BackendError) as e:
            if combined:
                hdv.drive_traffic_grouped_native(handle, groups, capacity=1 << 16)
            else:
                hdv.drive_grouped_native(handle, groups)
        assert e.value.status == -1 and text in str(e.value), str(e.value)
        works()

    works()
    slot, m = members[3]
    g = m.group(slot)
    refused([members[0][1].group(HAND), dict(g, routes=[m.routes[0], ([1, 3, 10], False), m.routes[2]])], "group 1: HDV 1: route position 2: lanelet 10 is no successor of lanelet 3")
    refused([dict(g, states=[m.states[0], (0, 10000, 0.0), m.states[2]])], "group 0: HDV 1: a state that is not on its route")
    refused([dict(g, params=(2.0, 0.3, 0.1, 0.125))], "headway < dt")
    refused([dict(g, dt=0.0)], "positive")
    refused([dict(g, slot=7)], "no map was uploaded")
    refused([dict(g, v_des=[0.5, -1.0, 0.5])], "desired speed")
    t = _traffic_group(slot, m, True)
    refused([dict(t, routes=[m.routes[0], ([1, 3, 10], False), m.routes[2]])], "group 0: HDV 1: route position 2", combined=True)
    refused([dict(t, trim=[1, 10000, 1])], "trim out of range", combined=True)
    # a group that does not drive may bring anything for a route: it is not read
    hdv.drive_traffic_grouped_native(handle, [dict(_traffic_group(slot, m, False), routes=None)], capacity=1 << 16)
    works()
