"""The HDV traffic stage of a sweep on the MI355X (csrc/step_controller.cpp: hdv_traffic_stage): the members with
HDVs are the groups of ONE pdmpc_hdv_traffic_grouped per lock-step, members on equal maps share a map slot of the handle, and a map
that is resident is not uploaded again -- while every member's records and traffic info stay byte for byte those of a twin that steps
alone (on a handle of its own, so that the twins' uploads do not make the sweep's maps resident)."""
import copy

import numpy as np
import pytest

import hdv_cases as H
from pdmpc import backend, hdv
from pdmpc.backend import Group, Handle
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeController, NativeSweep
from pdmpc.road_network import commonroad_scenario
from test_native_controller import assert_same_problem

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

MOVE = (10.0, 0.0)


def _hdv_mpa(Hp):
    from pdmpc.config import Config, MpaType, ScenarioType

    return get_mpa(Config(scenario_type=ScenarioType.commonroad, amount=1, Hp=Hp, mpa_type=MpaType.single_speed, recursive_feasibility=False))


def _scenario(options, move=(0.0, 0.0)):
    """the four-CAV loop on the lab map, every coordinate of the map and of the vehicles moved by `move`: another map for the handle"""
    sc = commonroad_scenario(options, seed=1)
    d = np.array(move)
    if d.any():
        sc.lanelet_boundary = [(np.asarray(b[0]) + d, np.asarray(b[1]) + d) for b in sc.lanelet_boundary]
        for v in sc.vehicles:
            v.reference_path = v.reference_path + d
            v.x_start += float(d[0])
            v.y_start += float(d[1])
    return sc


def _member(options, handle, move=(0.0, 0.0)):
    sc = _scenario(options, move)
    nat = NativeController(options, sc, get_mpa(options), handle, coupling="distance")
    nat.move = move
    if options.manual_control:
        hmap = hdv.scenario_hdv_map(sc)
        nat.set_hdvs(_hdv_mpa(options.Hp), hmap.successors, hmap.relationship)
    return nat


def _four(handle, with_hdvs, plain):
    """A and B with HDVs on the lab map, C with HDVs on the lab map moved by MOVE, D without HDVs"""
    return [_member(with_hdvs, handle), _member(with_hdvs, handle), _member(with_hdvs, handle, MOVE), _member(plain, handle)]


def _measure(members, step):
    """the HDVs of the test at time step `step`; B's are a step ahead of A's, C's stand on its moved map"""
    for i, c in enumerate(members[:3]):
        x, y, yaw = H.hdv_poses_at(step + (i == 1))
        c.set_hdv_measurements([v + c.move[0] for v in x], [v + c.move[1] for v in y], yaw)


def _options():
    with_hdvs = H.loop_options(2, max_nodes=1 << 16, max_vehicles=64)
    plain = H.loop_options(0, max_nodes=1 << 16, max_vehicles=64)
    return with_hdvs, plain


def _lock_steps(sweep, swept, solo, first=1, steps=3, uploads_first=2):
    for step in range(first, first + steps):
        _measure(solo, step)
        _measure(swept, step)
        alone = [c.step() for c in solo]
        together = sweep.step()
        for i in range(4):
            assert together[i].tobytes() == alone[i].tobytes(), (step, i)
        for i in range(3):
            H.assert_same(swept[i].hdv_info(), solo[i].hdv_info(), "traffic info of member %d at step %d" % (i, step))
        assert sweep.last_hdv_calls() == (1, uploads_first if step == first else 0), step


def _close(*things):
    for t in things:
        for c in t if isinstance(t, list) else [t]:
            c.close()


def test_four_members_make_one_call_and_upload_two_maps_once():
    with_hdvs, plain = _options()
    h, h2 = Handle(with_hdvs), Handle(with_hdvs)
    for x in (h, h2):
        x.upload_mpa(get_mpa(with_hdvs))
    swept, solo = _four(h, with_hdvs, plain), _four(h2, with_hdvs, plain)
    sweep = NativeSweep(swept, h)
    assert h.hdv_map_slot_state(0) == (0, 0)  # (setting the HDVs uploads nothing)
    _lock_steps(sweep, swept, solo)
    # A and B share slot 0, C has slot 1; nothing else was uploaded in three lock-steps
    assert h.hdv_map_slot_state(0)[0] > 0 and h.hdv_map_slot_state(1)[0] > h.hdv_map_slot_state(0)[0] and h.hdv_map_slot_state(2) == (0, 2)
    # one explorative lock-step of 4 prioritizations: the same stage
    _measure(solo, 4)
    _measure(swept, 4)
    for c in solo:
        c.explore_step(4)
    alone = [c.records() for c in solo]  # the kept (chosen) records, as the sweep returns them
    together = sweep.explore_step(4)
    for i in range(4):
        assert np.ascontiguousarray(together[i]).tobytes() == np.ascontiguousarray(alone[i]).tobytes(), i
    for i in range(3):
        H.assert_same(swept[i].hdv_info(), solo[i].hdv_info(), "traffic info of member %d in the explorative step" % i)
    assert sweep.last_hdv_calls() == (1, 0) and h.hdv_map_slot_state(0)[1] == 2
    _close(sweep, swept, solo, h, h2)


def test_on_a_group_of_two_logical_ranks():
    """the grouped call runs on rank 0's handle; the lock-steps are planned over the group"""
    with_hdvs, plain = _options()
    g = Group(with_hdvs, n_devices=2, devices=[0, 0], collective=backend.COLLECTIVE_COPY)
    g.upload_mpa(get_mpa(with_hdvs))
    h2 = Handle(with_hdvs)
    h2.upload_mpa(get_mpa(with_hdvs))
    swept, solo = _four(g.rank0(), with_hdvs, plain), _four(h2, with_hdvs, plain)
    sweep = NativeSweep(swept, g.rank0())
    sweep.set_group(g, backend.SHARD_AUTO)
    _lock_steps(sweep, swept, solo)
    _close(sweep, swept, solo, h2, g)


def test_two_controllers_that_take_turns_on_one_handle_upload_once_each():
    """solo controllers are sweeps of one: each finds its map where it left it, so after their first steps no step uploads anything --
    read off the handle's upload counter and the slots' generations"""
    with_hdvs, _ = _options()
    h = Handle(with_hdvs)
    h.upload_mpa(get_mpa(with_hdvs))
    a, b, same_as_a = _member(with_hdvs, h), _member(with_hdvs, h, MOVE), _member(with_hdvs, h)
    first = None
    for step in range(1, 4):
        for c in (a, b, same_as_a):
            x, y, yaw = H.hdv_poses_at(step)
            c.set_hdv_measurements([v + c.move[0] for v in x], [v + c.move[1] for v in y], yaw)
            c.step()
        state = [h.hdv_map_slot_state(s) for s in range(3)]
        assert state[0][1] == 2 and state[2][0] == 0, (step, state)  # two uploads in all: a's map (which same_as_a finds) and b's
        first = first or state
        assert state == first, step  # the generations have not moved
    H.assert_same(a.hdv_info(), same_as_a.hdv_info(), "two controllers on one map")
    _close([a, b, same_as_a], h)


def test_nine_members_on_nine_maps_build_in_two_calls():
    """PDMPC_HDV_MAP_SLOTS distinct maps fit one call: the ninth member makes a second one.  Build only (no search is launched); the
    problems are the ones the members build alone."""
    with_hdvs = copy.copy(H.loop_options(2, max_nodes=1 << 16, max_vehicles=64))
    h, h2 = Handle(with_hdvs), Handle(with_hdvs)
    for x in (h, h2):
        x.upload_mpa(get_mpa(with_hdvs))
    moves = [(10.0 * i, 0.0) for i in range(9)]
    swept, solo = [_member(with_hdvs, h, m) for m in moves], [_member(with_hdvs, h2, m) for m in moves]
    for c in swept + solo:
        x, y, yaw = H.hdv_poses_at(1)
        c.set_hdv_measurements([v + c.move[0] for v in x], [v + c.move[1] for v in y], yaw)
    sweep = NativeSweep(swept, h)
    sweep.build()
    assert sweep.last_hdv_calls() == (2, 9)
    for i, (a, b) in enumerate(zip(swept, solo)):
        b.build_step()
        H.assert_same(a.hdv_info(), b.hdv_info(), "member %d" % i)
        pa, pb = a.problem(), b.problem()
        assert_same_problem(pa, pb, "member %d" % i)
        for ia, ib in zip(pa["iters"], pb["iters"]):
            assert [np.ascontiguousarray(p).tobytes() for row in ia.hdv_reachable_sets for p in row] == [np.ascontiguousarray(p).tobytes() for row in ib.hdv_reachable_sets for p in row]
    sweep.build()
    # nine maps and eight slots: the second batch's map took the last slot from the eighth member's, so each build the first batch
    # uploads that one again and the second batch its own -- two uploads, the fewest there can be -- while slots 0 .. 6 never move
    before = [h.hdv_map_slot_state(s)[0] for s in range(7)]
    sweep.build()
    assert sweep.last_hdv_calls() == (2, 2) and [h.hdv_map_slot_state(s)[0] for s in range(7)] == before
    _close(sweep, swept, solo, h, h2)
