"""HDVs that move themselves in closed loops on the MI355X (DESIGN.md §3.24 "Drivers"): the traffic stage makes ONE
pdmpc_hdv_drive_traffic_grouped per built step -- the drive launch in front of the five of the traffic call.  pdmpc_controller_run over 6
steps with drivers ends where six checked single steps end, whose records are the oracle's (the sampled reference's) on the controller's own
problems and whose driver state is the CPU run's; a sweep of four members -- two with drivers, one with a recording on a moved map, one
without HDVs -- ends byte for byte where its solo twins end, with one call per lock-step, on a handle and on a group of two logical ranks."""
import numpy as np
import pytest

import hdv_cases as H
import hdv_drive_cases as D
import sampled_step_reference as ref_step
from oracle import oracle
from pdmpc import backend, hdv
from pdmpc.backend import Group, Handle
from pdmpc.iteration_data import info_from_record
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeSweep
from test_gpu_hdv_controller import _native_twins
from test_gpu_hdv_sweep import MOVE, _close, _member, _options
from test_gpu_parity import assert_records_equal
from test_hdv_drive_controller import PARAMS, ROUTE, STARTS, V_DES, _same_driver_state
from test_native_controller import assert_same_problem

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]


def _cpu_run(options, steps):
    """the driver state after `steps` steps of the native controller without a handle, the oracle as the planner"""
    from test_hdv_drive_controller import _driven, _native_step

    _, nat = _driven(options)
    for _ in range(steps):
        _native_step(nat, options, get_mpa(options))
    out = nat.hdv_driver_state(), nat.state()
    nat.close()
    return out


def _driven_loop(options, handle, reference, optimizer="graph_search", steps=6):
    mpa = get_mpa(options)
    py, nat = _native_twins(options, handle, optimizer=optimizer)
    _, ran = _native_twins(options, handle, optimizer=optimizer)
    for c in (py, nat, ran):
        c.set_hdv_drivers([ROUTE, ROUTE], STARTS, V_DES, PARAMS)
    ran.run(steps)
    for step in range(1, steps + 1):
        recs = nat.step()
        q, info = nat.problem(), nat.hdv_info()

        def plan_step(prob):
            assert_same_problem(prob, q, "step %d" % step)
            for a, b in zip(prob["iters"], q["iters"]):
                assert [p.tobytes() for row in a.hdv_reachable_sets for p in row] == [np.ascontiguousarray(p).tobytes() for row in b.hdv_reachable_sets for p in row]
            ref = reference(prob, mpa, py)
            assert_records_equal(recs, ref, "native step %d" % step)
            return [info_from_record(ref[i], options.Hp) for i in range(len(ref))]

        py.step(plan_step=plan_step)
        H.assert_same({k: v for k, v in py.hdv_info.items()}, info, "traffic info of step %d" % step)
        _same_driver_state(py.hdv_driver_state(), nat.hdv_driver_state(), "step %d" % step)
    # pdmpc_controller_run ends where the six checked steps end
    _same_driver_state(ran.hdv_driver_state(), nat.hdv_driver_state(), "pdmpc_controller_run")
    a, b = ran.state(), nat.state()
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("x", "y", "yaw"))
    H.assert_same(ran.hdv_info(), nat.hdv_info(), "pdmpc_controller_run")
    assert max(nat.hdv_driver_state()["speed"]) > 0.0
    out = nat.hdv_driver_state(), nat.state()
    nat.close()
    ran.close()
    return out


def test_run_with_drivers_and_the_graph_search():
    from pdmpc.optimizer import GraphSearchHip

    options = H.loop_options(2, max_nodes=1 << 16, max_vehicles=32)
    opt = GraphSearchHip(options)
    opt._ensure_mpa(get_mpa(options))
    ds, st = _driven_loop(options, opt.handle, lambda prob, mpa, ctl: oracle.plan_step(options, mpa, prob)[0])
    cpu_ds, cpu_st = _cpu_run(H.loop_options(2, max_nodes=1 << 16), 6)
    _same_driver_state(ds, cpu_ds, "against the run without a handle")
    assert np.asarray(st["x"]).tobytes() == np.asarray(cpu_st["x"]).tobytes()
    opt.handle.close()


def test_run_with_drivers_and_the_sampled_optimizer():
    options = H.loop_options(2, max_vehicles=16)
    h = Handle(options)
    h.upload_mpa(get_mpa(options))
    _driven_loop(options, h, lambda prob, mpa, ctl: ref_step.plan_step_sampled(options, mpa, prob, ref_step.step_seeds(prob, ctl.k)), optimizer="sampled")
    h.close()


def _four(handle, with_hdvs, plain):
    """A and B on the lab map with drivers (B's HDVs start elsewhere and drive slower), C on the lab map moved by MOVE with a
    recording of hdv_poses_at, D without HDVs"""
    a, b, c, d = _member(with_hdvs, handle), _member(with_hdvs, handle), _member(with_hdvs, handle, MOVE), _member(plain, handle)
    a.set_hdv_drivers([ROUTE, ROUTE], STARTS, V_DES, PARAMS)
    b.set_hdv_drivers([ROUTE, ROUTE], [1.1, 3.3], [0.3, 0.5], (1.5, 0.35, 0.5, 0.125))
    rows = [H.hdv_poses_at(s) for s in range(1, 4)]
    c.set_hdv_recording([[v + MOVE[0] for v in r[0]] for r in rows], [[v + MOVE[1] for v in r[1]] for r in rows], [r[2] for r in rows])
    return [a, b, c, d]


def _sweep_against_solo_twins(sweep, swept, solo):
    together = sweep.run(3)
    assert sweep.last_hdv_calls() == (1, 0)  # the combined call counts as one; the maps were uploaded by the first lock-step
    for c in solo:
        c.run(3)
    for i in range(4):
        a, b = swept[i].state(), solo[i].state()
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("x", "y", "yaw")), i
        assert np.ascontiguousarray(swept[i].records()).tobytes() == np.ascontiguousarray(solo[i].records()).tobytes(), i
    for c in solo:
        c.explore_step(4)
    alone = [c.records() for c in solo]
    together = sweep.explore_step(4)
    assert sweep.last_hdv_calls() == (1, 0)
    for i in range(4):
        assert np.ascontiguousarray(together[i]).tobytes() == np.ascontiguousarray(alone[i]).tobytes(), i
        a, b = swept[i].state(), solo[i].state()
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("x", "y", "yaw")), i
    for i in range(3):
        H.assert_same(swept[i].hdv_info(), solo[i].hdv_info(), "traffic info of member %d" % i)
    for i in range(2):
        _same_driver_state(swept[i].hdv_driver_state(), solo[i].hdv_driver_state(), "member %d" % i)
        assert max(swept[i].hdv_driver_state()["speed"]) > 0.0
    assert swept[0].hdv_driver_state()["states"] != swept[1].hdv_driver_state()["states"]


def test_a_sweep_of_driven_recorded_and_plain_members_ends_where_its_solo_twins_end():
    with_hdvs, plain = _options()
    h, h2 = Handle(with_hdvs), Handle(with_hdvs)
    for x in (h, h2):
        x.upload_mpa(get_mpa(with_hdvs))
    swept, solo = _four(h, with_hdvs, plain), _four(h2, with_hdvs, plain)
    sweep = NativeSweep(swept, h)
    sweep.build()
    assert sweep.last_hdv_calls() == (1, 2)  # one call -- no member drives at its first built step --, two maps
    for c in solo:
        c.build_step()
    _sweep_against_solo_twins(sweep, swept, solo)
    _close(sweep, swept, solo, h, h2)


def test_the_same_sweep_on_a_group_of_two_logical_ranks():
    with_hdvs, plain = _options()
    g = Group(with_hdvs, n_devices=2, devices=[0, 0], collective=backend.COLLECTIVE_COPY)
    g.upload_mpa(get_mpa(with_hdvs))
    h2 = Handle(with_hdvs)
    h2.upload_mpa(get_mpa(with_hdvs))
    swept, solo = _four(g.rank0(), with_hdvs, plain), _four(h2, with_hdvs, plain)
    sweep = NativeSweep(swept, g.rank0())
    sweep.set_group(g, backend.SHARD_AUTO)
    _sweep_against_solo_twins(sweep, swept, solo)
    _close(sweep, swept, solo, h2, g)
