"""The verification of an arrival from the lists of collision-free and parked nodes (bulk_search.hpp, BK_VLIST / BK_PLIST): the
benchmarked windows, whose heavy searches meet several arrival events each and re-check thousands of nodes per event, against the
oracle every step — with the kernel built for two workgroups per CU, and with every search ending on the replay (which wants
final verdicts: everything the lists held has been re-checked by then)."""
import os

import pytest

from pdmpc.config import Config, ScenarioType

from test_gpu_step import run_closed_loop

pytestmark = pytest.mark.gpu


def c2_window(n_steps):
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=32, max_nodes=1 << 17)
    sc = commonroad_scenario(options, seed=1)
    return run_closed_loop(options, sc, "distance", boundary_provider(sc), n_steps, oracle_threads=os.cpu_count() or 1).handle_stats


@pytest.mark.parametrize("tuning", ["compact=1", "compact=1,force_tie=1", "force_tie=1,share_min=64,tile=32"])
def test_c2_window_with_arrival_events(tuning, monkeypatch):
    monkeypatch.setenv("PDMPC_TUNING", tuning)
    stats = c2_window(30)
    assert stats["kernel"] == 2


def test_c3_window_with_arrival_events(monkeypatch):
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    monkeypatch.setenv("PDMPC_TUNING", "force_tie=1")
    options = Config(scenario_type=ScenarioType.commonroad, amount=128, Hp=8, max_num_CLs=2, max_vehicles=128, max_nodes=1 << 16)
    sc = commonroad_scenario(options, seed=1, tiles=7)
    ctl = run_closed_loop(options, sc, "distance", boundary_provider(sc), 12, oracle_threads=os.cpu_count() or 1, priority_strategy="coloring")
    assert int(ctl.last_levels.max()) == 2
