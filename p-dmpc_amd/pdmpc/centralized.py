"""CentralizedController — the non-prioritized baseline (hlc/controller/centralized/CentralizedController.m).

One optimizer call per time step plans every vehicle at once: GraphSearch.run_optimizer with iter.amount = N, i.e. one graph
search over the joint state of all vehicles (pdmpc_plan_joint on the GPU).  There is no coupling graph and there are no
priorities (CentralizedController.m:26-32); the vehicles see the scenario's obstacles and keep clear of each other inside the
search.  An exhausted search is an error, as in the reference, which has no fallback for this controller (:63-69).

The traffic info and the plant update are those of the prioritized controller (HighLevelController.m:167-270,
Simulation.m:86-100); the planner is injected: `plan_joint(list[VehicleIter]) -> list[ControlResultsInfo]`, one per vehicle
(GraphSearchHip.run_optimizer_joint on the GPU).
"""
import dataclasses
from typing import Callable, List

from .config import Config
from .controller import Measurement, PrioritizedSequentialController
from .iteration_data import ControlResultsInfo, VehicleIter
from .mpa import get_mpa


class CentralizedExhaustedError(RuntimeError):
    pass


def centralized_options(options: Config) -> Config:
    """The options of a centralized run: is_prioritized = false, so the maneuver areas are convex and the separating-axis checker
    applies (Config.are_any_obstacles_non_convex, Config.m:71-87; systemtests.m:21)."""
    return dataclasses.replace(options, is_prioritized=False)


def centralized_mpa(options: Config):
    """The MPA built from the controller's own options (convex areas)."""
    return get_mpa(centralized_options(options))


class CentralizedController(PrioritizedSequentialController):
    hdvs_supported = False  # set_hdvs refuses: the joint kernel does not check HDV sets

    def __init__(
        self,
        options: Config,
        scenario,
        mpa,
        plan_joint: Callable[[List[VehicleIter]], List[ControlResultsInfo]],
        boundary_provider=None,
    ):
        options = centralized_options(options)
        super().__init__(options, scenario, mpa, None, coupling="none", boundary_provider=boundary_provider)
        self.plan_joint = plan_joint

    def build_iters(self) -> List[VehicleIter]:
        """The iteration data of all N vehicles (row v of the reference's iter): the traffic info, the scenario's obstacles."""
        self._traffic_info()
        obstacles = list(self.scenario.obstacles)
        dyn = [list(r) for r in self.scenario.dynamic_obstacle_area]
        return [
            VehicleIter(
                x0=self.x0[i].copy(),
                trim_index=int(self.trims[i]),
                reference_trajectory_points=self.ref_points[i],
                v_ref=self.v_ref[i],
                predicted_lanelet_boundary=self.boundary[i],
                obstacles=list(obstacles),
                dynamic_obstacle_area=list(dyn),
                amount=self.n,
            )
            for i in range(self.n)
        ]

    def step(self, plan_step=None):
        """One pass of HighLevelController.main_control_loop with CentralizedController.controller (:34-61)."""
        if plan_step is not None:
            raise ValueError("the centralized controller plans with its plan_joint callable")
        self.k += 1
        iters = self.build_iters()
        self.last_iters = iters
        infos = list(self.plan_joint(iters))
        if len(infos) != self.n:
            raise ValueError("plan_joint returned %d results for %d vehicles" % (len(infos), self.n))
        if any(info.is_exhausted for info in infos):
            raise CentralizedExhaustedError("graph search exhausted at time step %d: the centralized controller has no fallback" % self.k)
        self.infos = infos
        # Simulation.apply (Simulation.m:86-100)
        for i, info in enumerate(infos):
            t = self.mpa.trims[int(info.predicted_trims[0]) - 1]
            self.meas[i] = Measurement(float(info.y_predicted[0, 0]), float(info.y_predicted[1, 0]), float(info.y_predicted[2, 0]), t.speed, t.steering)
        self.info_old = list(infos)
        return infos
