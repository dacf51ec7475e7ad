"""The ctypes prototype of every function of include/pdmpc.h: name -> (restype, [argtypes]), in the header's order and groups.

The one place a prototype is written down.  `declare` applies the table to a loaded library (backend.load_library) and
tests/test_abi.py checks it against the header, argument by argument.  Opaque objects (pdmpc_handle*, pdmpc_group*,
pdmpc_controller*, pdmpc_sweep*) are void pointers, every struct the header defines is its twin of pdmpc.abi.
"""
import ctypes as C

from . import abi

P = C.POINTER
INT, STR = C.c_int, C.c_char_p
OBJ = C.c_void_p  # an opaque object of the library; P(OBJ) where a call returns one or takes a list of them
VOIDP = C.c_void_p  # device memory, a stream
I32, I64, U32, F64 = C.c_int32, C.c_int64, C.c_uint32, C.c_double
DP, IP, BP, UP = abi.c_double_p, abi.c_int32_p, abi.c_uint8_p, abi.c_uint32_p
CONFIG, MPA, POLYS, VIN, VOUT, CHOICE = P(abi.Config), P(abi.Mpa), P(abi.PolygonSet), P(abi.VehicleIn), P(abi.VehicleOut), P(abi.ChoiceStruct)

STEP = [I32, VIN, IP, IP, POLYS]  # n_vehicles, in, pred_offset, pred_index, fallback_shapes
STEP_OUT = [P(I32), P(VIN), P(IP), P(IP), P(POLYS)]  # ... of a built problem, read back
POSES = [DP, DP, DP, DP, IP]  # x, y, cos_yaw, sin_yaw, trim
TABLE = [I32, I32, POLYS]  # n_trims, Hp, local_sets
COUPLED = [BP, DP]  # adjacency, area
BOUND = POSES + [POLYS, I32, I32, IP, DP, DP, BP]  # ..., lanelet_polygons, all_steps, capacity, offset, out_x, out_y, flags
FCA = [I32, I32, DP, DP, DP, DP, I32, IP, POLYS, POLYS, F64, F64, F64, IP, IP]
FCA_GROUPED = [I32, P(abi.FcaGroup), I32, DP, DP, DP, DP, IP, IP]
CHOSEN = [CHOICE, IP, DP]  # choice, chosen, cell_cost
HDV_MAP = [I32, IP, IP, DP, DP, DP, DP, IP, IP, BP] + TABLE  # n_lanelets, left/right offsets, left/right x y, successors, relationship, local sets
HDV_CALL = [I32, DP, DP, DP, DP, IP, DP, DP, I32, DP, DP, IP, DP, DP, IP, IP, I32, IP, IP, IP, DP, DP, BP, BP]
# n_groups, group_slot, hdv_offset, cav_offset | the HDVs | the CAVs | closest_offset, closest_index, capacity, n_rows, row_hdv, set_offset, set_base, set_x, set_y, set_flags, adjacency
HDV_GROUPED = [I32, IP, IP, IP] + [DP, DP, DP, DP, IP, DP, DP] + [DP, DP, IP, DP, DP] + [IP, IP, I32, IP, IP, IP, IP, DP, DP, BP, BP]
HDV_ROAD = HDV_MAP[:10]  # the map without the local sets
HDV_ROUTES = [I32, IP, IP, BP]  # n_hdv, route_offset, route_lanelet, closed
HDV_DRIVEN = [IP, DP, DP, DP, DP, DP, DP, DP]  # new_seg, new_u, x, y, cos_yaw, sin_yaw, speed, gap
UNIQUE = [I32, BP, I64, P(I64), UP, IP]
UNIQUE_GROUPED = [I32, IP, P(BP), P(I64), P(I64), UP, IP]  # n_groups, group_n, adjacency, max_out, n_out, masks, priorities

PROTOTYPES = {
    # ---- life cycle
    "pdmpc_create": (INT, [CONFIG, P(OBJ)]),
    "pdmpc_destroy": (INT, [OBJ]),
    "pdmpc_launch_plan_host": (INT, [STR, P(abi.LaunchQuery), P(abi.LaunchPlan)]),
    "pdmpc_get_config": (INT, [OBJ, CONFIG, P(I32)]),
    "pdmpc_upload_mpa": (INT, [OBJ, MPA]),
    "pdmpc_mpa_reach_host": (INT, [MPA, DP, DP]),
    "pdmpc_reach_lists_host": (INT, [I32, F64, F64, F64, F64, DP, DP, IP, IP, IP, IP]),
    "pdmpc_mpa_reach_rects_host": (INT, [MPA, I32, DP]),
    "pdmpc_reach_lists_oriented_host": (INT, [I32, I32, DP, I32, F64, F64, F64, DP, DP, IP, IP, IP, IP]),
    "pdmpc_plan_batch": (INT, [OBJ, I32, VIN, VOUT]),
    "pdmpc_set_arena_limit": (INT, [OBJ, I32]),
    "pdmpc_grow_arena": (INT, [OBJ, I32]),
    "pdmpc_arena_nodes": (INT, [OBJ, P(I32), P(I64)]),
    "pdmpc_plan_step": (INT, [OBJ] + STEP + [VOUT]),
    "pdmpc_plan_step_literal": (INT, [OBJ] + STEP + [VOUT]),
    # ---- device-resident path
    "pdmpc_pack_batch": (INT, [OBJ, I32, VIN]),
    "pdmpc_plan_step_lean": (INT, [OBJ] + STEP + [IP, DP]),
    "pdmpc_fetch_records_at": (INT, [OBJ, I32, IP, VOUT]),
    # ---- the choice among the plans of a batch
    "pdmpc_choose_host": (INT, [I32, IP, DP] + CHOSEN),
    "pdmpc_choose_resident": (INT, [OBJ, I32] + CHOSEN + [VOUT]),
    "pdmpc_plan_step_chosen": (INT, [OBJ] + STEP + CHOSEN + [VOUT]),
    "pdmpc_choice_kernel_ms": (INT, [OBJ, DP]),
    "pdmpc_last_call_timing": (INT, [OBJ, DP]),
    "pdmpc_launch_packed": (INT, [OBJ]),
    "pdmpc_launch_range": (INT, [OBJ, I32, I32]),
    "pdmpc_fetch_results": (INT, [OBJ, I32, VOUT]),
    "pdmpc_synchronize": (INT, [OBJ]),
    "pdmpc_set_safe_launch": (INT, [OBJ, I32]),
    "pdmpc_set_device_share": (INT, [OBJ, I32]),
    "pdmpc_begin_step": (INT, [OBJ]),
    "pdmpc_select_bank": (INT, [OBJ, I32]),
    "pdmpc_reset_stats": (INT, [OBJ]),
    # ---- step-level planning
    "pdmpc_set_step_weights": (INT, [OBJ, I32, DP]),
    "pdmpc_pack_step": (INT, [OBJ] + STEP),
    "pdmpc_result_device_buffer": (INT, [OBJ, P(VOIDP), P(C.c_size_t)]),
    "pdmpc_import_results": (INT, [OBJ, I32, I32, VOIDP]),
    "pdmpc_export_results": (INT, [OBJ, I32, I32, VOIDP]),
    "pdmpc_export_results_async": (INT, [OBJ, I32, I32, VOIDP]),
    "pdmpc_stream": (INT, [OBJ, P(VOIDP)]),
    "pdmpc_get_last_stats": (INT, [OBJ, P(abi.Stats)]),
    # ---- debug / parity instrumentation
    "pdmpc_debug_pop_trace": (INT, [OBJ, I32, I32, IP, IP]),
    "pdmpc_debug_tree": (INT, [OBJ, I32, I32] + [DP] * 5 + [IP] * 4),
    "pdmpc_debug_edge_check": (INT, [OBJ, I32, I32, IP, DP, DP, IP, DP, DP, IP]),
    "pdmpc_debug_interx_soups": (INT, [OBJ, I32, IP, DP, DP, DP, DP, IP, DP, DP, IP]),
    "pdmpc_debug_sincos": (INT, [OBJ, I32, DP, DP, DP]),
    "pdmpc_debug_raw_tree": (INT, [OBJ, I32, I32] + [DP] * 5 + [IP] * 3 + [DP, BP, IP]),
    "pdmpc_debug_counters": (INT, [OBJ, P(C.c_uint64)]),
    "pdmpc_debug_packed_offsets": (INT, [OBJ, I32, IP, IP, IP]),
    "pdmpc_debug_progress": (INT, [OBJ, I32, UP]),
    "pdmpc_debug_heap_script": (INT, [OBJ, I32, IP, IP, DP, I32, IP, IP, DP, DP]),
    # ---- the sampled optimizer
    "pdmpc_plan_batch_sampled": (INT, [OBJ, I32, VIN, UP, VOUT]),
    "pdmpc_plan_step_sampled": (INT, [OBJ] + STEP + [UP, VOUT]),
    "pdmpc_set_step_seeds": (INT, [OBJ, I32, UP]),
    "pdmpc_debug_random_numbers": (INT, [OBJ, I32, UP, I32, DP]),
    "pdmpc_set_sampled_budget": (INT, [OBJ, I32]),
    "pdmpc_get_sampled_budget": (INT, [OBJ, IP]),
    "pdmpc_last_sampled_kernel": (STR, [OBJ]),
    "pdmpc_sampled_plan_host": (INT, [STR, P(abi.LaunchQuery), I32, P(abi.LaunchPlan), P(I64)]),
    "pdmpc_sampled_plan_bank": (INT, [OBJ, I32, P(abi.LaunchPlan), P(I64)]),
    "pdmpc_debug_random_stream": (INT, [OBJ, I32, UP, I32, DP]),
    "pdmpc_set_sampled_ensemble": (INT, [OBJ, I32]),
    "pdmpc_get_sampled_ensemble": (INT, [OBJ, IP]),
    "pdmpc_sampled_member_seed": (U32, [U32, I32]),
    "pdmpc_sampled_ensemble_result": (INT, [OBJ, I32, IP, IP, DP]),
    "pdmpc_sampled_ensemble_plan_host": (INT, [STR, P(abi.LaunchQuery), I32, I32, P(abi.LaunchPlan), P(I64)]),
    # ---- centralized control
    "pdmpc_plan_joint": (INT, [OBJ, I32, IP, VIN, VOUT]),
    # ---- the unique prioritizations of a coupling graph
    "pdmpc_unique_priorities": (INT, [OBJ] + UNIQUE),
    "pdmpc_unique_priorities_host": (INT, UNIQUE),
    "pdmpc_unique_priorities_grouped": (INT, [OBJ] + UNIQUE_GROUPED),
    "pdmpc_unique_priorities_grouped_host": (INT, UNIQUE_GROUPED),
    # ---- reachable sets
    "pdmpc_local_reachable_sets": (INT, [MPA, I32, IP, DP, DP]),
    "pdmpc_upload_reachable_sets": (INT, [OBJ] + TABLE),
    "pdmpc_reachable_set_coupling": (INT, [OBJ, I32] + POSES + COUPLED),
    "pdmpc_reachable_set_coupling_host": (INT, TABLE + [I32] + POSES + COUPLED),
    "pdmpc_reachable_set_coupling_kernel_ms": (INT, [OBJ, DP]),
    "pdmpc_bound_reachable_sets": (INT, [OBJ, I32] + BOUND),
    "pdmpc_bound_reachable_sets_host": (INT, TABLE + [I32] + BOUND),
    "pdmpc_bounded_set_coupling": (INT, [OBJ] + COUPLED),
    "pdmpc_polygon_set_coupling_host": (INT, [POLYS, I32] + COUPLED),
    "pdmpc_bounded_reachable_kernel_ms": (INT, [OBJ, DP]),
    "pdmpc_reachable_set_coupling_grouped": (INT, [OBJ, I32, IP] + POSES + COUPLED),
    "pdmpc_bounded_set_coupling_grouped": (INT, [OBJ, I32, IP] + COUPLED),
    "pdmpc_reachable_set_coupling_grouped_host": (INT, TABLE + [I32, IP] + POSES + COUPLED),
    "pdmpc_polygon_set_coupling_grouped_host": (INT, [POLYS, I32, IP] + COUPLED),
    # ---- future collision assessment
    "pdmpc_fca_collisions": (INT, [OBJ] + FCA),
    "pdmpc_fca_collisions_host": (INT, FCA),
    "pdmpc_fca_kernel_ms": (INT, [OBJ, DP]),
    "pdmpc_fca_collisions_grouped": (INT, [OBJ] + FCA_GROUPED),
    "pdmpc_fca_collisions_grouped_host": (INT, FCA_GROUPED),
    # ---- human-driven vehicles
    "pdmpc_upload_hdv_map": (INT, [OBJ] + HDV_MAP),
    "pdmpc_hdv_traffic": (INT, [OBJ] + HDV_CALL),
    "pdmpc_hdv_traffic_host": (INT, HDV_MAP + HDV_CALL),
    "pdmpc_hdv_lanelet_distances_host": (INT, [I32, IP, IP, DP, DP, DP, DP, F64, F64, DP]),
    "pdmpc_hdv_kernel_ms": (INT, [OBJ, DP]),
    "pdmpc_upload_hdv_map_slot": (INT, [OBJ, I32] + HDV_MAP),
    "pdmpc_hdv_map_slot_state": (INT, [OBJ, I32, P(I64), P(I64), IP]),
    "pdmpc_hdv_map_slot_holds": (INT, [OBJ, I32] + HDV_MAP + [IP]),
    "pdmpc_hdv_check_map_host": (INT, HDV_MAP),
    "pdmpc_hdv_grouped_layout_host": (INT, [I32, IP, IP, I32, IP, IP, IP, IP, P(I64)]),
    "pdmpc_hdv_traffic_grouped": (INT, [OBJ] + HDV_GROUPED),
    "pdmpc_hdv_route_check_host": (INT, HDV_ROAD + HDV_ROUTES),
    "pdmpc_hdv_place_host": (INT, HDV_ROAD + HDV_ROUTES + [DP, DP, DP, IP, DP, DP, DP, DP, DP]),
    # ... state_seg, state_u, tile_dx, tile_dy, v_des | n_cav, the CAVs | parameters, dt
    "pdmpc_hdv_drive_host": (INT, HDV_ROAD + HDV_ROUTES + [IP, DP, DP, DP, DP] + [I32, DP, DP, DP, DP] + [DP, F64] + HDV_DRIVEN),
    "pdmpc_hdv_drive_grouped": (INT, [OBJ, I32, IP, IP, IP] + HDV_ROUTES[1:] + [IP, DP, DP, DP, DP] + [DP, DP, DP, DP] + [DP, DP] + HDV_DRIVEN),
    # n_groups, group_slot, hdv_offset, cav_offset, drives | routes | state_seg, state_u, v_des, parameters, dt | new_seg, new_u, speed, gap | the grouped traffic call
    "pdmpc_hdv_drive_traffic_grouped": (INT, [OBJ, I32, IP, IP, IP, BP] + HDV_ROUTES[1:] + [IP, DP, DP, DP, DP] + [IP, DP, DP, DP] + HDV_GROUPED[4:]),
    # ---- the caller's side of the boundary, natively
    "pdmpc_controller_create": (INT, [OBJ, P(abi.ControllerConfig), P(abi.ScenarioStruct), P(OBJ)]),
    "pdmpc_controller_destroy": (INT, [OBJ]),
    "pdmpc_controller_step": (INT, [OBJ]),
    "pdmpc_controller_set_hdvs": (INT, [OBJ, I32, MPA, IP, IP, BP, DP, DP]),
    "pdmpc_controller_set_hdv_measurements": (INT, [OBJ, DP, DP, DP]),
    "pdmpc_controller_set_hdv_drivers": (INT, [OBJ, IP, IP, BP, DP, DP, DP]),
    "pdmpc_controller_hdv_driver_state": (INT, [OBJ, IP, DP, DP, DP, DP, DP, DP]),
    "pdmpc_controller_set_hdv_recording": (INT, [OBJ, I32, DP, DP, DP]),
    "pdmpc_controller_set_hdv_poses": (INT, [OBJ, DP, DP, DP, DP]),
    "pdmpc_controller_hdv_info": (INT, [OBJ, IP, P(IP), P(IP), IP, P(IP), P(IP), P(DP), P(DP), P(BP), P(BP)]),
    "pdmpc_controller_run": (INT, [OBJ, I32, DP]),
    "pdmpc_controller_build_step": (INT, [OBJ]),
    "pdmpc_controller_apply": (INT, [OBJ, VOUT]),
    "pdmpc_controller_problem": (INT, [OBJ] + STEP_OUT + [P(IP), P(IP)]),
    "pdmpc_controller_state": (INT, [OBJ] + [DP] * 5 + [IP, P(I32)]),
    "pdmpc_controller_records": (VOUT, [OBJ]),
    "pdmpc_exploration_permutations": (INT, [I32, I32, U32, IP]),
    "pdmpc_controller_explore_build": (INT, [OBJ, I32, U32]),
    "pdmpc_controller_explore_problem": (INT, [OBJ] + STEP_OUT + [P(IP)] * 3),
    "pdmpc_controller_explore_choose": (INT, [OBJ, VOUT, IP, P(I32), DP]),
    "pdmpc_controller_explore_step": (INT, [OBJ, I32]),
    "pdmpc_controller_explore_run": (INT, [OBJ, I32, I32, DP]),
    "pdmpc_controller_explore_follow_own": (INT, [OBJ, I32]),
    "pdmpc_controller_explore_result": (INT, [OBJ, IP, P(I32), P(DP), P(VOUT)]),
    "pdmpc_controller_optimal_build": (INT, [OBJ, I32]),
    "pdmpc_controller_optimal_choose": (INT, [OBJ, VOUT, IP, DP]),
    "pdmpc_controller_optimal_step": (INT, [OBJ, I32]),
    "pdmpc_controller_optimal_run": (INT, [OBJ, I32, I32, DP]),
    "pdmpc_controller_optimal_result": (INT, [OBJ, IP, P(I32), P(DP), P(VOUT)]),
    "pdmpc_controller_last_timing": (INT, [OBJ, DP]),
    "pdmpc_controller_timing_sum": (INT, [OBJ, DP, P(I64), I32]),
    "pdmpc_controller_last_error": (STR, []),
    "pdmpc_controller_set_reachability": (INT, [OBJ, MPA]),
    "pdmpc_controller_set_parallel_coupling": (INT, [OBJ, I32]),
    "pdmpc_controller_set_lanelet_bounding": (INT, [OBJ, I32]),
    "pdmpc_controller_set_optimizer": (INT, [OBJ, I32]),
    "pdmpc_controller_seeds": (INT, [OBJ, P(I32), P(UP)]),
    "pdmpc_controller_priorities": (INT, [OBJ, P(I32), P(IP), P(I32), P(IP)]),
    "pdmpc_controller_set_device_choice": (INT, [OBJ, I32]),
    "pdmpc_controller_centralized_build": (INT, [OBJ]),
    "pdmpc_controller_centralized_problem": (INT, [OBJ, P(I32), P(VIN)]),
    "pdmpc_controller_centralized_apply": (INT, [OBJ, VOUT]),
    "pdmpc_controller_centralized_step": (INT, [OBJ]),
    "pdmpc_controller_centralized_run": (INT, [OBJ, I32, DP]),
    # ---- several closed loops in lock-step
    "pdmpc_sweep_create": (INT, [OBJ, I32, P(OBJ), P(OBJ)]),
    "pdmpc_sweep_destroy": (INT, [OBJ]),
    "pdmpc_sweep_build": (INT, [OBJ]),
    "pdmpc_sweep_problem": (INT, [OBJ] + STEP_OUT + [P(IP), P(IP)]),
    "pdmpc_sweep_apply": (INT, [OBJ, VOUT]),
    "pdmpc_sweep_step": (INT, [OBJ]),
    "pdmpc_sweep_run": (INT, [OBJ, I32, DP]),
    "pdmpc_sweep_last_timing": (INT, [OBJ, DP]),
    "pdmpc_sweep_last_prep_calls": (INT, [OBJ, IP]),
    "pdmpc_sweep_last_hdv_calls": (INT, [OBJ, IP]),
    "pdmpc_sweep_explore_build": (INT, [OBJ, I32]),
    "pdmpc_sweep_explore_problem": (INT, [OBJ] + STEP_OUT + [P(IP)] * 4),
    "pdmpc_sweep_explore_apply": (INT, [OBJ, VOUT]),
    "pdmpc_sweep_explore_step": (INT, [OBJ, I32]),
    "pdmpc_sweep_explore_run": (INT, [OBJ, I32, I32, DP]),
    "pdmpc_sweep_optimal_build": (INT, [OBJ, I32]),
    "pdmpc_sweep_optimal_problem": (INT, [OBJ] + STEP_OUT + [P(IP)] * 4),
    "pdmpc_sweep_optimal_apply": (INT, [OBJ, VOUT]),
    "pdmpc_sweep_optimal_step": (INT, [OBJ, I32]),
    "pdmpc_sweep_optimal_run": (INT, [OBJ, I32, I32, DP]),
    "pdmpc_sweep_optimal_last_calls": (INT, [OBJ, IP]),
    "pdmpc_sweep_centralized_build": (INT, [OBJ]),
    "pdmpc_sweep_centralized_problem": (INT, [OBJ, P(I32), P(IP), P(VIN), P(IP)]),
    "pdmpc_sweep_centralized_apply": (INT, [OBJ, VOUT]),
    "pdmpc_sweep_centralized_step": (INT, [OBJ]),
    "pdmpc_sweep_centralized_run": (INT, [OBJ, I32, DP]),
    "pdmpc_sweep_centralized_status": (INT, [OBJ, IP]),
    # ---- several GPUs behind the same boundary
    "pdmpc_group_create": (INT, [CONFIG, I32, IP, P(OBJ)]),
    "pdmpc_group_create_ex": (INT, [CONFIG, I32, IP, I32, P(OBJ)]),
    "pdmpc_group_collective": (INT, [OBJ, P(I32)]),
    "pdmpc_group_destroy": (INT, [OBJ]),
    "pdmpc_group_size": (INT, [OBJ, P(I32)]),
    "pdmpc_group_handle": (INT, [OBJ, I32, P(OBJ)]),
    "pdmpc_group_grow_arena": (INT, [OBJ, I32]),
    "pdmpc_group_upload_mpa": (INT, [OBJ, MPA]),
    "pdmpc_group_plan_step": (INT, [OBJ] + STEP + [DP, I32, VOUT]),
    "pdmpc_group_pack_step": (INT, [OBJ, I32] + STEP + [DP, I32]),
    "pdmpc_group_launch": (INT, [OBJ, I32]),
    "pdmpc_group_fetch": (INT, [OBJ, I32, I32, VOUT]),
    "pdmpc_group_partition": (INT, [I32, IP, IP, DP, I32, I32, IP, IP, IP]),
    "pdmpc_group_last_timing": (INT, [OBJ, DP]),
    # ---- the sampled optimizer, the lean read-back and the choice on a group
    "pdmpc_group_set_step_seeds": (INT, [OBJ, I32, UP]),
    "pdmpc_group_set_sampled_budget": (INT, [OBJ, I32]),
    "pdmpc_group_set_sampled_ensemble": (INT, [OBJ, I32]),
    "pdmpc_group_plan_step_lean": (INT, [OBJ] + STEP + [DP, I32, IP, DP]),
    "pdmpc_group_fetch_records_at": (INT, [OBJ, I32, IP, VOUT]),
    "pdmpc_group_plan_step_chosen": (INT, [OBJ] + STEP + [DP, I32] + CHOSEN + [VOUT]),
    "pdmpc_group_choose_resident": (INT, [OBJ, I32, I32] + CHOSEN + [VOUT]),
    "pdmpc_group_debug_choose": (INT, [OBJ, I32, VOUT, IP] + CHOSEN + [VOUT]),
    "pdmpc_group_last_exchange": (INT, [OBJ, P(I64)]),
    "pdmpc_group_route_host": (INT, [I32, IP, IP, DP, I32, I32, IP, IP]),
    "pdmpc_controller_set_group": (INT, [OBJ, OBJ, I32]),
    "pdmpc_sweep_set_group": (INT, [OBJ, OBJ, I32]),
    "pdmpc_last_error": (STR, []),
    "pdmpc_version": (STR, []),
}


def declare(L):
    """Give every function of the table its prototype on the loaded library L."""
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L
