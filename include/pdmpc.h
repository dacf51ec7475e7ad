/* pdmpc.h — C ABI of libpdmpc_hip.so: the MI355X (gfx950) backend for p-dmpc's
 * per-vehicle graph-search trajectory optimizer.
 *
 * Drop-in boundary.  The reference selects its optimizer in
 * hlc/optimizer/OptimizerInterface.m:19-34 (`get_optimizer`) and calls it through
 *     info = run_optimizer(obj, veh_index, iter, mpa, options, time_step)   (OptimizerInterface.m:14)
 * from hlc/controller/prioritized/PrioritizedController.m:335-341.  A MATLAB MEX shim (or a
 * ctypes binding) marshals the 1-vehicle `iter` slice, the `mpa` tables and
 * `options` into the plain structs below and calls pdmpc_plan_batch(); one vehicle per call is the
 * literal `run_optimizer`, n vehicles per call is one computation level of
 * hlc/controller/prioritized/PrioritizedSequentialController.m:83-91.
 *
 * Conventions
 *  - every entry point returns an int status (PDMPC_OK == 0); no exceptions cross the ABI;
 *  - all floating point is IEEE double, all indices that mirror MATLAB values are 1-based
 *    (trim indices, tree node ids, tree_path) exactly as the reference stores them;
 *  - the caller owns every host buffer; the library owns all device memory inside the handle;
 *  - a handle is bound to one GPU and is not re-entrant (one call in flight per handle), which is
 *    the reference's threading model (one blocking optimizer per controller process, main.m:43-60).
 *  - polygons are stored as the reference stores them: 2 x V column lists [x; y] whose last column
 *    repeats the first (closed), see generate_maneuver.m:46 and vectorize_all_obstacles.m:68-75.
 */
#ifndef PDMPC_H
#define PDMPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDMPC_HP_MAX 16 /* largest prediction horizon Hp accepted (BASELINE configs use 5..10) */
#define PDMPC_VMAX 8    /* columns reserved per maneuver area (reference: 5, 6 or 7; generate_maneuver.m:74-101) */
#define PDMPC_JOINT_MAX 4 /* vehicles per joint problem (pdmpc_plan_joint) */

/* status codes (function results and pdmpc_vehicle_out.status) */
enum {
    PDMPC_OK = 0,
    PDMPC_EXHAUSTED = 1,        /* per vehicle: open list ran empty == info.is_exhausted (GraphSearch.m:57-61) */
    PDMPC_ARENA_OVERFLOW = 2,   /* per vehicle: search tree outgrew its arena and could not be grown further (see pdmpc_set_arena_limit);
                                   NOT an exhaustion: the reference tree is unbounded (Tree.m:54-70) and would have kept searching */
    PDMPC_ERR_INVALID = -1,     /* bad argument / inconsistent sizes */
    PDMPC_ERR_NO_DEVICE = -2,   /* no gfx950 device, or the HIP code object failed to load */
    PDMPC_ERR_HIP = -3,         /* a HIP runtime call failed; see pdmpc_last_error() */
    PDMPC_ERR_CAPACITY = -4,    /* problem does not fit the per-vehicle LDS/HBM budget of this handle */
    PDMPC_ERR_NO_MPA = -5       /* pdmpc_plan_* before pdmpc_upload_mpa */
};

/* constraint checker, chosen by OptimizerInterface.set_constraint_checker (OptimizerInterface.m:36-46)
 * from Config.are_any_obstacles_non_convex (config/Config.m:71-87) */
enum {
    PDMPC_CHECK_SAT = 0,   /* are_constraints_satisfied_sat.m  (circle scenario / convex areas) */
    PDMPC_CHECK_INTERX = 1 /* are_constraints_satisfied_interx.m + vectorize_all_obstacles.m (road networks) */
};

typedef struct pdmpc_handle pdmpc_handle;

/* options.* fields read on the hot path (config/Config.m:32-33,47) plus backend sizing */
typedef struct {
    int32_t Hp;           /* options.Hp */
    int32_t checker;      /* PDMPC_CHECK_* */
    double dt_seconds;    /* options.dt_seconds (expand_node.m:70) */
    int32_t device;       /* HIP device ordinal */
    int32_t max_nodes;    /* per-vehicle tree capacity in HBM (0 = default 32768) */
    int32_t max_vehicles; /* largest batch this handle will see (0 = default 256) */
    int32_t trace_pops;   /* unused (kept for the layout): pdmpc_debug_pop_trace reconstructs the pop sequence from the tree */
} pdmpc_config;

/* One maneuver mpa.maneuvers{i,j} (generate_maneuver.m:25-66).  area* are [2][PDMPC_VMAX]
 * row-major (row 0 = x, row 1 = y), the first n_cols columns valid. */
typedef struct {
    double dx, dy, dyaw;
    int32_t n_cols;
    int32_t _pad;
    double area[2][PDMPC_VMAX];
    double area_without_offset[2][PDMPC_VMAX];
    double area_large_offset[2][PDMPC_VMAX];
} pdmpc_maneuver;

/* The MPA tables the search reads (MotionPrimitiveAutomaton.m:5-9). */
typedef struct {
    int32_t n_trims;               /* length(mpa.trims) */
    int32_t Hp;                    /* size(transition_matrix_single, 3) */
    const uint8_t* transition;     /* [Hp][n_trims][n_trims]: transition[k][i][j] = transition_matrix_single(i+1, j+1, k+1) */
    const int32_t* maneuver_index; /* [n_trims][n_trims]: index into maneuvers[] or -1 where maneuvers{i,j} is empty */
    int32_t n_maneuvers;
    const pdmpc_maneuver* maneuvers;
} pdmpc_mpa;

/* A list of polygons/polylines: polygon p = columns offset[p] .. offset[p+1]-1 of (x, y). */
typedef struct {
    int32_t n_polygons;
    const int32_t* offset; /* [n_polygons + 1] */
    const double* x;
    const double* y;
} pdmpc_polygon_set;

/* The 1-vehicle IterationData slice (hlc/controller/common/IterationData.m:4-33, filter :95-114)
 * as PrioritizedController.plan hands it to run_optimizer (PrioritizedController.m:297-341). */
typedef struct {
    double x0, y0, yaw0;  /* iter.x0(1, 1:3) */
    int32_t trim0;        /* iter.trim_indices (1-based) */
    int32_t n_left;       /* columns of predicted_lanelet_boundary{1,1} (0 = empty, circle scenario) */
    int32_t n_right;      /* columns of predicted_lanelet_boundary{1,2} */
    int32_t _pad;
    const double* ref_x;  /* [Hp] iter.reference_trajectory_points(1, :, 1) */
    const double* ref_y;  /* [Hp] iter.reference_trajectory_points(1, :, 2) */
    const double* v_ref;  /* [Hp] iter.v_ref(1, :) */
    const double* left_x; /* left boundary polyline */
    const double* left_y;
    const double* right_x;
    const double* right_y;
    pdmpc_polygon_set obstacles;          /* iter.obstacles: n_s polygons */
    pdmpc_polygon_set dynamic_obstacles;  /* iter.dynamic_obstacle_area: n_d x Hp cell, polygon index = i*Hp + (k-1) */
    pdmpc_polygon_set hdv_reachable_sets; /* iter.hdv_reachable_sets(adjacent, :): n_h x Hp, same indexing (InterX only) */
} pdmpc_vehicle_in;

/* ControlResultsInfo for one vehicle (hlc/controller/common/ControlResultsInfo.m:5-17) in the
 * fixed-stride form create_control_results_info_from_mex expects (OptimizerInterface.m:63-101). */
typedef struct {
    int32_t status;      /* PDMPC_OK / PDMPC_EXHAUSTED / PDMPC_ARENA_OVERFLOW */
    int32_t n_expanded;  /* info.n_expanded == tree size (GraphSearch.m:58,89) */
    int32_t n_popped;    /* nodes taken from the open list, incl. rejected ones */
    int32_t n_hp;        /* Hp this record was written for */
    int32_t tree_path[PDMPC_HP_MAX + 1];   /* info.tree_path, 1-based node ids (GraphSearch.m:84) */
    int32_t predicted_trims[PDMPC_HP_MAX]; /* info.predicted_trims (GraphSearch.m:86) */
    int32_t shape_cols[PDMPC_HP_MAX];      /* columns of info.shapes{1,k} */
    int32_t _pad;
    double y_predicted[PDMPC_HP_MAX][3];   /* info.y_predicted(:, k, 1) = [x; y; yaw] (return_path_to.m:14-23); NaN if exhausted */
    double shapes[PDMPC_HP_MAX][2][PDMPC_VMAX]; /* info.shapes{1,k} (return_path_area.m:1-8) */
    double path_nodes[PDMPC_HP_MAX + 1][8]; /* rows in NodeInfo order x,y,yaw,trim,g,h,k,exactEval (NodeInfo.m:4-13) */
} pdmpc_vehicle_out;

/* counters of the last pdmpc_plan_* call, summed over the batch (feeds the roofline formula) */
typedef struct {
    int64_t n_vehicles;
    int64_t nodes_popped;
    int64_t nodes_generated;  /* children created (tree size minus roots) */
    int64_t obstacle_columns; /* sum over plans and steps of the obstacle-soup columns + boundary columns */
    int64_t algorithmic_bytes;/* SURVEY.md 8(d) formula evaluated for the call */
    double kernel_ms;         /* duration of the search kernel measured with HIP events on the launch stream */
    int64_t lds_bytes;        /* dynamic LDS per workgroup used by the launch */
    int64_t lds_nodes;        /* tree nodes resident in LDS per vehicle */
    int64_t n_launches;       /* kernel launches since the last pdmpc_pack_* (kernel_ms is their sum) */
    int64_t queue_fallbacks;  /* searches since pdmpc_create / pdmpc_reset_stats that met equal keys where the pop order decides and ended
                                 on the replay of their tree through the libstdc++-faithful binary heap (priority_queue_interface_mex.cpp:19-31) */
    int64_t speculation_arrivals; /* verifications of a running search's tree against areas of predecessors that finished meanwhile (same period) */
    int64_t edge_checks;       /* eval_edge_exact evaluations since pdmpc_create / pdmpc_reset_stats (incl. the ones the reference never makes) */
    int64_t segment_pair_tests;/* (area segment, obstacle segment) pairs those checks stand for: sum of (V-1)(M-1) per soup,
                                  InterX.m:63-76 (InterX checker only) */
    int64_t kernel;            /* kernel of the last launch: 2 the graph search (bulk-synchronous rounds), 3 the sampled optimizer,
                                  4 the joint search of centralized control (pdmpc_plan_joint: n_vehicles, nodes_popped and
                                  nodes_generated count each problem once; obstacle_columns and algorithmic_bytes are 0) */
    int64_t nodes_processed;   /* nodes whose edge was evaluated (same period; the reference pops nodes_popped of them, the rest is what
                                  the parallel rounds overshoot) */
    int64_t rounds;            /* rounds (select a batch of the smallest open keys, process it) */
    int64_t shared_rounds;     /* ... of which shared with helper workgroups (CUs the launch left idle; same period) */
    int64_t helper_checked;    /* ... and the nodes whose edges those helpers evaluated (part of nodes_processed) */
    int64_t safe_replans;      /* calls since pdmpc_create that were planned a second time in resident slices because a search of an
                                  oversubscribed launch gave up waiting for a predecessor (see pdmpc_set_safe_launch) */
    int64_t bad_status_plans;  /* plans since pdmpc_create / pdmpc_reset_stats whose record carries neither PDMPC_OK nor PDMPC_EXHAUSTED
                                  (arena overflow, predecessor time-out), counted on the device: also covers launches nobody fetched */
} pdmpc_stats;

/* Tuning.  The graph search's knobs (round sizes, helper workgroups, tiles, the open set's lists) and its A/B and test switches have
 * measured defaults; ONE environment variable, read once in pdmpc_create, overrides them for benchmarking and tests:
 *     PDMPC_TUNING="key=value,key=value,..."
 * keys: round0 round ramp ready share_min tile mid_min mid_fill (rounds and lists), tentative fast_arrival speculate helpers
 * helpers_oversub helpers_first seat_nodes waves compact generic (A/B switches; compact takes -1, 0 or 1), force_tie reverse_dispatch
 * spin_limit (testing), debug_tail debug_lds debug_host debug_progress (diagnostics); csrc/launch_plan.hpp: struct Tuning documents each.
 * The search kernels have the defaults of tentative fast_arrival speculate force_tie reverse_dispatch debug_tail compiled
 * in; any other value of one of them, or generic=1, runs the kernels' generic twins, which read them at run time.
 * No setting changes a result; an unknown key fails pdmpc_create. */

/* ---- life cycle (replaces GraphSearch() construction in OptimizerInterface.get_optimizer, :26-27,
 *      and the MEX instance table of priority_queue_interface_mex.cpp:48-53,111) ---- */
int pdmpc_create(const pdmpc_config* config, pdmpc_handle** out_handle);
int pdmpc_destroy(pdmpc_handle* handle);

/* The plan of a launch, without a device (csrc/launch_plan.hpp): what pdmpc_launch_range / pdmpc_plan_joint decide
 * before they launch -- the LDS layout, the kernel, the sizes of the rounds, the helper workgroups, the slices of the safe mode -- from the
 * same functions they call.  tuning: a PDMPC_TUNING string (NULL or empty: the defaults).  query: the configuration (checker, Hp), the
 * automaton (n_trims, n_man: maneuvers), the device (n_cu compute units, device_share: pdmpc_set_device_share, max_nodes: the arena's),
 * the launch (kind: 0 graph search, 1 sampled optimizer, 2 joint search; count: searches / vehicles / problems; n_chained: how many of
 * them have predecessors; safe: pdmpc_set_safe_launch) and the packed batch (soup_cap: obstacle columns -- for a joint launch the most
 * distinct soup columns of a problem + 2 --, ll_cap: boundary columns, cand_cap: segments of one edge check).  plan: the layout's
 * numbers, the launch policy (the fields of the same names in csrc/pdmpc_device.h: KernelArgs), variant / generic / kernel (which search
 * kernel, static name), slice (searches per kernel launch), heap_lds (joint), then every region's byte offset (graph search and sampled
 * optimizer: LdsLayout; joint: JointLds, the others 0).  PDMPC_ERR_INVALID: a tuning error (pdmpc_last_error: the text pdmpc_create
 * gives); PDMPC_ERR_CAPACITY: the soup and the automaton's tables do not fit into LDS. */
typedef struct {
    int32_t checker, Hp, n_trims, n_man;
    int32_t n_cu, device_share, max_nodes;
    int32_t kind;
    int32_t count, n_chained;
    int32_t soup_cap, ll_cap, cand_cap, safe;
} pdmpc_launch_query;
typedef struct {
    int32_t n_waves, NL, NV, areas_in_lds, ready, compact;
    int32_t bk_ready_cap, bk_round0, bk_round, bk_ramp, bk_tile, bk_share_min, n_helpers, bk_helpers_first, bk_seat_nodes, reverse_dispatch;
    int32_t variant, generic, slice, heap_lds;
    uint32_t spin_limit;
    uint32_t mask, man_index, pose, area, ref, shape, path, soup, cand, vstate, expand, tree16, rand, nodes, total;
    uint32_t bk_near_key, bk_near_id, bk_ready, bk_hist, bk_misc, bk_pshape, reach_shared, bk_reach, reach;
    uint32_t ints, succ, heap_key, heap_id;
    const char* kernel;
} pdmpc_launch_plan;
int pdmpc_launch_plan_host(const char* tuning, const pdmpc_launch_query* query, pdmpc_launch_plan* plan);

/* the configuration the handle runs with (defaults filled in, max_nodes = current arena size) and whether the MPA is uploaded */
int pdmpc_get_config(pdmpc_handle* handle, pdmpc_config* config, int32_t* mpa_uploaded);

/* uploads mpa.maneuvers / mpa.transition_matrix_single once (MotionPrimitiveAutomaton.m:5-9) */
int pdmpc_upload_mpa(pdmpc_handle* handle, const pdmpc_mpa* mpa);
/* The automaton's reach (include/pdmpc_reach.h): dmax = the longest maneuver displacement hypot(dx, dy), amax = the
 * largest hypot over the used columns of area, area_without_offset and area_large_offset.  Every point of every area a graph search
 * checks at step k lies within (k - 1) dmax + amax of its root.  pdmpc_upload_mpa stores the two behind the maneuver areas. */
int pdmpc_mpa_reach_host(const pdmpc_mpa* mpa, double* dmax, double* amax);
/* The segments in reach of each step of a search rooted at (root_x, root_y), by the rule of include/pdmpc_reach.h: the host twin of
 * the lists the graph-search kernel builds in LDS.  Step k = 1 .. Hp has the step_count[k - 1] soup columns of (x, y) from column
 * step_first[k - 1] on (ranges may repeat: the lanelet boundary is the same for every step); its segment j joins columns j and j + 1 of
 * that range.  Out: list[list_offset[k - 1] .. list_offset[k]) = the segments in reach of step k, ascending (list holds up to one entry
 * per segment of every step). */
int pdmpc_reach_lists_host(int32_t Hp, double dmax, double amax, double root_x, double root_y, const double* x, const double* y, const int32_t* step_first,
                           const int32_t* step_count, int32_t* list_offset, int32_t* list);
/* The automaton's reach rectangles (include/pdmpc_reach.h, the oriented rule): rects[(r * Hp + k - 1) * 4 ..] = (x_lo, x_hi,
 * y_lo, y_hi), in the frame of a root at the origin with yaw 0 in trim r + 1, of every point of every area (three variants, used columns)
 * a graph search can check at step k = 1 .. Hp under the transition masks of steps 1 .. k; NaN where there is none.  rects holds
 * n_trims * Hp * 4 doubles, 1 <= Hp <= mpa.Hp.  pdmpc_upload_mpa stores the table of config.Hp behind dmax and amax. */
int pdmpc_mpa_reach_rects_host(const pdmpc_mpa* mpa, int32_t Hp, double* rects);
/* pdmpc_reach_lists_host by the oriented rule: the root has yaw root_yaw and trim root_trim (1-based), rects is the table of
 * pdmpc_mpa_reach_rects_host for n_trims trims and this Hp.  The host twin of the lists the graph-search kernel builds. */
int pdmpc_reach_lists_oriented_host(int32_t Hp, int32_t n_trims, const double* rects, int32_t root_trim, double root_x, double root_y, double root_yaw, const double* x, const double* y,
                                    const int32_t* step_first, const int32_t* step_count, int32_t* list_offset, int32_t* list);

/* Plans n independent vehicles (one computation level).  Blocking.  With n == 1 this is
 * GraphSearch.run_optimizer (GraphSearch.m:14-17). */
int pdmpc_plan_batch(pdmpc_handle* handle, int32_t n_vehicles, const pdmpc_vehicle_in* in,
                     pdmpc_vehicle_out* out);

/* Arena growth.  The reference's search tree is unbounded (Tree.m:54-70: add_nodes appends); this backend keeps the tree of
 * every vehicle in a fixed HBM arena of config.max_nodes nodes.  pdmpc_plan_batch / pdmpc_plan_step therefore re-plan a
 * call in which some search outgrew its arena with arenas twice as large (the searches are deterministic: vehicles that
 * fitted produce the same records again), repeatedly, until every search fits.  PDMPC_ARENA_OVERFLOW is only ever
 * returned when the limit set here is reached (max_nodes_limit == current size: growth off; 0: up to what HBM holds). */
int pdmpc_set_arena_limit(pdmpc_handle* handle, int32_t max_nodes_limit);
/* explicit growth for the device-resident path below (launch / fetch do not grow by themselves) */
int pdmpc_grow_arena(pdmpc_handle* handle, int32_t max_nodes);
/* current per-vehicle arena size and how often a call had to be re-planned with larger arenas since pdmpc_create */
int pdmpc_arena_nodes(pdmpc_handle* handle, int32_t* max_nodes, int64_t* regrows);

/* A whole time step in one call (PrioritizedSequentialController.controller, :77-94): pdmpc_pack_step + launch + fetch,
 * with arena growth as above.  Arguments as for pdmpc_pack_step (below). */
int pdmpc_plan_step(pdmpc_handle* handle, int32_t n_vehicles, const pdmpc_vehicle_in* in, const int32_t* pred_offset,
                    const int32_t* pred_index, const pdmpc_polygon_set* fallback_shapes, pdmpc_vehicle_out* out);

/* The same step the way an UNMODIFIED reference controller drives this backend: one pdmpc_plan_batch of ONE vehicle per
 * run_optimizer call (PrioritizedController.m:335-341) in kahn order (PrioritizedSequentialController.m:77-94), the predecessors'
 * solved areas handed over on the host as dynamic obstacles (PrioritizedController.m:476-491).  Arguments and records as for
 * pdmpc_plan_step (slots in level order).  The slow way to use the library: bench.py reports it as value_run_optimizer_literal. */
int pdmpc_plan_step_literal(pdmpc_handle* handle, int32_t n_vehicles, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                            const pdmpc_polygon_set* fallback_shapes, pdmpc_vehicle_out* out);

/* ---- device-resident path used by the batched host driver and bench.py ----
 * pdmpc_pack_batch flattens host inputs into the handle's device blob (H2D copy, async on the
 * handle's stream); pdmpc_launch_packed runs the search kernel on whatever is packed (no copies);
 * pdmpc_fetch_results copies the result records back.  pdmpc_plan_batch == pack + launch + fetch.
 * A pack writes the batch straight into the selected bank's staging memory: one that fails (invalid input, out of memory) leaves that
 * bank EMPTY — the batch that was in it is gone, a launch on it returns PDMPC_ERR_INVALID until the next successful pack. */
int pdmpc_pack_batch(pdmpc_handle* handle, int32_t n_vehicles, const pdmpc_vehicle_in* in);
/* pdmpc_plan_step for a caller that keeps only a few of the batch's plans (the explorative step: the choice among the prioritizations
 * rests on the cost-to-come of every vehicle's final node, PrioritizedExplorativeController.m:94-112, and only the chosen plans are
 * applied): plans the step like pdmpc_plan_step but copies back status[v] and final_cost[v] = path_nodes[Hp][4] only (12 bytes per
 * vehicle instead of 2.9 KB); the records stay on the device until the next launch and pdmpc_fetch_records_at reads the ones wanted
 * (vehicles: indices into the step as it was handed over). */
int pdmpc_plan_step_lean(pdmpc_handle* handle, int32_t n_vehicles, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                         const pdmpc_polygon_set* fallback_shapes, int32_t* status, double* final_cost);
int pdmpc_fetch_records_at(pdmpc_handle* handle, int32_t count, const int32_t* vehicles, pdmpc_vehicle_out* out);
/* ---- the choice among the plans of a batch, as data (csrc/choice_kernel.hip) ----
 * One description covers the explorative choice (PrioritizedExplorativeController.m:94-176), the optimal-priority choice
 * (PrioritizedOptimalController.m:56-114), follow-own, and any concatenation of these over the members of a sweep.  Slots are the
 * caller's slots of the planned batch.
 *   cells   cell c = the sum, started at +0.0 and added IN LIST ORDER, over cell_slot[cell_offset[c] .. cell_offset[c + 1]) of
 *           status == PDMPC_OK ? path_nodes[Hp][4] : +inf, then rounded as round(., 8): nearbyint(v * 1e8) / 1e8.  The order of the
 *           list is the order of addition and part of the contract (the sums are doubles).
 *   graphs  the candidates of graph g are the consecutive cells graph_offset[g] .. graph_offset[g + 1] - 1; chosen[g] = the index
 *           among them of the first minimum ([~, i] = min(.)); all candidates +inf (or none): 0.
 *   picks   pick i returns the record of slot pick_slot[pick_offset[i] + chosen[pick_graph[i]]]; with pick_graph[i] == -1 its single
 *           listed slot (follow-own).
 * Only PDMPC_OK and PDMPC_EXHAUSTED are planning results: any other status among the batch's n records — whether a cell lists the
 * record or not — makes the choice fail with PDMPC_ERR_HIP.
 * Checked before anything is launched (PDMPC_ERR_INVALID): offsets are not negative and do not decrease, graph offsets stay within the cells,
 * slots lie within the batch, pick_graph within [-1, n_graphs), and a pick lists as many slots as its graph has candidates (one for
 * pick_graph == -1). */
typedef struct {
    int32_t n_cells;
    int32_t n_graphs;
    int32_t n_picks;
    int32_t _pad;
    const int32_t* cell_offset;  /* [n_cells + 1] */
    const int32_t* cell_slot;
    const int32_t* graph_offset; /* [n_graphs + 1] */
    const int32_t* pick_graph;   /* [n_picks] */
    const int32_t* pick_offset;  /* [n_picks + 1] */
    const int32_t* pick_slot;
} pdmpc_choice;
/* The choice on the host (no GPU needed): status[n] and final_cost[n] = path_nodes[Hp][4] of the batch's records; chosen[n_graphs] and
 * cell_cost[n_cells] (either may be NULL).  Picks are validated and otherwise ignored.  The twin and checker of the device choice. */
int pdmpc_choose_host(int32_t n, const int32_t* status, const double* final_cost, const pdmpc_choice* choice, int32_t* chosen, double* cell_cost);
/* The choice on the device, on the n records resident in the current bank (after pdmpc_launch_packed, pdmpc_import_results, ...): the
 * sums and the first minima in one launch, the gather of the picked records in a second, ONE copy back (picked records, chosen, cell
 * costs and the status counters) and one synchronisation.  picks[n_picks]; chosen / cell_cost may be NULL.  Slots are the caller's
 * vehicles also for a batch that pdmpc_pack_step put into level order (then n must be the packed batch). */
int pdmpc_choose_resident(pdmpc_handle* handle, int32_t n, const pdmpc_choice* choice, int32_t* chosen, double* cell_cost, pdmpc_vehicle_out* picks);
/* pdmpc_plan_step + the choice on the device: packs, launches and chooses with no host synchronisation between the search's launch
 * and the read-back.  Arena overflow and predecessor time-outs are read from counters the choice keeps on the device and handled as
 * pdmpc_plan_step handles them (planned again with larger arenas / in resident slices).  pdmpc_last_call_timing as for pdmpc_plan_step. */
int pdmpc_plan_step_chosen(pdmpc_handle* handle, int32_t n_vehicles, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                           const pdmpc_polygon_set* fallback_shapes, const pdmpc_choice* choice, int32_t* chosen, double* cell_cost, pdmpc_vehicle_out* picks);
/* kernel time (HIP events, ms) of the two launches of the last pdmpc_choose_resident / pdmpc_plan_step_chosen */
int pdmpc_choice_kernel_ms(pdmpc_handle* handle, double* ms);
/* host wall-clock microseconds of the last pdmpc_plan_batch / pdmpc_plan_step / pdmpc_plan_joint on this handle: [0] pack (flatten + queue the
 * host-to-device copy), [1] enqueue the launch, [2] wait for the kernel + copy the records back */
int pdmpc_last_call_timing(pdmpc_handle* handle, double* us3);
int pdmpc_launch_packed(pdmpc_handle* handle);
/* launches only slots [first, first + count) of the packed batch: one computation level, or one GPU's shard of it */
int pdmpc_launch_range(pdmpc_handle* handle, int32_t first, int32_t count);
int pdmpc_fetch_results(pdmpc_handle* handle, int32_t n_vehicles, pdmpc_vehicle_out* out);
int pdmpc_synchronize(pdmpc_handle* handle);
/* Forward progress of launches with more searches than resident workgroups (256 CUs x 1 workgroup; x 2 with the compact kernel).
 * A search spins for predecessors of the same launch.  Every predecessor sits in a lower slot (pdmpc_pack_step puts a batch into a
 * topological order of its coupling DAG — level order, or priority order with pdmpc_set_step_weights — unless it is in one already),
 * so as long as the hardware hands workgroups out IN INDEX ORDER whoever a search waits for was dispatched before it and the launch
 * cannot stall.  THAT ORDER IS AN ASSUMPTION about the dispatcher (observed on gfx950 / ROCm 7, not a documented guarantee).
 * Should a launch stall anyway, the kernel's watchdog (spin limit) ends the waiting searches with status PDMPC_ERR_HIP.
 * Which entry points recover by themselves:
 *   pdmpc_plan_batch, pdmpc_plan_step, pdmpc_plan_step_literal, pdmpc_controller_step / _run / _explore_*  — plan the call again in
 *     slices that are resident as a whole (predecessors in the same or an earlier slice: no assumption left), counted in
 *     pdmpc_stats.safe_replans;
 *   pdmpc_launch_packed, pdmpc_launch_range, pdmpc_group_launch, pdmpc_group_plan_step (the resident paths)  — do NOT: the records
 *     carry the error status (pdmpc_stats.bad_status_plans counts them on the device) and the caller decides.
 * pdmpc_set_safe_launch(on != 0) makes every launch of this handle, resident paths included, use the resident slices from the start.
 * Tested against the adversarial order with PDMPC_TUNING=reverse_dispatch=1 (tests/test_gpu_step.py). */
int pdmpc_set_safe_launch(pdmpc_handle* handle, int32_t on);
/* n_handles handles of this process launch on the handle's device side by side (pdmpc_group_create_ex sets it for logical ranks that
 * share a GPU): the helper workgroups of a launch are sized for 1 / n_handles of the device's idle CUs and none of them is dispatched
 * in front of the searches — four launches with half a chip's worth of helpers in front of each would fill the device with helpers
 * that wait for searches which cannot start. */
int pdmpc_set_device_share(pdmpc_handle* handle, int32_t n_handles);
/* starts a new time step for launches issued with pdmpc_launch_range: results of earlier steps stop
 * satisfying predecessor waits (pdmpc_launch_packed does this implicitly) */
int pdmpc_begin_step(pdmpc_handle* handle);
/* several packed batches can stay resident in HBM side by side; pack/launch/fetch act on the selected
 * bank (default 0).  bench.py keeps one bank per recorded time step so the timed region has no copies. */
int pdmpc_select_bank(pdmpc_handle* handle, int32_t bank);
/* forget the kernel timings accumulated so far (pdmpc_get_last_stats sums launches since the last reset/pack) */
int pdmpc_reset_stats(pdmpc_handle* handle);

/* Step-level planning (PrioritizedSequentialController.controller, :77-94): all vehicles of a
 * time step in ONE launch.  pred_offset/pred_index (CSR over vehicles, 0-based vehicle indices of
 * this batch) list each vehicle's sequential predecessors; their solved info.shapes(1,:) are appended
 * on the device to the vehicle's dynamic obstacles (PrioritizedController.m:476-491) before it plans.
 * fallback_shapes (may be NULL) gives, per vehicle, the Hp areas published when its search is
 * exhausted (PrioritizedController.m:568-616,678-718): [n][Hp] pdmpc_polygon_set-style via offsets. */
/* Expected work per vehicle of the NEXT packed step (n = its vehicle count, the caller's vehicle order; e.g. n_popped of the previous
 * time step), consumed by the next pdmpc_pack_step / pdmpc_plan_step / pdmpc_pack_batch.  With it, a launch of the whole step hands its
 * searches out by priority — the largest expected work among a vehicle and its descendants in the coupling DAG, descending — instead
 * of slot order: still a topological order (whoever a search waits for was dispatched before it), but in a launch of more searches
 * than CUs the heavy searches of late computation levels start with the launch instead of behind the finished searches that wait for
 * their predecessors.  Slots, records and results are the same bit for bit.  Optional: without it searches go out in slot order.
 * A pack that fails consumes the weights too: the pack after it has none. */
int pdmpc_set_step_weights(pdmpc_handle* handle, int32_t n_vehicles, const double* weights);
int pdmpc_pack_step(pdmpc_handle* handle, int32_t n_vehicles, const pdmpc_vehicle_in* in,
                    const int32_t* pred_offset, const int32_t* pred_index,
                    const pdmpc_polygon_set* fallback_shapes);

/* raw device pointer + byte size of the packed result records (pdmpc_vehicle_out[n]) for exchange
 * between GPUs (RCCL all-gather of solved areas).  This entry point, pdmpc_import_results and
 * pdmpc_export_results(_async) address SLOTS: they return PDMPC_ERR_INVALID for a batch that pdmpc_pack_step had to put into level
 * order itself (slots then are not the caller's vehicles); pack in level order -- predecessors in lower slots -- to use them. */
int pdmpc_result_device_buffer(pdmpc_handle* handle, void** dev_ptr, size_t* nbytes);
/* make result records produced elsewhere (e.g. gathered from another GPU into dev_ptr) visible as
 * predecessor outputs: copies n records into slots [first, first+n) of the handle's result buffer */
int pdmpc_import_results(pdmpc_handle* handle, int32_t first, int32_t n, const void* dev_records);
/* the other direction: copies the records of slots [first, first+n) into the caller's DEVICE buffer (the send
 * buffer of the all-gather) and waits for the copy, so the buffer can be handed to another stream */
int pdmpc_export_results(pdmpc_handle* handle, int32_t first, int32_t n, void* dev_records);

/* the same without the wait: the copy is only ordered on the handle's stream (see pdmpc_stream) */
int pdmpc_export_results_async(pdmpc_handle* handle, int32_t first, int32_t n, void* dev_records);
/* The HIP stream (hipStream_t) every launch and copy of this handle is enqueued on.  A caller that exchanges records
 * between GPUs enqueues its collective on THIS stream (e.g. torch.cuda.ExternalStream around it), so export -> all-gather
 * -> import -> next launch are ordered by the stream itself, with no host synchronisation and no cross-stream race. */
int pdmpc_stream(pdmpc_handle* handle, void** hip_stream);

int pdmpc_get_last_stats(pdmpc_handle* handle, pdmpc_stats* stats);

/* ---- debug / parity instrumentation (no reference counterpart: the reference keeps the whole
 *      Tree in info.tree, Tree.m:3-13; these calls read it back from HBM) ---- */
/* node ids popped by vehicle v in order; returns count in *n */
int pdmpc_debug_pop_trace(pdmpc_handle* handle, int32_t vehicle, int32_t capacity, int32_t* ids, int32_t* n);
/* the search tree of vehicle v: arrays of length capacity, *n receives tree size */
int pdmpc_debug_tree(pdmpc_handle* handle, int32_t vehicle, int32_t capacity, double* x, double* y,
                     double* yaw, double* g, double* h, int32_t* trim, int32_t* k, int32_t* parent,
                     int32_t* n);

/* The collision primitives on given polygons, n_cases at once (one wavefront each, the device functions the search kernels
 * inline): mode 0 = InterX(a, b) (graph_search/InterX.m:48-103, isReturnPoints = false; b may hold NaN separators),
 * mode 1 = intersect_sat(a, b) (graph_search/intersect_sat.m:1-42), mode 2 = intersect_lanelet_boundary(a, [left, NaN, right, NaN])
 * (optimizer/common/intersect_lanelet_boundary.m:1-56), mode 3 = intersect_sat(a, p) for any polygon p of the NaN-separated soup b
 * (are_constraints_satisfied_sat.m:15-35).  Case c: a = columns a_off[c] .. a_off[c+1]-1 of (a_x, a_y), at most
 * PDMPC_VMAX; b likewise, at most 1024 columns; PDMPC_ERR_INVALID for more, before any launch.  hit[c] = 1 if the reference function
 * returns true.  Every mode runs the wave-wide form and the per-lane form of its check; should they disagree, hit[c] = 2 + the per-lane
 * answer. */
int pdmpc_debug_edge_check(pdmpc_handle* handle, int32_t mode, int32_t n_cases, const int32_t* a_off, const double* a_x, const double* a_y,
                           const int32_t* b_off, const double* b_x, const double* b_y, int32_t* hit);
/* The InterX check of one edge on its three soups (are_constraints_satisfied_interx.m:17-37): InterX(A, vehicle soup) || InterX(A, HDV
 * soup) || InterX(B, lanelet boundary).  Case c: shape A = columns a_off[c] .. a_off[c+1]-1 of (a_x, a_y) and shape B = the same columns
 * of (b_x, b_y), at most PDMPC_VMAX; its soups 3c, 3c+1, 3c+2 = columns s_off[3c+q] .. s_off[3c+q+1]-1 of (s_x, s_y), at most 1024
 * columns together; PDMPC_ERR_INVALID for more, before any launch.  hit[c] as for pdmpc_debug_edge_check. */
int pdmpc_debug_interx_soups(pdmpc_handle* handle, int32_t n_cases, const int32_t* a_off, const double* a_x, const double* a_y, const double* b_x,
                             const double* b_y, const int32_t* s_off, const double* s_x, const double* s_y, int32_t* hit);
/* include/pdmpc_math.h's pdmpc_sincos in a kernel: s[i], c[i] = sin, cos of x[i], i < n */
int pdmpc_debug_sincos(pdmpc_handle* handle, int32_t n, const double* x, double* s, double* c);

/* the arena of vehicle v as the kernel left it (the frontier kernel's own creation order, incl. nodes the reference never
 * creates), with every node's open-list key and validity byte (0 never evaluated, 1 collision-free, 2 colliding) */
int pdmpc_debug_raw_tree(pdmpc_handle* handle, int32_t vehicle, int32_t capacity, double* x, double* y, double* yaw, double* g,
                         double* h, int32_t* trim, int32_t* k, int32_t* parent, double* key, uint8_t* validity, int32_t* n);

/* the device's work counters since pdmpc_create / pdmpc_reset_stats, raw: [0..6] as pdmpc_stats reports them, [8..12] with
 * PDMPC_TUNING=debug_tail=1 the helper workgroups' time in 100 MHz ticks (idle, claim -> soup, records, checks, verdicts + report), [13] tiles */
int pdmpc_debug_counters(pdmpc_handle* handle, uint64_t* out16);
/* where the last pack put the caller's vehicle `vehicle` in the batch's point pool: lit_off[Hp + 1] and hdv_off[Hp + 1] (the per-step
 * soups of its obstacles and HDV sets), ll2 = {offset, length} of its lanelet boundary.  Vehicles that handed over the same arrays
 * report the same offsets (one copy in the pool). */
int pdmpc_debug_packed_offsets(pdmpc_handle* handle, int32_t vehicle, int32_t* lit_off, int32_t* hdv_off, int32_t* ll2);

/* live counters of a running frontier launch (needs PDMPC_DEBUG_PROGRESS=1 in the environment; callable from another thread
 * while pdmpc_plan_* blocks): rounds, nodes processed, tree size, near / far entries, flags, best candidate, stage */
int pdmpc_debug_progress(pdmpc_handle* handle, int32_t vehicle, uint32_t* words16);

/* drives the device open list with a command script (op[i] == 0: push (id[i], key[i]); op[i] == 1: pop) the way the
 * reference drives priority_queue_interface_mex (PUSH / POP, .cpp:62-99); popped[] receives the popped ids (-1 on an empty
 * queue).  lds_entries = how many heap entries live in LDS (the rest spills to HBM).  Used by the heap-order unit test. */
int pdmpc_debug_heap_script(pdmpc_handle* handle, int32_t n, const int32_t* op, const int32_t* id, const double* key,
                            int32_t lds_entries, int32_t* popped, int32_t* n_popped, double* cycles_per_pop,
                            double* cycles_per_push);

/* ---- the sampled optimizer (replaces MonteCarloTreeSearch.run_optimizer, graph_search/MonteCarloTreeSearch.m:30-35,
 *      selected by OptimizerType.MatlabSampled in OptimizerInterface.get_optimizer, OptimizerInterface.m:29-31) ----
 * One computation level like pdmpc_plan_batch.  seeds[i] = time_step + vehicle_index of vehicle i, the seed of its
 * mt19937ar stream (:32).  Records: status OK / EXHAUSTED, n_expanded = expansions (:209), tree_path = node ids of the
 * chosen descent, path_nodes rows with g = -1 except the cost of the chosen node, h = -1, k = 1..Hp+1 (:223-244). */
int pdmpc_plan_batch_sampled(pdmpc_handle* handle, int32_t n_vehicles, const pdmpc_vehicle_in* in, const uint32_t* seeds,
                             pdmpc_vehicle_out* out);
/* A whole time step of the sampled optimizer in one launch: arguments, slot order, level reordering, fallback areas
 * and records as for pdmpc_plan_step; seeds[v] = time_step + vehicle_index of the caller's vehicle v.  A slot waits on the device for
 * its predecessors (blocking, no speculation) and plans against their areas — a predecessor's solved areas, or its fallback areas if
 * it was exhausted, which an exhausted slot publishes in its record.  Every slot draws its first Hp * 250 numbers of mt19937ar(seed)
 * itself.  A watchdog time-out is re-planned in resident slices as for pdmpc_plan_step; there are no arenas to grow.  Stats: kernel 3.
 * Equivalent to pdmpc_set_step_seeds(seeds) + pdmpc_plan_step.  PDMPC_ERR_INVALID for a NULL handle and for NULL seeds with n > 0. */
int pdmpc_plan_step_sampled(pdmpc_handle* handle, int32_t n_vehicles, const pdmpc_vehicle_in* in, const int32_t* pred_offset,
                            const int32_t* pred_index, const pdmpc_polygon_set* fallback_shapes, const uint32_t* seeds,
                            pdmpc_vehicle_out* out);
/* Seeds of the sampled optimizer per vehicle of the NEXT packed step (the caller's vehicle order), consumed by the next
 * pdmpc_pack_step / pdmpc_plan_step / pdmpc_plan_step_lean / pdmpc_pack_batch, which then packs a SAMPLED bank: every launch of that
 * bank (pdmpc_launch_packed, pdmpc_launch_range, the plan calls) runs the sampled optimizer instead of the graph search, and the
 * resident path (pack once, launch many; pdmpc_fetch_records_at) works as for the graph search.  A pack without seeds packs a graph
 * search bank.  A pack that fails consumes the seeds too; a pack of another vehicle count than n_vehicles fails (PDMPC_ERR_INVALID). */
int pdmpc_set_step_seeds(pdmpc_handle* handle, int32_t n_vehicles, const uint32_t* seeds);
/* the sampled optimizer's device generator on its own: out[i * n + j] = the j-th double of mt19937ar(seeds[i]) (n <= 4000) */
int pdmpc_debug_random_numbers(pdmpc_handle* handle, int32_t count, const uint32_t* seeds, int32_t n, double* out);

/* The sampled optimizer's expansion budget: n_expansions_max of MonteCarloTreeSearch.m:8, which the reference's constructor (:16-26)
 * overrides from config/mcts.json -- the optimizer's one quality / time knob.  The budget is the handle's, as its
 * automaton is: the NEXT pack of a sampled bank reads it and it stays with that bank (resident banks keep the budget they were packed
 * with; a re-plan after a watchdog time-out keeps it too).  A slot then draws the first Hp * budget numbers of mt19937ar(seed).
 * PDMPC_SAMPLED_BUDGET_DEFAULT runs pdmpc_sampled_kernel exactly as before; any other budget runs pdmpc_sampled_budget_kernel, whose
 * tree lives in LDS where it fits and in a per-handle HBM buffer otherwise (allocated by the pack; PDMPC_ERR_CAPACITY if that fails).
 * PDMPC_SAMPLED_BUDGET_MAX keeps node ids in 16 bits (nodes <= 1 + budget + Hp - 1) and a slot's tree at about 590 KB.
 * PDMPC_ERR_INVALID for a NULL handle or pointer and for a budget outside 1..PDMPC_SAMPLED_BUDGET_MAX (the handle keeps its budget). */
#define PDMPC_SAMPLED_BUDGET_DEFAULT 250
#define PDMPC_SAMPLED_BUDGET_MAX 16384
int pdmpc_set_sampled_budget(pdmpc_handle* handle, int32_t n_expansions_max);
int pdmpc_get_sampled_budget(pdmpc_handle* handle, int32_t* n_expansions_max);
/* The name of the kernel the handle's last sampled launch ran ("" before the first one): a static string. */
const char* pdmpc_last_sampled_kernel(pdmpc_handle* handle);
/* The plan of a sampled launch with a budget, without a device: pdmpc_launch_plan_host's query (kind is ignored) and record, and what
 * the budget adds in extra[4].  PDMPC_SAMPLED_BUDGET_DEFAULT gives pdmpc_launch_plan_host's plan of kind 1, field for field.
 * extra[0] node capacity: rows of a slot's tree, more than budget + Hp, so that the tree never ends a search the reference would continue;
 * extra[1] tree_in_lds: 1 if the layout holds the tree (the 80 KB layout first, then the 160 KB one), 0 if it is in HBM; extra[2] bytes of
 * the HBM tree per slot (0 with the tree in LDS); extra[3] the random-number chunk: numbers drawn at a time (Hp * 250 for the default
 * kernel, one twist of 312 otherwise).  Errors as for pdmpc_launch_plan_host, and PDMPC_ERR_INVALID for a budget outside
 * 1..PDMPC_SAMPLED_BUDGET_MAX. */
int pdmpc_sampled_plan_host(const char* tuning, const pdmpc_launch_query* query, int32_t n_expansions_max, pdmpc_launch_plan* plan,
                            int64_t* extra);
/* ... and the same plan for the handle's current bank (the dimensions pdmpc_launch_range reads: the automaton, the device, the packed
 * obstacle columns) at any budget: where a budget would put this bank's trees.  PDMPC_ERR_INVALID for a NULL argument, an empty bank or a
 * bank packed without seeds. */
int pdmpc_sampled_plan_bank(pdmpc_handle* handle, int32_t n_expansions_max, pdmpc_launch_plan* plan, int64_t* extra);
/* the chunked generator of pdmpc_sampled_budget_kernel on its own: out[i * n + j] = the j-th double of mt19937ar(seeds[i]), any n >= 0 */
int pdmpc_debug_random_stream(pdmpc_handle* handle, int32_t count, const uint32_t* seeds, int32_t n, double* out);

/* Seed ensembles of the sampled optimizer: every vehicle of a sampled bank is planned by E members side by side,
 * each the whole sampled search on a random stream of its own, and the cheapest collision-free plan becomes the vehicle's record ON
 * THE DEVICE, before the done flag its successors wait for.  E (1..PDMPC_SAMPLED_ENSEMBLE_MAX) is the handle's, like the budget: the
 * NEXT pack of a sampled bank reads it and it stays with that bank (resident launches and the re-plan in slices after a watchdog
 * time-out keep it).  The default is 1, and with E == 1 nothing changes: the same kernels, the same bytes.
 *  - Member e (0-based) of a vehicle with seed s draws from mt19937ar(PDMPC_SAMPLED_MEMBER_SEED(s, e)); member 0 is the reference's
 *    stream.  Every member runs the search as it is (the same descents, checks and floating-point order) at the handle's budget
 *    against the same obstacles, the predecessors' published areas among them.
 *  - The winner is the member with status PDMPC_OK and the smallest final cost (path_nodes[Hp][4], compared as doubles with <; on
 *    equality the lowest member index).  The vehicle's record is the winner's, byte for byte what pdmpc_plan_step_sampled returns
 *    for the vehicle with the winner's seed and the same predecessor records.
 *  - No member OK: the record is member 0's, status PDMPC_EXHAUSTED, with the vehicle's fallback areas as before.  Any member timed
 *    out waiting for predecessors: the record's status is PDMPC_ERR_HIP and the host re-plans in slices as before.
 *  - Forward progress: the grid is count * E workgroups, block b is member b % E of slot b / E, so all members of a slot lie below
 *    the blocks of its successors.  No member ever waits for a member: each writes its record and a 16-byte entry, draws a ticket,
 *    and only the one that arrives last picks the winner, copies its record and sets the slot's done flag.  A workgroup still depends
 *    only on workgroups dispatched before it (see pdmpc_plan_step).
 * PDMPC_ERR_INVALID for a NULL argument and for a size outside 1..PDMPC_SAMPLED_ENSEMBLE_MAX (the handle keeps its value).  A pack
 * with E > 1 allocates E records, entries and -- where the budget puts trees in HBM -- trees per slot: PDMPC_ERR_CAPACITY if that
 * fails (the bank is then empty and the handle goes on working). */
#define PDMPC_SAMPLED_ENSEMBLE_MAX 16
#define PDMPC_SAMPLED_ENSEMBLE_STRIDE 1000003u
#define PDMPC_SAMPLED_MEMBER_SEED(seed, e) ((uint32_t)((uint32_t)(seed) + (uint32_t)(e) * PDMPC_SAMPLED_ENSEMBLE_STRIDE)) /* modulo 2^32 */
int pdmpc_set_sampled_ensemble(pdmpc_handle* handle, int32_t n_members);
int pdmpc_get_sampled_ensemble(pdmpc_handle* handle, int32_t* n_members);
/* PDMPC_SAMPLED_MEMBER_SEED as a call (what a host twin of another language evaluates) */
uint32_t pdmpc_sampled_member_seed(uint32_t seed, int32_t member);
/* The members of the current bank's last launch, in the caller's vehicle order: winner[v] (the member whose record the vehicle got: 0
 * if none was OK, the first timed-out member after a time-out), member_status[v * E + e] and member_cost[v * E + e] (+inf where the
 * member is not OK).  Any output may be NULL.  One small copy of the 16-byte entries, not of records.  PDMPC_ERR_INVALID for a NULL
 * handle, a vehicle count other than the bank's, and a bank that was not packed as an ensemble (E > 1) or not launched since. */
int pdmpc_sampled_ensemble_result(pdmpc_handle* handle, int32_t n_vehicles, int32_t* winner, int32_t* member_status, double* member_cost);
/* pdmpc_sampled_plan_host with an ensemble size: extra is an int64[8].  n_members == 1 gives that call's plan and extra[0..3] field
 * for field.  Otherwise the plan is the ensemble kernel's (pdmpc_sampled_ensemble_kernel, _hbm with the trees in HBM) on the budget
 * kernel's layout at ANY budget, the default included; slice counts slots.  extra[4] bytes of member records per slot and extra[5] bytes
 * of HBM trees per slot (both times E; 0 for one member), extra[6] the workgroups of a kernel launch: min(slice, count) * n_members,
 * extra[7] n_members.  PDMPC_ERR_INVALID also for n_members outside 1..PDMPC_SAMPLED_ENSEMBLE_MAX. */
int pdmpc_sampled_ensemble_plan_host(const char* tuning, const pdmpc_launch_query* query, int32_t n_expansions_max, int32_t n_members,
                                     pdmpc_launch_plan* plan, int64_t* extra);

/* ---- centralized control: one joint graph search over several vehicles (CentralizedController.m:34-46, GraphSearch.do_graph_search
 *      with iter.amount = N; separating-axis checker only) ----
 * n_problems independent joint searches in one launch.  Problem p = vehicles in[problem_offset[p] .. problem_offset[p+1]), 1 to
 * PDMPC_JOINT_MAX of them.  Each vehicle's obstacles and dynamic_obstacles are the sets its own check reads (a caller mirroring the
 * reference passes the scenario's sets to every vehicle); hdv_reachable_sets is ignored.  A tree node holds one pose and trim per
 * vehicle; children are the Cartesian product of the vehicles' successor trims, vehicle 1 varying fastest (expand_node.m:15-29), and
 * a node is valid iff no vehicle's area meets an obstacle, a lower-numbered vehicle's area of the same node, or its lanelet boundary
 * (GraphSearch.m:130-193, are_constraints_satisfied_sat.m).  out[i] = vehicle i's slice of its problem's ControlResultsInfo:
 * status / n_expanded / n_popped / tree_path shared by the problem, its own predicted_trims, y_predicted, shapes; path_nodes rows
 * (x_v, y_v, yaw_v, trim_v, g, h, k, 1) with the joint g and h.  The arena holds config.max_nodes joint nodes per problem and grows
 * as for pdmpc_plan_batch (PDMPC_ARENA_OVERFLOW only at the limit).  PDMPC_ERR_INVALID for a handle whose checker is not
 * PDMPC_CHECK_SAT, for a problem of 0 or more than PDMPC_JOINT_MAX vehicles, and for a NULL out with vehicles to plan.
 * LDS holds one copy of every DISTINCT obstacle set of a problem: vehicles of a problem that hand over the same obstacles and
 * dynamic_obstacles arrays (same pointers, same counts) share one copy, and likewise vehicles with the same boundary arrays, so N
 * vehicles that see the scenario's sets need the room of one (PDMPC_ERR_CAPACITY only if the distinct sets of one problem do not fit). */
int pdmpc_plan_joint(pdmpc_handle* handle, int32_t n_problems, const int32_t* problem_offset, const pdmpc_vehicle_in* in,
                     pdmpc_vehicle_out* out);

/* ---- the unique prioritizations of a coupling graph (Prioritizer.unique_priorities, priority/Prioritizer.m:97-140) ----
 * adjacency: n x n, row-major, non-zero = coupled; only the strict upper triangle is read (triu(adjacency, 1)).  Edge e (0-based, in
 * the order of find(triu(adjacency, 1)): by column, then by row) runs row -> column unless it is flipped; orientation m (0 .. 2^E - 1)
 * flips edge e exactly when bit E - 1 - e of m is set (dec2bin(m, E)).  Out: the acyclic orientations in ascending m, masks[k] = m and
 * priorities[k * n + v] = position (1-based) of vehicle v in the orientation's lexicographically smallest topological order
 * (toposort(..., 'Order', 'stable')).  *n_out = K, the number of acyclic orientations, whatever max_out is (-1 for a graph outside
 * the limits).  PDMPC_ERR_CAPACITY without a launch for n > 64 or E > 32, and PDMPC_ERR_CAPACITY with nothing written for K > max_out:
 * the list is never truncated.  pdmpc_unique_priorities runs on the handle's device (csrc/priority_kernel.hip);
 * pdmpc_unique_priorities_host is its C++ twin and checker (csrc/step_priorities.hpp behind csrc/step_controller.cpp, no GPU needed). */
int pdmpc_unique_priorities(pdmpc_handle* handle, int32_t n, const uint8_t* adjacency, int64_t max_out, int64_t* n_out, uint32_t* masks,
                            int32_t* priorities);
int pdmpc_unique_priorities_host(int32_t n, const uint8_t* adjacency, int64_t max_out, int64_t* n_out, uint32_t* masks, int32_t* priorities);
/* ... of n_groups graphs in one call: graph g is adjacency[g], group_n[g] x group_n[g], with the rules above.
 * n_out[g] = K_g is always reported (-1 for a graph outside the limits n <= 64, E <= 32); masks holds the graphs' lists one after the
 * other (sum of K_g entries, ascending within a graph), priorities their K_g x group_n[g] rows one after the other: block g is bit for
 * bit what pdmpc_unique_priorities returns for graph g alone.  max_out[g] (only read) bounds K_g: if any K_g > max_out[g], or any graph is
 * outside the limits, the call returns PDMPC_ERR_CAPACITY, every count is reported and NOTHING is written.  PDMPC_ERR_INVALID for
 * n_groups < 1, a group_n[g] < 1, a max_out[g] < 0 and null arguments (masks / priorities may be NULL when every max_out[g] is 0).
 * On the device the orientations of all graphs are tested in one launch per pass, in tiles of 4096 orientations (a graph of E edges has
 * ceil(2^E / 4096) of them): a call whose graphs have 2^24 or more tiles together (sixteen graphs of 32 edges) returns
 * PDMPC_ERR_CAPACITY without a launch and with every count -1.  One staging copy and one read-back of the counts per call, whatever
 * n_groups is.  pdmpc_unique_priorities_grouped_host: the C++ twin and checker, the host enumeration graph by graph. */
int pdmpc_unique_priorities_grouped(pdmpc_handle* handle, int32_t n_groups, const int32_t* group_n, const uint8_t** adjacency, int64_t* max_out,
                                    int64_t* n_out, uint32_t* masks, int32_t* priorities);
int pdmpc_unique_priorities_grouped_host(int32_t n_groups, const int32_t* group_n, const uint8_t** adjacency, int64_t* max_out, int64_t* n_out,
                                         uint32_t* masks, int32_t* priorities);

/* ---- reachable sets (csrc/reachable_sets.cpp, csrc/reachable_kernel.hip) ----
 * pdmpc_local_reachable_sets: MotionPrimitiveAutomaton.local_reachable_sets_conv (reachability_analysis_offline_DP,
 * MotionPrimitiveAutomaton.m:394-647, convexified) of an automaton: polygon trim * Hp + k (0-based trim and k) is the convex hull
 * of what the trim reaches at step k + 1 from the origin, clockwise from its smallest-x (then smallest-y) vertex, open (first vertex
 * not repeated).  offset has n_trims * Hp + 1 entries and is always written; x and y (capacity entries each) only if the table fits,
 * PDMPC_ERR_CAPACITY otherwise (call with capacity 0 to size them). */
int pdmpc_local_reachable_sets(const pdmpc_mpa* mpa, int32_t capacity, int32_t* offset, double* x, double* y);
/* ReachableSetCoupler.couple (ReachableSetCoupler.m:5-56) on the step-Hp hulls of n vehicles at (x, y, yaw) in trim (1-based):
 * bounding-box pre-filter (boxes that only touch are not coupled), then coupled iff the overlap area exceeds 1e-3.  adjacency is
 * n x n bytes (symmetric, zero diagonal); area (n x n, or NULL) holds the area of every pair that passed the box test, 0 elsewhere.
 * cos_yaw / sin_yaw are the caller's cos(yaw) / sin(yaw): the sets move with the caller's libm. */
#define PDMPC_REACHABLE_MAX_COLS 256 /* vertices of one local hull the device coupler accepts (single_speed Hp 10: 146 at most) */
int pdmpc_upload_reachable_sets(pdmpc_handle* handle, int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* local_sets);
int pdmpc_reachable_set_coupling(pdmpc_handle* handle, int32_t n, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw,
                                 const int32_t* trim, uint8_t* adjacency, double* area);
int pdmpc_reachable_set_coupling_host(int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* local_sets, int32_t n, const double* x, const double* y,
                                      const double* cos_yaw, const double* sin_yaw, const int32_t* trim, uint8_t* adjacency, double* area);
/* kernel time (HIP events, ms) of the last pdmpc_reachable_set_coupling */
int pdmpc_reachable_set_coupling_kernel_ms(pdmpc_handle* handle, double* ms);
/* Lanelet bounding of the reachable sets (bound_reachable_sets.m, HighLevelController.m:241-246; the rules are in
 * include/pdmpc_geometry.h).  Vehicle v's sets at its pose (x, y, yaw, 1-based trim, as for the coupler) are
 * intersected with lanelet_polygons polygon v: its raw predicted-lanelet polygon (left boundary, then the reversed right boundary;
 * 0 vertices: not bounded).  all_steps != 0: sets of steps 1 .. Hp, polygon v * Hp + k; all_steps == 0: step Hp only, polygon v.
 * Every result is closed (first vertex repeated).  offset (one entry more than polygons) is always written; out_x / out_y
 * (capacity entries each) and flags (PDMPC_BOUND_*, one per polygon, or NULL) only if the result fits, PDMPC_ERR_CAPACITY otherwise
 * (the offsets size a second call).  A lanelet polygon over PDMPC_LANELET_POLY_MAX_COLS vertices, or a bounded set over
 * PDMPC_BOUNDED_MAX_COLS (closing vertex included), is PDMPC_ERR_CAPACITY as well. */
#define PDMPC_LANELET_POLY_MAX_COLS 512
#define PDMPC_BOUNDED_MAX_COLS 1024
int pdmpc_bound_reachable_sets(pdmpc_handle* handle, int32_t n, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw,
                               const int32_t* trim, const pdmpc_polygon_set* lanelet_polygons, int32_t all_steps, int32_t capacity, int32_t* offset,
                               double* out_x, double* out_y, uint8_t* flags);
int pdmpc_bound_reachable_sets_host(int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* local_sets, int32_t n, const double* x, const double* y,
                                    const double* cos_yaw, const double* sin_yaw, const int32_t* trim, const pdmpc_polygon_set* lanelet_polygons,
                                    int32_t all_steps, int32_t capacity, int32_t* offset, double* out_x, double* out_y, uint8_t* flags);
/* ReachableSetCoupler.couple on the bounded step-Hp sets of the last successful pdmpc_bound_reachable_sets, on the device (the sets
 * never leave it): the box pre-filter, then the overlap area of two simple polygons (pdmpc_edge_overlap_term) for every pair that
 * passes it, coupled iff it exceeds 1e-3.  adjacency / area as for pdmpc_reachable_set_coupling. */
int pdmpc_bounded_set_coupling(pdmpc_handle* handle, uint8_t* adjacency, double* area);
/* ... its host twin for any n simple clockwise polygons (closed or open) */
int pdmpc_polygon_set_coupling_host(const pdmpc_polygon_set* sets, int32_t n, uint8_t* adjacency, double* area);
/* kernel times (HIP events, ms) of the last pdmpc_bound_reachable_sets and pdmpc_bounded_set_coupling: ms2[0] bounding, ms2[1] coupling */
int pdmpc_bounded_reachable_kernel_ms(pdmpc_handle* handle, double* ms2);
/* The two couplers for several independent sets of vehicles at once.  The N = group_offset[n_groups] vehicles handed
 * over are n_groups consecutive groups, group g = vehicles group_offset[g] .. group_offset[g + 1] - 1 (group_offset[0] = 0,
 * non-decreasing; empty groups are legal); pairs are formed inside a group only.  adjacency / area: block g is n_g x n_g, row-major, at
 * element offset sum_{h<g} n_h^2 (area may be NULL), and holds byte for byte what the ungrouped call returns for group g's vehicles alone.
 * A call is one staging copy, the pose pass, one pair pass, one copy back and one synchronisation whatever n_groups is.
 * pdmpc_bounded_set_coupling_grouped runs on the sets the last pdmpc_bound_reachable_sets left on the device: its groups cover exactly
 * that call's vehicles.  PDMPC_ERR_INVALID for n_groups < 0, decreasing offsets, or a call before the upload / the bounding;
 * PDMPC_ERR_CAPACITY for N > config.max_vehicles.  pdmpc_reachable_set_coupling_kernel_ms / pdmpc_bounded_reachable_kernel_ms report
 * the grouped call when it was the last one.  The host twins loop over the ungrouped host twins. */
int pdmpc_reachable_set_coupling_grouped(pdmpc_handle* handle, int32_t n_groups, const int32_t* group_offset, const double* x, const double* y,
                                         const double* cos_yaw, const double* sin_yaw, const int32_t* trim, uint8_t* adjacency, double* area);
int pdmpc_bounded_set_coupling_grouped(pdmpc_handle* handle, int32_t n_groups, const int32_t* group_offset, uint8_t* adjacency, double* area);
int pdmpc_reachable_set_coupling_grouped_host(int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* local_sets, int32_t n_groups, const int32_t* group_offset,
                                              const double* x, const double* y, const double* cos_yaw, const double* sin_yaw, const int32_t* trim,
                                              uint8_t* adjacency, double* area);
int pdmpc_polygon_set_coupling_grouped_host(const pdmpc_polygon_set* sets, int32_t n_groups, const int32_t* group_offset, uint8_t* adjacency, double* area);

/* ---- future collision assessment (FcaPrioritizer.m:11-92; csrc/fca.cpp, csrc/fca_kernel.hip) ----
 * Vehicle v's footprint at step k is the box [-1,-1,1,1]·(length/2 + offset), [-1,1,1,-1]·(width/2 + offset) rotated by
 * (cos_yaw, sin_yaw)[v * Hp + k] and moved to (x, y)[v * Hp + k], its reference point (calculate_yaw of the reference points, central
 * differences with one-sided ends, and its cos / sin are the caller's: the footprints are built from the caller's libm).  Counted
 * with intersect_sat (intersect_sat.m:1-42), per step k:
 *   every coupled pair (pairs[2 p], pairs[2 p + 1]) that meets counts once for each of its two vehicles;
 *   every vehicle v < n - 1 (the reference's outer loop stops at n - 1) counts once per static obstacle (obstacles, or NULL) and once
 *   per dynamic obstacle row r (polygon r * Hp + k of dynamic_rows, or NULL; n_polygons a multiple of Hp) that its footprint meets.
 * pairs: n_pairs coupled pairs a < b, ascending by (a, b), no repeats.  Out: collisions[n], and priorities[n] = the index vector
 * (1-based) of a stable descending sort of the counts — what the reference passes to directed_coupling_from_priorities as it is.
 * PDMPC_ERR_INVALID for n < 1, Hp < 2 (the yaw needs two points), a malformed pair list or an empty polygon.
 * pdmpc_fca_collisions runs on the handle's device (buffers kept on the handle: one copy in, one copy out); pdmpc_fca_collisions_host
 * is its C++ twin and checker (no GPU needed).  The counts are integers: both give the same counts in any order of the tests. */
int pdmpc_fca_collisions(pdmpc_handle* handle, int32_t n, int32_t Hp, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw,
                         int32_t n_pairs, const int32_t* pairs, const pdmpc_polygon_set* obstacles, const pdmpc_polygon_set* dynamic_rows, double length,
                         double width, double offset, int32_t* collisions, int32_t* priorities);
int pdmpc_fca_collisions_host(int32_t n, int32_t Hp, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw, int32_t n_pairs,
                              const int32_t* pairs, const pdmpc_polygon_set* obstacles, const pdmpc_polygon_set* dynamic_rows, double length, double width,
                              double offset, int32_t* collisions, int32_t* priorities);
/* kernel time (HIP events, ms) of the last pdmpc_fca_collisions or pdmpc_fca_collisions_grouped */
int pdmpc_fca_kernel_ms(pdmpc_handle* handle, double* ms);
/* The assessment for several independent sets of vehicles at once: n_groups consecutive groups, each with its own
 * coupled pairs (numbered inside the group), static obstacles, dynamic rows and vehicle sizes.  x, y, cos_yaw, sin_yaw hold the
 * N * Hp reference points of the N = sum n_g vehicles group after group; collisions and priorities (N each) stand group after group
 * too, priorities being every group's own 1-based index vector.  Group g's slices hold exactly what pdmpc_fca_collisions returns for
 * group g alone: nothing is counted across groups, and the last vehicle of every group skips its group's obstacles.  Groups with
 * n = 0 are legal and write nothing; so is n_groups = 0.  A call is one staging copy, the two kernel launches, one copy back and one
 * synchronisation whatever n_groups is; the host twin loops over pdmpc_fca_collisions_host.
 * PDMPC_ERR_INVALID for n_groups < 0, Hp < 2, a null array with N > 0 or a group that pdmpc_fca_collisions would refuse (the message
 * names the group); PDMPC_ERR_CAPACITY for N > config.max_vehicles. */
typedef struct pdmpc_fca_group {
    int32_t n, n_pairs;
    const int32_t* pairs;                  /* group-local, 0 <= a < b < n, ascending, no repeats */
    const pdmpc_polygon_set* obstacles;    /* or NULL */
    const pdmpc_polygon_set* dynamic_rows; /* or NULL; n_polygons a multiple of Hp */
    double length, width, offset;
} pdmpc_fca_group;
int pdmpc_fca_collisions_grouped(pdmpc_handle* handle, int32_t n_groups, const pdmpc_fca_group* groups, int32_t Hp, const double* x, const double* y,
                                 const double* cos_yaw, const double* sin_yaw, int32_t* collisions, int32_t* priorities);
int pdmpc_fca_collisions_grouped_host(int32_t n_groups, const pdmpc_fca_group* groups, int32_t Hp, const double* x, const double* y, const double* cos_yaw,
                                      const double* sin_yaw, int32_t* collisions, int32_t* priorities);

/* ---- human-driven vehicles (HighLevelController.update_hdv_traffic_info, HighLevelController.m:394-447; include/pdmpc_hdv.h, csrc/hdv.cpp,
 * csrc/hdv_kernel.hip) ----
 * What a search's third obstacle soup (pdmpc_vehicle_in.hdv_reachable_sets) is filled from: for every human-driven vehicle (HDV) the
 * lanelets closest to it, the chains (closest lanelet, successor) it may drive along, its reachable sets clipped to every chain, and
 * which controlled vehicles (CAVs) it is adjacent to.
 * The map: lanelet i (id i + 1) has the left points left_offset[i] .. left_offset[i + 1] - 1 and as many right points (at least one);
 * its centre line is 0.5 * (left + right).  succ_offset / succ_index: the successor ids (1-based) of every lanelet in the map's
 * order (succ_offset[0] = 0).  relationship: n_lanelets x n_lanelets bytes, read at (min id, max id): 0 none, 1 longitudinal, 2 side,
 * 3 merging, 4 forking, 5 crossing (LaneletRelationshipType.m).  hdv_local_sets: pdmpc_local_reachable_sets of the HDVs' automaton,
 * polygon trim * Hp + k.  A chain polygon (the boundary points of a lanelet and one successor) of more than
 * PDMPC_LANELET_POLY_MAX_COLS vertices, a local set of more than PDMPC_REACHABLE_MAX_COLS or a map of more than 1024 lanelets is
 * PDMPC_ERR_CAPACITY.
 * A traffic call, for n_hdv HDVs at (x, y, cos_yaw, sin_yaw: the caller's cos / sin) in trim (1-based) on the copy of the map moved by
 * (tile_dx, tile_dy), and n_cav CAVs at (cav_x, cav_y) on lanelet cav_lanelet (1-based) of the copy moved by (cav_tile_dx, cav_tile_dy):
 *   closest lanelets  map_position_to_closest_lanelets.m:1-25 at (x - tile_dx, y - tile_dy), literally: in id order a lanelet whose
 *                     distance is below the best so far starts the list anew, one within 0.1 of the best so far is appended.
 *                     closest_offset[n_hdv + 1], closest_index (ids, room for n_hdv * PDMPC_HDV_MAX_CHAINS).
 *   rows              one per (HDV, chain), HDV by HDV; a chain is (closest lanelet, one of its successors) in list and successor
 *                     order, or the lanelet alone if it has no successor.  *n_rows, row_hdv[row] (room for n_hdv * PDMPC_HDV_MAX_CHAINS).
 *   reachable lanes   polygon row * Hp + k = the HDV's step-(k + 1) set K at its pose intersected with the row's chain polygon (left
 *                     points of both lanelets, then their right points reversed, moved by the tile offset) by the rule of
 *                     pdmpc_bound_reachable_sets, closed; an empty intersection is a polygon of 0 vertices (flag PDMPC_BOUND_RESTORED).
 *                     set_offset (room for n_hdv * PDMPC_HDV_MAX_CHAINS * Hp + 1) is always written; set_x / set_y (capacity entries
 *                     each) and set_flags (one per polygon, or NULL) only if the lanes fit: PDMPC_ERR_CAPACITY otherwise, and the
 *                     offsets size a second call.  This is the layout of pdmpc_vehicle_in.hdv_reachable_sets.
 *   adjacency         n_cav x n_hdv bytes: 1 unless the HDV is behind the CAV (is_hdv_behind.m:13-92 with the CAV's own position;
 *                     no predecessor lanelet found means "not on one"), 0 for a CAV on another copy of the map.
 * Lists, rows, offsets and adjacency are written whenever the call gets that far: also when the capacity is too small.  An HDV with
 * more than PDMPC_HDV_MAX_CHAINS closest lanelets or chains is PDMPC_ERR_CAPACITY with *n_rows = -1 and nothing else promised;
 * PDMPC_ERR_INVALID for a call before the upload, a trim or lanelet id out of range, n < 0, Hp > PDMPC_HP_MAX or a null array that is
 * needed; PDMPC_ERR_CAPACITY for more than 64 HDVs or 2^20 CAVs in one call (both twins; config.max_vehicles is not read):
 * the device keeps 16 x Hp slots of PDMPC_BOUNDED_MAX_COLS vertices per HDV, 256 KB x Hp, allocated on the first call that needs them.
 * pdmpc_hdv_traffic runs on the handle's device: one staging copy, four launches, one copy back, one synchronisation.  The copy back
 * moves the room for `capacity` vertices (at most what the slots can hold), not the result's size, which the host learns only from it:
 * give the call the room the result needs -- the last step's total and some slack, or the exact total of a sizing call -- not a
 * generous buffer (2 HDVs at Hp 8 with unlimited room copy back 4 MB per call).  pdmpc_hdv_traffic_host is its C++ twin and checker with the map and the sets as arguments (no GPU needed);
 * both give the same bits.  pdmpc_hdv_lanelet_distances_host: the distance of (px, py) to every lanelet's centre line, distance[n_lanelets]. */
#define PDMPC_HDV_MAX_CHAINS 16
int pdmpc_upload_hdv_map(pdmpc_handle* handle, int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x,
                         const double* left_y, const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index,
                         const uint8_t* relationship, int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* hdv_local_sets);
int pdmpc_hdv_traffic(pdmpc_handle* handle, int32_t n_hdv, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw, const int32_t* trim,
                      const double* tile_dx, const double* tile_dy, int32_t n_cav, const double* cav_x, const double* cav_y, const int32_t* cav_lanelet,
                      const double* cav_tile_dx, const double* cav_tile_dy, int32_t* closest_offset, int32_t* closest_index, int32_t capacity, int32_t* n_rows,
                      int32_t* row_hdv, int32_t* set_offset, double* set_x, double* set_y, uint8_t* set_flags, uint8_t* adjacency);
int pdmpc_hdv_traffic_host(int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y,
                           const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship,
                           int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* hdv_local_sets, int32_t n_hdv, const double* x, const double* y,
                           const double* cos_yaw, const double* sin_yaw, const int32_t* trim, const double* tile_dx, const double* tile_dy, int32_t n_cav,
                           const double* cav_x, const double* cav_y, const int32_t* cav_lanelet, const double* cav_tile_dx, const double* cav_tile_dy,
                           int32_t* closest_offset, int32_t* closest_index, int32_t capacity, int32_t* n_rows, int32_t* row_hdv, int32_t* set_offset, double* set_x,
                           double* set_y, uint8_t* set_flags, uint8_t* adjacency);
int pdmpc_hdv_lanelet_distances_host(int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y,
                                     const double* right_x, const double* right_y, double px, double py, double* distance);
/* kernel time (HIP events, ms) of the last pdmpc_hdv_traffic (its four launches), pdmpc_hdv_traffic_grouped (its five),
 * pdmpc_hdv_drive_grouped (its one) or pdmpc_hdv_drive_traffic_grouped (its six), whichever was called last */
int pdmpc_hdv_kernel_ms(pdmpc_handle* handle, double* ms);

/* Several maps on a handle, and several independent sets of HDVs and CAVs in one call.
 * A handle has PDMPC_HDV_MAP_SLOTS map slots, each with its own map and HDV automaton hulls.  pdmpc_upload_hdv_map_slot fills one
 * (pdmpc_upload_hdv_map is slot 0, which pdmpc_hdv_traffic reads); PDMPC_ERR_INVALID for a slot out of range.  Every successful upload
 * gives its slot a new generation number, larger than any before it (0: never uploaded; a failed upload leaves the slot empty with
 * generation 0); pdmpc_hdv_map_slot_state reports it, the uploads into all slots of the handle so far, and the Hp of the hulls the slot holds
 * (0: empty; any of the three may be NULL).
 * pdmpc_hdv_map_slot_holds: *holds = 1 if the slot holds exactly this map and these hulls -- the arguments compared byte for byte with
 * the handle's host copy of what was uploaded, no hash --, else 0.  pdmpc_hdv_check_map_host: the checks of an upload alone (host only; pdmpc_last_error has the reason of a refusal).
 *
 * pdmpc_hdv_traffic_grouped: group g has the HDVs hdv_offset[g] .. hdv_offset[g + 1] - 1 and the CAVs cav_offset[g] .. of the call's
 * arrays (offsets [n_groups + 1], from 0, non-decreasing) and drives on the map of slot group_slot[g].  Its slices of the outputs hold
 * byte for byte what pdmpc_hdv_traffic returns for the group alone on a handle whose slot 0 holds that map: HDV indices (row_hdv) and
 * vertex offsets (set_offset, from 0) are the group's own, nothing is computed across groups, a CAV meets the HDVs of its group only.
 * With h0 = hdv_offset[g] the group's blocks start at: closest_offset (n_g + 1 entries) h0 + g; closest_index and row_hdv
 * h0 * PDMPC_HDV_MAX_CHAINS; set_offset (n_rows[g] * Hp + 1 entries) h0 * PDMPC_HDV_MAX_CHAINS * Hp + g; set_flags
 * h0 * PDMPC_HDV_MAX_CHAINS * Hp; set_x / set_y set_base[g] (set_base[n_groups]: all vertices); adjacency (n_cav_g x n_hdv_g) the sum
 * of n_cav_h * n_hdv_h over h < g.  pdmpc_hdv_grouped_layout_host (host only) is the one statement of these starts: arrays of
 * n_groups + 1 entries, the last the room the array needs; any may be NULL.  Groups without HDVs or CAVs (they write what has a size:
 * an offset entry 0, n_rows[g] = 0), n_groups = 0, several groups on one slot and any slot order are fine.
 * capacity is the room for the vertices of all groups together: too small is PDMPC_ERR_CAPACITY with every list, row, offset, set_base
 * entry and adjacency byte written (the totals size a second call), and no more than the room for capacity vertices is copied back.
 * PDMPC_ERR_INVALID: n_groups < 0, decreasing offsets, a slot out of range or never uploaded, slots in use whose Hp differ, a null array
 * that is needed, a trim or lanelet id out of range for the group's map (pdmpc_last_error names the group).  PDMPC_ERR_CAPACITY: more than
 * PDMPC_HDV_MAX_VEHICLES (64) HDVs or PDMPC_HDV_MAX_CAVS (2^20) CAVs in a group, more than PDMPC_HDV_GROUPED_MAX_VEHICLES in the call (the slots of the lane pass are
 * 256 KB x Hp per HDV: 512 MB at the limit and Hp 16; they are grown to what a call needs), 2^31 or more (CAV, HDV) pairs; an HDV whose
 * lists run over makes n_rows[g] = -1 for its group, whose other blocks then hold nothing, while the other groups' results are written.
 * One staging copy, FIVE launches whatever n_groups is (closest, lane, scan, copy, adjacency), one copy back, one synchronisation.
 * There is no grouped host twin: a reference is pdmpc_hdv_traffic_host called for every group. */
#define PDMPC_HDV_MAP_SLOTS 8
#define PDMPC_HDV_GROUPED_MAX_VEHICLES 128
int pdmpc_upload_hdv_map_slot(pdmpc_handle* handle, int32_t slot, int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x,
                              const double* left_y, const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index,
                              const uint8_t* relationship, int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* hdv_local_sets);
int pdmpc_hdv_map_slot_state(pdmpc_handle* handle, int32_t slot, int64_t* generation, int64_t* uploads, int32_t* Hp);
int pdmpc_hdv_map_slot_holds(pdmpc_handle* handle, int32_t slot, int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x,
                             const double* left_y, const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index,
                             const uint8_t* relationship, int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* hdv_local_sets, int32_t* holds);
int pdmpc_hdv_check_map_host(int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y,
                             const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship,
                             int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* hdv_local_sets);
int pdmpc_hdv_grouped_layout_host(int32_t n_groups, const int32_t* hdv_offset, const int32_t* cav_offset, int32_t Hp, int32_t* closest_at, int32_t* list_at,
                                  int32_t* set_offset_at, int32_t* set_at, int64_t* adjacency_at);
int pdmpc_hdv_traffic_grouped(pdmpc_handle* handle, int32_t n_groups, const int32_t* group_slot, const int32_t* hdv_offset, const int32_t* cav_offset, const double* x,
                              const double* y, const double* cos_yaw, const double* sin_yaw, const int32_t* trim, const double* tile_dx, const double* tile_dy,
                              const double* cav_x, const double* cav_y, const int32_t* cav_lanelet, const double* cav_tile_dx, const double* cav_tile_dy,
                              int32_t* closest_offset, int32_t* closest_index, int32_t capacity, int32_t* n_rows, int32_t* row_hdv, int32_t* set_offset,
                              int32_t* set_base, double* set_x, double* set_y, uint8_t* set_flags, uint8_t* adjacency);

/* Simulated human drivers (include/pdmpc_hdv.h: "the driver model"; csrc/hdv_drive_host.hpp).  An HDV follows a route --
 * route_lanelet[route_offset[h] .. route_offset[h + 1]): 1 .. PDMPC_HDV_ROUTE_MAX 1-based lanelet ids, each a successor of the one
 * before it, on a route with closed[h] != 0 the first of the last too -- along the centre lines of its lanelets, and keeps a gap to the
 * nearest vehicle ahead on the route: speed = min(v_des, max(0, (gap - gap_min) / headway)).  Its state is (r, j, u): u metres along
 * segment j of route position r; state_seg holds r of every HDV of the call, then j of every HDV.  parameters[4] = look_ahead, gap_min,
 * headway, lateral (PDMPC_HDV_*_DEFAULT of pdmpc_hdv.h).  One step of length dt: the gap is the smallest distance ahead, along the route
 * within look_ahead (at most PDMPC_HDV_WINDOW_MAX segments), of a CAV (cav_x, cav_y) or of another HDV of the call at its pose BEFORE the
 * step that lies within `lateral` of the route on the same map copy (equal tile_dx / tile_dy), +inf if there is none; then all HDVs
 * move at once by speed * dt (the end of an open route stops an HDV there with speed 0).  Outputs: the new state, the pose (x, y and
 * cos_yaw / sin_yaw = the direction of the segment it stands on: no libm), speed and gap.
 * pdmpc_hdv_route_check_host: the route checks alone.  pdmpc_hdv_place_host: the state and pose start_distance[h] metres from the start
 * of every route (the walk of the step).  pdmpc_hdv_drive_host: one step of the HDVs and CAVs of one member, no GPU.
 * pdmpc_hdv_drive_grouped: the same step for the groups of pdmpc_hdv_traffic_grouped (parameters [4 n_groups], dt [n_groups]) on the
 * handle's device, group g on the map of slot group_slot[g]: one staging copy, ONE launch (a wavefront per HDV), one copy back, one
 * synchronisation; per group the bits of pdmpc_hdv_drive_host.  pdmpc_hdv_drive_traffic_grouped: that launch followed by the five of
 * pdmpc_hdv_traffic_grouped, which read the poses it left on the device -- one staging copy, SIX launches whatever n_groups is, one copy
 * back, one synchronisation.  Group g drives if drives[g] != 0: its x, y, cos_yaw, sin_yaw entries are outputs, like new_seg, new_u,
 * speed and gap; a group with drives[g] == 0 needs no routes (route_offset does not move over its HDVs), leaves those entries alone
 * and is exactly pdmpc_hdv_traffic_grouped's group.  The traffic outputs are pdmpc_hdv_traffic_grouped's.
 * PDMPC_ERR_INVALID (pdmpc_last_error names the group, the HDV and the route position): a route that is empty, too long, leaves the
 * map, steps to a non-successor or has no segment of positive length; a state that is not on its route; a parameter or dt that is not
 * positive and finite; headway < dt (with headway >= dt an HDV closes at most gap - gap_min per step); a negative v_des; a start distance
 * that is negative or at or beyond the end of an open route.  A refused call has launched nothing. */
int pdmpc_hdv_route_check_host(int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y,
                               const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship,
                               int32_t n_hdv, const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed);
int pdmpc_hdv_place_host(int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y, const double* right_x,
                         const double* right_y, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship, int32_t n_hdv,
                         const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const double* start_distance, const double* tile_dx,
                         const double* tile_dy, int32_t* state_seg, double* state_u, double* x, double* y, double* cos_yaw, double* sin_yaw);
int pdmpc_hdv_drive_host(int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y, const double* right_x,
                         const double* right_y, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship, int32_t n_hdv,
                         const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const int32_t* state_seg, const double* state_u,
                         const double* tile_dx, const double* tile_dy, const double* v_des, int32_t n_cav, const double* cav_x, const double* cav_y,
                         const double* cav_tile_dx, const double* cav_tile_dy, const double* parameters, double dt, int32_t* new_seg, double* new_u, double* x, double* y,
                         double* cos_yaw, double* sin_yaw, double* speed, double* gap);
int pdmpc_hdv_drive_grouped(pdmpc_handle* handle, int32_t n_groups, const int32_t* group_slot, const int32_t* hdv_offset, const int32_t* cav_offset,
                            const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const int32_t* state_seg, const double* state_u,
                            const double* tile_dx, const double* tile_dy, const double* v_des, const double* cav_x, const double* cav_y, const double* cav_tile_dx,
                            const double* cav_tile_dy, const double* parameters, const double* dt, int32_t* new_seg, double* new_u, double* x, double* y,
                            double* cos_yaw, double* sin_yaw, double* speed, double* gap);
int pdmpc_hdv_drive_traffic_grouped(pdmpc_handle* handle, int32_t n_groups, const int32_t* group_slot, const int32_t* hdv_offset, const int32_t* cav_offset,
                                    const uint8_t* drives, const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const int32_t* state_seg,
                                    const double* state_u, const double* v_des, const double* parameters, const double* dt, int32_t* new_seg, double* new_u,
                                    double* speed, double* gap, double* x, double* y, double* cos_yaw, double* sin_yaw, const int32_t* trim, const double* tile_dx,
                                    const double* tile_dy, const double* cav_x, const double* cav_y, const int32_t* cav_lanelet, const double* cav_tile_dx,
                                    const double* cav_tile_dy, int32_t* closest_offset, int32_t* closest_index, int32_t capacity, int32_t* n_rows, int32_t* row_hdv,
                                    int32_t* set_offset, int32_t* set_base, double* set_x, double* set_y, uint8_t* set_flags, uint8_t* adjacency);

/* ---- the caller's side of the boundary, natively (csrc/step_controller.cpp and its stages csrc/step_*.hpp) ----
 * One MPC time step of the prioritized sequential controller around pdmpc_plan_step, without any interpreter in the loop:
 * traffic info, coupling, priorities, grouping, computation levels, obstacle assembly, ONE launch, exhaustion handling,
 * fallbacks, plant update (HighLevelController.main_control_loop, hlc/controller/HighLevelController.m:334-373;
 * PrioritizedSequentialController.controller, hlc/controller/prioritized/PrioritizedSequentialController.m:77-94;
 * PrioritizedController.m:297-324,375-389,449-718; plant/Simulation.m:86-100).  p-dmpc_amd/pdmpc/controller.py is the same
 * logic in Python; the two build bit-identical step problems with every priority and weight strategy below.  FCA priorities run on
 * the device (pdmpc_fca_collisions) for a controller with a handle, on the host twin without one. */
enum { PDMPC_COUPLING_FULL = 0, PDMPC_COUPLING_DISTANCE = 1, PDMPC_COUPLING_NONE = 2 };          /* Coupler.m:31-32, DistanceCoupler.m:15-50 */
enum { PDMPC_COUPLING_REACHABLE_SET = 3 };                                                     /* ReachableSetCoupler.m:5-56 */
/* how a parallel predecessor (a higher-priority coupled vehicle whose coupling was cut into another computation level) enters a
 * vehicle's search (Config.isDealPredictionInconsistency, PrioritizedController.m:29-33): its previous plan shifted by one step
 * (parallel_coupling_previous_trajectory, :409-447) or its Hp reachable sets at its current pose (parallel_coupling_reachability,
 * :391-407) */
enum { PDMPC_PARALLEL_PREVIOUS_TRAJECTORY = 0, PDMPC_PARALLEL_REACHABLE_SETS = 1 };
/* ConstantPrioritizer.m, ColoringPrioritizer.m, RandomPrioritizer.m (a Fisher-Yates shuffle on mt19937ar doubles seeded with the time
 * step), FcaPrioritizer.m (pdmpc_fca_collisions on the step's reference points and the scenario's obstacles) */
enum { PDMPC_PRIORITY_CONSTANT = 0, PDMPC_PRIORITY_COLORING = 1, PDMPC_PRIORITY_RANDOM = 2, PDMPC_PRIORITY_FCA = 3 };
/* weight/DistanceWeigher.m, ConstantWeigher.m, RandomWeigher.m (one mt19937ar double per directed edge in find() order, seeded with
 * the time step) */
enum { PDMPC_WEIGHT_DISTANCE = 0, PDMPC_WEIGHT_CONSTANT = 1, PDMPC_WEIGHT_RANDOM = 2 };
enum { PDMPC_SUCCESSOR_NONE = 0, PDMPC_SUCCESSOR_AREA_OF_STANDSTILL = 1, PDMPC_SUCCESSOR_AREA_OF_PREVIOUS_TRAJECTORY = 2 }; /* ConstraintFromSuccessor.m */

typedef struct {
    int32_t Hp;                        /* options.Hp */
    int32_t coupling;                  /* PDMPC_COUPLING_* */
    int32_t priority_strategy;         /* PDMPC_PRIORITY_* */
    int32_t weight_strategy;           /* PDMPC_WEIGHT_* (only matters when the coupling DAG is deeper than max_num_CLs) */
    int32_t max_num_CLs;               /* options.max_num_CLs (Config.m:28) */
    int32_t constraint_from_successor; /* PDMPC_SUCCESSOR_* (Config.m:37) */
    double dt_seconds;                 /* options.dt_seconds */
    double offset;                     /* options.offset (Config.m:49) */
    double vehicle_length, vehicle_width; /* scenarios/Vehicle.m:10-11 */
} pdmpc_controller_config;

/* The scenario fields the controller reads (scenarios/Scenario.m, Vehicle.m) plus the trims' speed / steering
 * (MotionPrimitiveAutomaton.trims) and the per-lanelet boundaries of the map (RoadDataCommonRoad.get_lanelet_boundary). */
typedef struct {
    int32_t n_vehicles;
    const double *x_start, *y_start, *yaw_start, *reference_speed; /* [n_vehicles] */
    const int32_t* path_offset;      /* [n_vehicles + 1]: reference path of vehicle v = points path_offset[v] .. path_offset[v+1]-1 */
    const double *path_x, *path_y;
    const int32_t* lanelets_offset;  /* [n_vehicles + 1] or NULL (no lanelets: circle scenario) */
    const int32_t* lanelets_index;   /* 1-based lanelet ids along the vehicle's loop (Vehicle.lanelets_index) */
    const int32_t* points_index;     /* same offsets: 1-based index of the last path point of each of those lanelets */
    const int32_t* is_loop;          /* [n_vehicles] or NULL */
    const double *tile_dx, *tile_dy; /* [n_vehicles] or NULL: translation of the vehicle's copy of the map */
    int32_t n_lanelets;
    const int32_t *left_offset, *right_offset; /* [n_lanelets + 1] */
    const double *left_x, *left_y, *right_x, *right_y;
    pdmpc_polygon_set obstacles;     /* scenario.obstacles */
    int32_t n_trims;
    const double *trim_speed, *trim_steering; /* [n_trims] */
} pdmpc_scenario;

typedef struct pdmpc_controller pdmpc_controller;

/* handle may be NULL for a controller that only builds step problems / applies given records (tests without a GPU) */
int pdmpc_controller_create(pdmpc_handle* handle, const pdmpc_controller_config* cfg, const pdmpc_scenario* scenario, pdmpc_controller** out);
int pdmpc_controller_destroy(pdmpc_controller* c);
/* one whole time step: build the step problem, plan it with ONE launch (pdmpc_plan_step), apply the result */
int pdmpc_controller_step(pdmpc_controller* c);
/* Human-driven vehicles in the controller's steps (HighLevelController.update_hdv_traffic_info).  set_hdvs: n_hdv HDVs
 * from now on, on the map of the controller's scenario (its per-lanelet left / right points) with the lanelet graph given here
 * (succ_offset / succ_index / relationship as for pdmpc_upload_hdv_map), hdv_mpa their own automaton (the reference: single_speed
 * without the recursive-feasibility mask; its Hp the controller's), tile_dx / tile_dy [n_hdv] (or NULL: 0) the map copy each drives on.
 * set_hdv_measurements: their measured poses [n_hdv], kept until set again.  Every built step (build_step, explore_build,
 * optimal_build, and so every *_step and *_run) then takes part in ONE pdmpc_hdv_traffic_grouped call on the handle (a group's rank 0)
 * -- a group of its own in it; the members of a sweep are the groups of one call, pdmpc_sweep_last_hdv_calls; its map stays in the
 * map slot of the handle it was found in or uploaded to --, the host twin without a handle, with trim 1 for every HDV and the CAVs'
 * measured positions and current lanelets,
 * and every search receives the rows of the HDVs adjacent to its vehicle, the same in every prioritization; the call's time counts into
 * ms6[0].  hdv_info: lists, rows, sets and adjacency of the last built step (pointers into the controller, valid until the next build;
 * any may be NULL).  PDMPC_ERR_INVALID: a scenario without lanelets, a handle with the separating-axis checker (the HDV soup is
 * InterX's), a step before the first measurement, pdmpc_controller_centralized_build with HDVs set (the joint search has no HDV check). */
int pdmpc_controller_set_hdvs(pdmpc_controller* c, int32_t n_hdv, const pdmpc_mpa* hdv_mpa, const int32_t* succ_offset, const int32_t* succ_index,
                              const uint8_t* relationship, const double* tile_dx, const double* tile_dy);
int pdmpc_controller_set_hdv_measurements(pdmpc_controller* c, const double* x, const double* y, const double* yaw);
/* HDVs that move themselves (DESIGN.md 3.24 "Drivers").  set_hdv_drivers, after set_hdvs: HDV q follows the route route_lanelet[route_offset[q] ..
 * route_offset[q + 1]) (closed[q] != 0: round and round) at up to v_des[q] with params[4] = look_ahead, gap_min, headway, lateral, from
 * start_distance[q] metres along it; the routes are checked against the controller's map, dt is the controller's dt_seconds.  The
 * placement is the measurement of the first built step; at every later built step (build_step, explore_build, optimal_build, every sweep
 * build, on a group through rank 0's handle) the traffic stage first moves the HDVs one driver step against the CAVs' measured positions:
 * with a handle ONE pdmpc_hdv_drive_traffic_grouped in the stage's batches and map slots (it counts as one call in
 * pdmpc_sweep_last_hdv_calls), without one pdmpc_hdv_drive_host, then pdmpc_hdv_traffic_host, per member.  hdv_driver_state: state
 * (r of every HDV, then j; u), pose (yaw = atan2(sin, cos), for read-back only), speed and gap of the last built step (speed 0 and gap
 * +inf at the placement); any may be NULL.  set_hdv_recording: T rows of n_hdv recorded poses (row t at [t * n_hdv]); built step s (from
 * 1) takes row min(s, T) - 1, with the cosines and sines set_hdv_measurements takes.  set_hdv_poses: measurements given as directions
 * (cos_yaw, sin_yaw as they are, no libm): what a caller that drives the HDVs itself with pdmpc_hdv_drive_host hands over.
 * PDMPC_ERR_INVALID: before set_hdvs; drivers and a recording exclude each other, and set_hdv_measurements / set_hdv_poses are refused
 * with either (the message says why); a bad route (the HDV and the position are named), headway < dt, a start distance at or beyond
 * the end of an open route. */
int pdmpc_controller_set_hdv_drivers(pdmpc_controller* c, const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const double* start_distance,
                                     const double* v_des, const double* params);
int pdmpc_controller_hdv_driver_state(pdmpc_controller* c, int32_t* state_seg, double* state_u, double* x, double* y, double* yaw, double* speed, double* gap);
int pdmpc_controller_set_hdv_recording(pdmpc_controller* c, int32_t T, const double* x, const double* y, const double* yaw);
int pdmpc_controller_set_hdv_poses(pdmpc_controller* c, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw);
int pdmpc_controller_hdv_info(pdmpc_controller* c, int32_t* n_hdv, const int32_t** closest_offset, const int32_t** closest_index, int32_t* n_rows,
                              const int32_t** row_hdv, const int32_t** set_offset, const double** set_x, const double** set_y, const uint8_t** set_flags,
                              const uint8_t** adjacency);
/* n_steps closed-loop time steps in one call; ms[i] (may be NULL) = wall-clock milliseconds of step i */
int pdmpc_controller_run(pdmpc_controller* c, int32_t n_steps, double* ms);
/* the two host halves on their own: build_step advances the time step counter and leaves the problem readable with
 * pdmpc_controller_problem; apply takes the records of that problem in slot order */
int pdmpc_controller_build_step(pdmpc_controller* c);
int pdmpc_controller_apply(pdmpc_controller* c, const pdmpc_vehicle_out* records);
/* the problem of the last build_step exactly as pdmpc_plan_step receives it (pointers stay valid until the next build_step);
 * order[s] = vehicle (0-based) in slot s, levels[v] = computation level (1-based) of vehicle v */
int pdmpc_controller_problem(pdmpc_controller* c, int32_t* n, const pdmpc_vehicle_in** in, const int32_t** pred_offset, const int32_t** pred_index,
                             const pdmpc_polygon_set** fallback, const int32_t** order, const int32_t** levels);
/* plant state after the last apply (PlantMeasurement), per vehicle; any pointer may be NULL */
int pdmpc_controller_state(pdmpc_controller* c, double* x, double* y, double* yaw, double* speed, double* steering, int32_t* needs_fallback,
                           int32_t* time_step);
const pdmpc_vehicle_out* pdmpc_controller_records(pdmpc_controller* c); /* records of the last pdmpc_controller_step, slot order */
/* The explorative controller's permutations of the computation levels (PrioritizedExplorativeController.m:241-309): n_perm x
 * n_levels, row-major, drawn from RandStream("mt19937ar", Seed = seed) / randi as the reference draws them (:249, :283-286);
 * rows beyond n_levels (the reference stops there) are shuffles from the same stream.  Twin of pdmpc.explorative. */
int pdmpc_exploration_permutations(int32_t n_levels, int32_t n_perm, uint32_t seed, int32_t* out);
/* The explorative time step (PrioritizedExplorativeController.m:25-176): the step's traffic state under n_perm
 * prioritizations — instance 0 the controller's own, instance p the computation levels permuted by row p of the table above —
 * flattened into one batch whose slots are ordered by (level, instance).  explore_build advances the time step like build_step and
 * leaves the batch readable with explore_problem (instance / vehicle / level per slot); explore_choose takes the batch's records:
 * per weakly connected sub-graph the instance with the smallest summed cost-to-come of the final nodes after round(., 8)
 * (:94-176), chosen[v] = the instance vehicle v goes on with, cost = n_perm x n_graphs; explore_step = build + ONE launch +
 * choose + apply of the chosen plans (seed = time step, :249); explore_run = n_steps of them, ms[i] = wall-clock of step i. */
int pdmpc_controller_explore_build(pdmpc_controller* c, int32_t n_perm, uint32_t seed);
int pdmpc_controller_explore_problem(pdmpc_controller* c, int32_t* n_slots, const pdmpc_vehicle_in** in, const int32_t** pred_offset, const int32_t** pred_index,
                                     const pdmpc_polygon_set** fallback, const int32_t** instance, const int32_t** vehicle, const int32_t** level);
int pdmpc_controller_explore_choose(pdmpc_controller* c, const pdmpc_vehicle_out* records, int32_t* chosen, int32_t* n_graphs, double* cost);
int pdmpc_controller_explore_step(pdmpc_controller* c, int32_t n_perm);
int pdmpc_controller_explore_run(pdmpc_controller* c, int32_t n_perm, int32_t n_steps, double* ms);
/* measurement only: on != 0 makes the explorative step build, plan and choose as always but APPLY the plans of the controller's own
 * prioritization, so that the traffic follows pdmpc_controller_step's closed loop (bench.py: the host-inclusive rate on the same steps
 * as the resident replay) */
int pdmpc_controller_explore_follow_own(pdmpc_controller* c, int32_t on);
int pdmpc_controller_explore_result(pdmpc_controller* c, int32_t* chosen, int32_t* n_graphs, const double** cost, const pdmpc_vehicle_out** records);
/* The optimal-priority time step (PrioritizedOptimalController.m:25-114, PrioritizedOptimalSequentialController.m): the step's traffic
 * state under EVERY unique prioritization of its coupling graph (pdmpc_unique_priorities_grouped with one graph on the controller's
 * device; the host twin for a controller without a handle), flattened into one batch whose slots are ordered by (level, instance, slot).  Instance p plans with
 * constant priorities = prioritization p, grouped as the controller groups (max_num_CLs); instance 0 (mask 0) is the problem
 * pdmpc_controller_build_step builds with constant priorities.  optimal_build advances the time step like build_step and leaves the
 * batch readable with pdmpc_controller_explore_problem; PDMPC_ERR_CAPACITY if more than max_instances prioritizations exist (and for
 * the limits of pdmpc_unique_priorities).  optimal_choose: for every vehicle v the instance with the smallest sum over ALL vehicles
 * of the cost-to-come of their final nodes (v's own first, then the others by index), round(., 8), the first minimum (:56-114); an
 * exhausted search makes its instance infinitely expensive.  chosen[v]; cost (may be NULL) = n x K, row v = vehicle v's sums.  Every
 * vehicle goes on with the couplings of its chosen instance.  optimal_step = build + ONE launch + choose + apply; optimal_run =
 * n_steps of them reading back status and final cost of every plan and the chosen records only; optimal_result: chosen instance per
 * vehicle, K, the cost table and (after optimal_step) the batch's records. */
int pdmpc_controller_optimal_build(pdmpc_controller* c, int32_t max_instances);
int pdmpc_controller_optimal_choose(pdmpc_controller* c, const pdmpc_vehicle_out* records, int32_t* chosen, double* cost);
int pdmpc_controller_optimal_step(pdmpc_controller* c, int32_t max_instances);
int pdmpc_controller_optimal_run(pdmpc_controller* c, int32_t max_instances, int32_t n_steps, double* ms);
int pdmpc_controller_optimal_result(pdmpc_controller* c, int32_t* chosen, int32_t* n_instances, const double** cost, const pdmpc_vehicle_out** records);
/* host wall-clock milliseconds of the last pdmpc_controller_step / pdmpc_controller_explore_step, by part: [0] build the step problem(s)
 * on the host (FCA priorities included, on the device or not), [1] pack, [2] enqueue, [3] wait + read-back, [4] choice among the
 * prioritizations (explorative step), [5] apply */
int pdmpc_controller_last_timing(pdmpc_controller* c, double* ms6);
/* ... and summed over the steps since the last call with reset != 0 (n_steps: how many) */
int pdmpc_controller_timing_sum(pdmpc_controller* c, double* ms6, int64_t* n_steps, int32_t reset);
const char* pdmpc_controller_last_error(void);
/* The reachable-set features of the controller.  pdmpc_controller_set_reachability computes the automaton's local
 * reachable sets (pdmpc_local_reachable_sets) and, for a controller with a handle, uploads them (pdmpc_upload_reachable_sets); a step
 * with PDMPC_COUPLING_REACHABLE_SET or PDMPC_PARALLEL_REACHABLE_SETS but without them returns PDMPC_ERR_INVALID.  With a handle the
 * coupling runs on the device (pdmpc_reachable_set_coupling), without one on the host twin (pdmpc_reachable_set_coupling_host). */
int pdmpc_controller_set_reachability(pdmpc_controller* c, const pdmpc_mpa* mpa);
int pdmpc_controller_set_parallel_coupling(pdmpc_controller* c, int32_t mode); /* PDMPC_PARALLEL_*, default PREVIOUS_TRAJECTORY */
/* on != 0: the reachable sets a step computes (for PDMPC_COUPLING_REACHABLE_SET or PDMPC_PARALLEL_REACHABLE_SETS) are bounded by every
 * vehicle's predicted lanelets (pdmpc_bound_reachable_sets on the device with a handle, its host twin without one) and the coupler
 * runs on the bounded step-Hp sets (pdmpc_bounded_set_coupling / pdmpc_polygon_set_coupling_host).  Vehicles without lanelets
 * (the circle scenario) are not bounded.  Default off. */
int pdmpc_controller_set_lanelet_bounding(pdmpc_controller* c, int32_t on);
/* The optimizer of the controller's steps (OptimizerType): the graph search (default) or the sampled optimizer
 * (MonteCarloTreeSearch.m, pdmpc_set_step_seeds + the plan calls).  pdmpc_controller_step / _run, _explore_step / _run and
 * _optimal_step / _run follow it.  The sampled optimizer's seeds are time_step + vehicle_index (1-based, MonteCarloTreeSearch.m:31-32,
 * PrioritizedController.m:335-341), the same for every instance of an explorative or optimal batch.  Its expansion budget is the
 * handle's (pdmpc_set_sampled_budget; on a group pdmpc_group_set_sampled_budget): the controller, its explorative and optimal steps
 * and sweeps plan on a handle and so follow the budget that handle has when the step is packed.  The same holds for its ensemble
 * size (pdmpc_set_sampled_ensemble; on a group pdmpc_group_set_sampled_ensemble): every vehicle of a step, an explorative or optimal
 * batch or a sweep is then planned by that many members and gets the winner's record. */
enum { PDMPC_OPTIMIZER_GRAPH_SEARCH = 0, PDMPC_OPTIMIZER_SAMPLED = 1 };
int pdmpc_controller_set_optimizer(pdmpc_controller* c, int32_t which); /* PDMPC_OPTIMIZER_*; anything else: PDMPC_ERR_INVALID */
/* the sampled optimizer's seed per slot of the last built step or batch (pdmpc_controller_build_step / _explore_build / _optimal_build),
 * whichever optimizer is selected: *n slots, *seeds valid until the next build */
int pdmpc_controller_seeds(pdmpc_controller* c, int32_t* n, const uint32_t** seeds);
/* The priorities of the last built step with constant, random or FCA priorities (1-based, what directed_coupling_from_priorities
 * received) and, after an FCA step, the collision counts behind them: pointers into the controller, valid until its next step; a
 * length of 0 where the strategy has none. */
int pdmpc_controller_priorities(pdmpc_controller* c, int32_t* n_priorities, const int32_t** priorities, int32_t* n_collisions, const int32_t** collisions);
/* on != 0: pdmpc_controller_explore_run and pdmpc_controller_optimal_run (the steps that keep the chosen plans only) make ONE
 * pdmpc_plan_step_chosen call per step -- the choice among the prioritizations and the gather of the chosen records run on the device
 * directly behind the search, one read-back -- instead of pdmpc_plan_step_lean, the choice on the host and pdmpc_fetch_records_at.  The
 * explorative step with and without follow-own and the optimal-priority step; state, chosen instances, cost table and kept records are
 * the same byte for byte.  Default off; nothing changes for a controller without a handle. */
int pdmpc_controller_set_device_choice(pdmpc_controller* c, int32_t on);
/* Centralized control natively (CentralizedController.m:33-59; the twin is pdmpc.centralized.CentralizedController; csrc/step_centralized.hpp;
 * DESIGN.md §3.15): one joint graph search over all vehicles of the controller per time step, no coupling, no priorities, no levels.
 * centralized_build advances the time step and runs the traffic info of a step (trim from the measurement, reference sampling,
 * predicted lanelet boundaries); centralized_problem hands out the joint problem: *n = the vehicle count, in[v] = vehicle v (vehicle
 * order), every entry's obstacles the scenario's set UNDER THE SAME POINTERS (pdmpc_plan_joint stages it once), dynamic_obstacles and
 * hdv_reachable_sets empty; valid until the next build.  centralized_apply takes the n records in vehicle order and is Simulation.apply
 * (Simulation.m:86-100): pose = y_predicted(:, 1), speed and steering those of predicted_trims(1); no fallbacks, no previous plans.
 * centralized_step = build + ONE pdmpc_plan_joint of one problem + apply (the records: pdmpc_controller_records); centralized_run =
 * n_steps of them, ms as for pdmpc_controller_run.  pdmpc_controller_last_timing / _timing_sum get their parts as for a plain step.
 * The reference has no fallback for this controller (:61-70): if any record carries PDMPC_EXHAUSTED, apply (and so step and run)
 * returns PDMPC_EXHAUSTED, applies nothing and leaves the plant state where it was; the time step stays advanced;
 * pdmpc_controller_last_error names the step, and centralized_run stops there.
 * Refused before anything advances: more than PDMPC_JOINT_MAX vehicles (PDMPC_ERR_CAPACITY); a handle whose checker is not
 * PDMPC_CHECK_SAT, and centralized_step / _run without a handle (PDMPC_ERR_INVALID).  Build, problem and apply work without a handle. */
int pdmpc_controller_centralized_build(pdmpc_controller* c);
int pdmpc_controller_centralized_problem(pdmpc_controller* c, int32_t* n, const pdmpc_vehicle_in** in);
int pdmpc_controller_centralized_apply(pdmpc_controller* c, const pdmpc_vehicle_out* records);
int pdmpc_controller_centralized_step(pdmpc_controller* c);
int pdmpc_controller_centralized_run(pdmpc_controller* c, int32_t n_steps, double* ms);

/* ---- several closed loops in lock-step (csrc/step_controller.cpp, the end of the file) ----
 * A sweep borrows n_members controllers that were created on the same handle (or all without one) and steps them together: every
 * member's build_step, with the device's step preparation grouped over the members (pdmpc_bound_reachable_sets on the concatenated
 * vehicles, pdmpc_*_coupling_grouped: a pair of two members is never looked at; pdmpc_fca_collisions_grouped for the members with FCA
 * priorities, each with its own pairs, obstacles and sizes), ONE pdmpc_plan_step for the concatenated problem,
 * every member's apply.  After a sweep step each member is byte for byte where its own pdmpc_controller_step would have left it
 * (state, records in its own slot order, problem, seeds, time step, expected work, fallback bookkeeping): a member can be taken out of
 * a sweep and stepped alone afterwards.  The plain prioritized step, the explorative step and the optimal-priority step (both below)
 * are part of a sweep, with the graph search or the sampled optimizer.
 * pdmpc_sweep_create checks before anything advances: members on the sweep's handle, or all without one; one Hp; one optimizer
 * (PDMPC_ERR_INVALID each); no member twice (PDMPC_ERR_INVALID); sum of the members' vehicles <= the handle's max_vehicles
 * (PDMPC_ERR_CAPACITY).  Members may differ in everything else.
 * pdmpc_sweep_problem: the concatenated problem as pdmpc_plan_step receives it (the members' entries shallow-copied, pred_index
 * shifted by the member's first slot); member[s] / member_slot[s] = whose slot s is and which slot of that member's own problem.
 * pdmpc_sweep_apply takes records in that slot order.  pdmpc_sweep_last_timing: the six parts of pdmpc_controller_last_timing for
 * the whole lock-step.
 * An error while a step is built or planned is returned as the failing call returned it and leaves the sweep refusing further steps
 * with PDMPC_ERR_INVALID: the members have then advanced UNEVENLY (some built or applied the step, others did not). */
typedef struct pdmpc_sweep pdmpc_sweep;
int pdmpc_sweep_create(pdmpc_handle* handle, int32_t n_members, pdmpc_controller* const* members, pdmpc_sweep** out);
int pdmpc_sweep_destroy(pdmpc_sweep* s); /* the members stay the caller's */
int pdmpc_sweep_build(pdmpc_sweep* s);
int pdmpc_sweep_problem(pdmpc_sweep* s, int32_t* n_slots, const pdmpc_vehicle_in** in, const int32_t** pred_offset, const int32_t** pred_index,
                        const pdmpc_polygon_set** fallback, const int32_t** member, const int32_t** member_slot);
int pdmpc_sweep_apply(pdmpc_sweep* s, const pdmpc_vehicle_out* records);
int pdmpc_sweep_step(pdmpc_sweep* s);
int pdmpc_sweep_run(pdmpc_sweep* s, int32_t n_steps, double* ms);
int pdmpc_sweep_last_timing(pdmpc_sweep* s, double* ms6);
/* The step-preparation calls the last build of the sweep made, whatever the number of members: calls4[0] lanelet bounding, [1] the
 * coupler on the bounded sets, [2] the coupler on the plain hulls, [3] future collision assessment -- device calls, or calls of the
 * host twins for a sweep without a handle (where lanelet bounding is one call per member and the hull coupler one per table of local
 * hulls).  A bounding call that is repeated with more room counts once. */
int pdmpc_sweep_last_prep_calls(pdmpc_sweep* s, int32_t* calls4);
/* ... and its HDV traffic stage: calls2[0] the traffic calls -- with a handle ONE pdmpc_hdv_traffic_grouped for all members with HDVs
 * (a further one for every PDMPC_HDV_MAP_SLOTS distinct maps or PDMPC_HDV_GROUPED_MAX_VEHICLES HDVs beyond the first), without a handle
 * one call of the host twin per such member --, calls2[1] the map uploads it made: members whose maps and hulls are equal byte for byte
 * share a map slot of the handle, and a map that is still resident is not uploaded again.  A call repeated with more room counts once. */
int pdmpc_sweep_last_hdv_calls(pdmpc_sweep* s, int32_t* calls2);
/* The explorative step of a sweep: every member's explorative batch of n_perm prioritizations (seed = its time step),
 * the step preparation grouped as for pdmpc_sweep_build, the members' flattened batches one after the other (predecessor slots shifted by
 * the member's first slot), ONE pdmpc_plan_step_chosen with the members' choice descriptions concatenated -- one launch of the searches,
 * the choice of every member on the device, one read-back --, every member's apply of its chosen plans.  After it each member is byte for
 * byte where its own pdmpc_controller_explore_step would have left it (state, chosen instances, cost table, kept records, couplings,
 * seeds, time step, expected work, fallback bookkeeping); pdmpc_controller_explore_result / _records read a member's part and
 * pdmpc_controller_explore_follow_own is honoured per member.  A sweep may alternate plain and explorative steps.
 * explore_problem: the concatenated batch; member / instance / vehicle / level per slot.  explore_apply takes the records of all its
 * slots, chooses per member on the host and applies (works without a handle).  Refused before any member advances: n_perm < 1 and a
 * broken sweep (PDMPC_ERR_INVALID), sum of n_m * n_perm > the handle's max_vehicles (PDMPC_ERR_CAPACITY), explore_step / explore_run
 * without a handle (PDMPC_ERR_INVALID). */
int pdmpc_sweep_explore_build(pdmpc_sweep* s, int32_t n_perm);
int pdmpc_sweep_explore_problem(pdmpc_sweep* s, int32_t* n_slots, const pdmpc_vehicle_in** in, const int32_t** pred_offset, const int32_t** pred_index,
                                const pdmpc_polygon_set** fallback, const int32_t** member, const int32_t** instance, const int32_t** vehicle,
                                const int32_t** level);
int pdmpc_sweep_explore_apply(pdmpc_sweep* s, const pdmpc_vehicle_out* records);
int pdmpc_sweep_explore_step(pdmpc_sweep* s, int32_t n_perm);
int pdmpc_sweep_explore_run(pdmpc_sweep* s, int32_t n_perm, int32_t n_steps, double* ms);
/* The optimal-priority step of a sweep: the step preparation grouped as for pdmpc_sweep_build up to every member's
 * coupling, ONE pdmpc_unique_priorities_grouped over the members' coupling graphs (its host twin for a sweep without a handle), every
 * member's optimal-priority batch (pdmpc_controller_optimal_build's instances: K_m differs per member and per step), the batches one
 * after the other, ONE pdmpc_plan_step_chosen with the members' optimal-priority choices concatenated, every member's apply of its chosen
 * plans.  After it each member is byte for byte where its own pdmpc_controller_optimal_step(max_instances) would have left it (state,
 * chosen instance per vehicle, the n x K cost table, kept records, the couplings of the chosen instances, seeds, time step, expected
 * work, fallback bookkeeping); pdmpc_controller_optimal_result / _records read a member's part (the sweep keeps the chosen records only).
 * A sweep may alternate plain, explorative and optimal-priority steps.  optimal_problem: the concatenated batch; member / instance /
 * vehicle / level per slot.  optimal_apply takes the records of all its slots, chooses per member on the host and applies (works
 * without a handle).  optimal_last_calls: calls2[0] the enumeration calls of the last build (1, whatever the number of members),
 * calls2[1] the launches of the searches of the last optimal_step (0 after a build alone).
 * Refused before any member advances: a null or broken sweep, max_instances < 1, optimal_step / optimal_run without a handle
 * (PDMPC_ERR_INVALID); a member with more than 64 vehicles (PDMPC_ERR_CAPACITY).  Known only once the couplings exist, so returned by
 * the build AFTER the members have advanced, and leaving the sweep refusing further steps as any failed step does (the handle goes on
 * working): a member with more than 32 coupling edges, a member with more than max_instances unique prioritizations, and a sum of
 * K_m * n_m above the handle's max_vehicles (PDMPC_ERR_CAPACITY each). */
int pdmpc_sweep_optimal_build(pdmpc_sweep* s, int32_t max_instances);
int pdmpc_sweep_optimal_problem(pdmpc_sweep* s, int32_t* n_slots, const pdmpc_vehicle_in** in, const int32_t** pred_offset, const int32_t** pred_index,
                                const pdmpc_polygon_set** fallback, const int32_t** member, const int32_t** instance, const int32_t** vehicle,
                                const int32_t** level);
int pdmpc_sweep_optimal_apply(pdmpc_sweep* s, const pdmpc_vehicle_out* records);
int pdmpc_sweep_optimal_step(pdmpc_sweep* s, int32_t max_instances);
int pdmpc_sweep_optimal_run(pdmpc_sweep* s, int32_t max_instances, int32_t n_steps, double* ms);
int pdmpc_sweep_optimal_last_calls(pdmpc_sweep* s, int32_t* calls2);
/* Centralized members in a sweep: every live member's pdmpc_controller_centralized_build, the members' joint problems
 * as the problems of ONE pdmpc_plan_joint -- one launch for the whole sweep, one wavefront per member --, every member's
 * centralized_apply.  Members may differ in vehicle count (1 to PDMPC_JOINT_MAX), scenario and everything else pdmpc_sweep_create
 * allows.  After a step each member is byte for byte where its own pdmpc_controller_centralized_step would have left it (state,
 * records, problem, time step): a member can be taken out and stepped alone.
 * centralized_problem: *n_problems live members' problems; problem p = in[problem_offset[p] .. problem_offset[p + 1]), member[p] = whose
 * it is.  centralized_apply takes the records in that order (works without a handle).
 * A member whose search is exhausted is not applied, is recorded (centralized_status: exhausted_at[m] = the time step at which member
 * m's search ran empty, 0 for a live member) and is left out of all later steps -- it is not built and its time step does not advance
 * --; the other members go on and the step returns PDMPC_OK.  Once no member is live, centralized_step returns PDMPC_EXHAUSTED (and
 * centralized_run stops there).
 * When one problem outgrows its arena, pdmpc_plan_joint plans the call again for ALL problems with larger arenas (its rule); an
 * overflow at the arena limit, or any error, breaks the sweep as every failed step does.
 * Refused before any member advances: a member with more than PDMPC_JOINT_MAX vehicles (PDMPC_ERR_CAPACITY); a handle whose checker is
 * not PDMPC_CHECK_SAT, a broken sweep, and centralized_step / _run without a handle (PDMPC_ERR_INVALID). */
int pdmpc_sweep_centralized_build(pdmpc_sweep* s);
int pdmpc_sweep_centralized_problem(pdmpc_sweep* s, int32_t* n_problems, const int32_t** problem_offset, const pdmpc_vehicle_in** in, const int32_t** member);
int pdmpc_sweep_centralized_apply(pdmpc_sweep* s, const pdmpc_vehicle_out* records);
int pdmpc_sweep_centralized_step(pdmpc_sweep* s);
int pdmpc_sweep_centralized_run(pdmpc_sweep* s, int32_t n_steps, double* ms);
int pdmpc_sweep_centralized_status(pdmpc_sweep* s, int32_t* exhausted_at); /* [n_members]: 0, or the time step at which the member's search ran empty */

/* ---- several GPUs behind the same boundary (csrc/group.cpp) ----
 * The reference's vehicles exchange their solved areas after every computation level: each publishes a Predictions message that every
 * coupled vehicle reads (hlc/communication/PredictionsCommunication.m:34-63, sent from PrioritizedController.publish_predictions,
 * PrioritizedController.m:356-365, read back at :476-491).  A group is that exchange between the GPUs of ONE process: one handle and
 * one stream per device, bound by an RCCL communicator (ncclCommInitAll; librccl is loaded when the first group is created, the
 * single-GPU entry points do not need it).  pdmpc_group_plan_step plans a time step over the group:
 *   PDMPC_SHARD_COMPONENTS  the weakly connected components of the step's coupling graph exchange nothing within the step: every
 *                           device takes whole components (longest processing time first on `weights`), plans them with ONE
 *                           launch, and ONE all-gather of the result records ends the step;
 *   PDMPC_SHARD_LEVELS      every computation level is block-partitioned over the devices; after each level one all-gather of the
 *                           level's records (2.9 KB per vehicle) on the handles' streams, imported on every device as predecessor
 *                           areas of the next level -- the literal image of the per-level Predictions broadcast;
 *   PDMPC_SHARD_AUTO        whole components, except a component that outweighs the mean load per device: that one by levels over
 *                           all devices, the others whole.
 * The prioritization instances of an explorative step (pdmpc_controller_explore_*) are components of their batch: COMPONENTS deals
 * them out.  Arguments as for pdmpc_plan_step (any slot order; records come back in the caller's order); weights (may be NULL: 1
 * each) = expected work per vehicle, e.g. n_popped of the previous step.  Results are those of the single launch, bit for bit. */
enum { PDMPC_SHARD_AUTO = 0, PDMPC_SHARD_COMPONENTS = 1, PDMPC_SHARD_LEVELS = 2 };
typedef struct pdmpc_group pdmpc_group;
/* devices: n_devices HIP device ordinals (NULL: 0 .. n_devices - 1); config as for pdmpc_create (config.device is ignored).
 * The exchange between the ranks sits behind a function table (csrc/group.cpp: struct Collective):
 *   PDMPC_COLLECTIVE_RCCL  ncclAllGather on the handles' streams, one communicator per device (ncclCommInitAll) — distinct devices;
 *   PDMPC_COLLECTIVE_COPY  the same all-gather as peer copies ordered by HIP events on the handles' streams (no library, no host
 *                          wait).  A device may then be listed more than once: such ranks are LOGICAL ranks — a handle, a stream
 *                          and arenas of their own on a shared GPU — and the whole multi-rank protocol (slot remapping, block
 *                          partition of a level, import of the other ranks' blocks) runs on a 1-GPU box;
 *   PDMPC_COLLECTIVE_AUTO  RCCL for distinct devices (PDMPC_GROUP_COLLECTIVE=copy in the environment: peer copies), peer copies
 *                          when a device is listed twice.
 * pdmpc_group_create = pdmpc_group_create_ex(..., PDMPC_COLLECTIVE_AUTO, ...).  Every pdmpc_group_* and pdmpc_* entry point leaves
 * the calling thread's current HIP device as it found it. */
enum { PDMPC_COLLECTIVE_AUTO = 0, PDMPC_COLLECTIVE_RCCL = 1, PDMPC_COLLECTIVE_COPY = 2 };
int pdmpc_group_create(const pdmpc_config* config, int32_t n_devices, const int32_t* devices, pdmpc_group** out_group);
int pdmpc_group_create_ex(const pdmpc_config* config, int32_t n_devices, const int32_t* devices, int32_t collective, pdmpc_group** out_group);
int pdmpc_group_collective(pdmpc_group* group, int32_t* collective); /* which of the two the group uses (RCCL or COPY) */
int pdmpc_group_destroy(pdmpc_group* group);
int pdmpc_group_size(pdmpc_group* group, int32_t* n_devices);
int pdmpc_group_handle(pdmpc_group* group, int32_t rank, pdmpc_handle** handle); /* rank's handle (statistics, debug read-backs) */
/* The arenas of every device at least `max_nodes` nodes per vehicle (pdmpc_grow_arena on each handle).  pdmpc_group_plan_step grows them
 * by itself when a search overflows; a caller of the resident path (pack_step / launch / fetch), which does not plan again, sizes them
 * here — e.g. with what a single handle needed for the same steps — and reads the statuses. */
int pdmpc_group_grow_arena(pdmpc_group* group, int32_t max_nodes);
int pdmpc_group_upload_mpa(pdmpc_group* group, const pdmpc_mpa* mpa);
int pdmpc_group_plan_step(pdmpc_group* group, int32_t n_vehicles, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                          const pdmpc_polygon_set* fallback_shapes, const double* weights, int32_t mode, pdmpc_vehicle_out* out);
/* The three parts of pdmpc_group_plan_step on their own, for steps that stay resident (bench.py's timed replay): pack partitions the
 * step and makes its sub-problems resident on the devices in group bank `bank` (0 .. 999; the handles' own banks 0 .. 2047 stay the
 * caller's), launch plans a packed bank (launches, all-gathers and imports enqueued on the handles' streams, ONE wait at the end; no
 * host-to-device copy), fetch copies the records of the bank launched last to the host (PDMPC_ERR_INVALID for any other bank: the
 * devices hold one step's gathered records).  plan_step = pack(0) + launch(0) + fetch(0). */
int pdmpc_group_pack_step(pdmpc_group* group, int32_t bank, int32_t n_vehicles, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                          const pdmpc_polygon_set* fallback_shapes, const double* weights, int32_t mode);
int pdmpc_group_launch(pdmpc_group* group, int32_t bank);
int pdmpc_group_fetch(pdmpc_group* group, int32_t bank, int32_t n_vehicles, pdmpc_vehicle_out* out);
/* The partition pdmpc_group_plan_step uses, on its own (no GPU needed): rank_of[v] = device that plans vehicle v as part of a whole
 * component, or -1 if v belongs to the component that is planned by levels over all devices (then level_of[v] = its computation
 * level, 1-based, and block_rank[v] = the device of its block within that level; 0 / -1 for the others).  Twin of
 * pdmpc.distributed.partition_components / hybrid_partition / level_partition. */
int pdmpc_group_partition(int32_t n_vehicles, const int32_t* pred_offset, const int32_t* pred_index, const double* weights, int32_t n_devices, int32_t mode,
                          int32_t* rank_of, int32_t* level_of, int32_t* block_rank);
/* wall-clock milliseconds of the last pdmpc_group_plan_step and of its phases: [0] total, [1] partition + sub-problems, [2] pack,
 * [3] launches and collectives enqueued, [4] wait, [5] read-back */
int pdmpc_group_last_timing(pdmpc_group* group, double* ms6);

/* ---- the sampled optimizer, the lean read-back and the choice on a group (csrc/group.cpp, group_route.hpp, group_choice_kernel.hip;
 * DESIGN.md section 6.1) ----
 * After the launches of a step a rank HOLDS the records it planned: those of its whole components in the order of its part; the
 * records of the component planned by levels pass through every rank, rank 0 holds them behind its own.  The calls below leave the
 * records there -- until the group's next launch, or a launch on one of its handles -- and move only what the caller keeps.
 *
 * pdmpc_group_set_step_seeds: the sampled optimizer's seed per vehicle, in the caller's order, for the NEXT pack of the group
 * (pdmpc_group_plan_step*, pdmpc_group_pack_step), which consumes them also if it fails -- pdmpc_set_step_seeds for a group.  The seeds
 * travel with the sub-problems, every rank packs a sampled bank for its share, and the records are pdmpc_plan_step_sampled's on one
 * handle, bit for bit, in every sharding mode.  A seed count other than the packed step's: PDMPC_ERR_INVALID. */
int pdmpc_group_set_step_seeds(pdmpc_group* group, int32_t n_vehicles, const uint32_t* seeds);
/* pdmpc_set_sampled_budget on every rank's handle: the sampled packs of the group from now on.  A pack with seeds that finds ranks
 * with different budgets (one set on a single rank's handle) returns PDMPC_ERR_INVALID.  PDMPC_ERR_INVALID for a NULL group and for a
 * budget outside 1..PDMPC_SAMPLED_BUDGET_MAX (no rank is changed). */
int pdmpc_group_set_sampled_budget(pdmpc_group* group, int32_t n_expansions_max);
/* pdmpc_set_sampled_ensemble on every rank's handle, with the same rules: a pack with seeds that finds ranks with different ensemble
 * sizes returns PDMPC_ERR_INVALID; PDMPC_ERR_INVALID for a NULL group and for a size outside 1..PDMPC_SAMPLED_ENSEMBLE_MAX (no rank
 * is changed).  The members of a slot run on the rank that holds the slot: what crosses ranks is the winner's record, as before. */
int pdmpc_group_set_sampled_ensemble(pdmpc_group* group, int32_t n_members);
/* pdmpc_plan_step_lean / pdmpc_fetch_records_at over the group: status[v] and final_cost[v] = path_nodes[Hp][4] in the caller's order
 * (every rank's kernel writes the 16-byte entries of the records it holds into host memory; no record leaves a device but in the
 * level exchanges of a shared component), then the records wanted, each read from the rank that holds it.  Arena overflow as in
 * pdmpc_group_plan_step: arenas doubled on every rank, the step planned again; a predecessor time-out stays a status.
 * pdmpc_group_fetch_records_at reads the step launched last (by any pdmpc_group_* launch): PDMPC_ERR_INVALID if there is none. */
int pdmpc_group_plan_step_lean(pdmpc_group* group, int32_t n_vehicles, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                               const pdmpc_polygon_set* fallback_shapes, const double* weights, int32_t mode, int32_t* status, double* final_cost);
int pdmpc_group_fetch_records_at(pdmpc_group* group, int32_t count, const int32_t* vehicles, pdmpc_vehicle_out* out);
/* pdmpc_plan_step_chosen / pdmpc_choose_resident over the group; the contract is pdmpc_choice's, unchanged, and pdmpc_choose_host the
 * checker.  A cell may list slots of several ranks and a graph's candidates usually lie on several: behind its launches every rank
 * writes a 16-byte entry per record it holds, ONE all-gather of the entries runs through the group's collective on the handles'
 * streams, every rank computes the cells and first minima from the same entries in the list's order (the same bits on every rank, and
 * the host twin's), and copies the picked records IT holds to their places in one block of host memory; rank 0 adds chosen, cell_cost
 * and the status counters.  The host waits once per planned attempt; the only whole records that leave a device are the picks.
 * pdmpc_group_choose_resident chooses on group bank `bank`, which must be the one launched last (else PDMPC_ERR_INVALID), and refuses
 * what pdmpc_choose_resident refuses. */
int pdmpc_group_plan_step_chosen(pdmpc_group* group, int32_t n_vehicles, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                                 const pdmpc_polygon_set* fallback_shapes, const double* weights, int32_t mode, const pdmpc_choice* choice, int32_t* chosen,
                                 double* cell_cost, pdmpc_vehicle_out* picks);
int pdmpc_group_choose_resident(pdmpc_group* group, int32_t bank, int32_t n_vehicles, const pdmpc_choice* choice, int32_t* chosen, double* cell_cost,
                                pdmpc_vehicle_out* picks);
/* The test window of the choice over ranks: record v is uploaded to rank rank_of[v] (a rank's records in ascending v); with
 * rank_of[v] == -1 to every rank, as a record of the shared component (rank 0 holds it); then exactly the entries, exchange and
 * kernels of pdmpc_group_choose_resident.  rank_of outside [-1, world): PDMPC_ERR_INVALID. */
int pdmpc_group_debug_choose(pdmpc_group* group, int32_t n_records, const pdmpc_vehicle_out* records, const int32_t* rank_of, const pdmpc_choice* choice,
                             int32_t* chosen, double* cell_cost, pdmpc_vehicle_out* picks);
/* The host code's own accounting of the last pdmpc_group_* call that launched or read back: [0] bytes EACH rank put into collectives,
 * [1] bytes that reached the host, by copies and by kernel writes to host memory, [2] times the host blocked (a wait on all streams
 * counts once, a blocking copy once), [3] attempts planned again after an arena overflow.  With E = 16 (an entry), R =
 * sizeof(pdmpc_vehicle_out), world ranks and per = the most records a rank holds:
 *   a choice (resident, debug)   [0] (per + 1) E   [1] 4 PDMPC_CHOICE-counters + 4 n_graphs (padded to 8) + 8 n_cells + n_picks R   [2] 1
 *   plan_step_lean               [0] the level exchanges' records only   [1] (n + world) E per attempt   [2] 1 per attempt
 *   fetch_records_at             [0] 0   [1] count R   [2] 1 */
int pdmpc_group_last_exchange(pdmpc_group* group, int64_t* out4);
/* The route on its own (no GPU needed): rank[v] = the rank that holds vehicle v's record after the launches of the step so
 * partitioned (pdmpc_group_partition's arguments), position[v] = its index among the records that rank holds. */
int pdmpc_group_route_host(int32_t n_vehicles, const int32_t* pred_offset, const int32_t* pred_index, const double* weights, int32_t n_devices, int32_t mode,
                           int32_t* rank, int32_t* position);
/* The native controller and the sweep on a group (csrc/step_controller.cpp: plan_built).  The controller -- the sweep and every member
 * -- must have been created on pdmpc_group_handle(group, 0), and mode must be a PDMPC_SHARD_* (else PDMPC_ERR_INVALID); group == NULL
 * returns it to its handle.  The step preparation stays on that handle (reachable-set coupling, bounding, FCA, unique prioritizations);
 * what is PLANNED goes over the group: pdmpc_controller_step / _run and pdmpc_sweep_step / _run through pdmpc_group_plan_step (last
 * step's pops are the partition's weights too), the explorative and optimal-priority steps through pdmpc_group_plan_step_lean +
 * pdmpc_group_fetch_records_at or, with the choice on the device (pdmpc_controller_set_device_choice; always in a sweep),
 * pdmpc_group_plan_step_chosen, the sampled optimizer through pdmpc_group_set_step_seeds.  After every step the controller's state,
 * records, problem, seeds, chosen instances and cost table are byte for byte what the same call leaves without a group.
 * Centralized steps (pdmpc_plan_joint) keep running on the handle.  pdmpc_controller_last_timing's backend parts are then
 * pdmpc_group_last_timing's: [1] partition and pack, [2] launches and collectives enqueued, [3] wait and read-back. */
int pdmpc_controller_set_group(pdmpc_controller* c, pdmpc_group* group, int32_t mode);
int pdmpc_sweep_set_group(pdmpc_sweep* s, pdmpc_group* group, int32_t mode);

const char* pdmpc_last_error(void);
const char* pdmpc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PDMPC_H */
