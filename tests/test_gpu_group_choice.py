"""The choice among the plans of a batch whose records lie on the ranks of a group (csrc/group_choice_kernel.hip behind
pdmpc_group_debug_choose), on logical ranks that share the one GPU (PDMPC_COLLECTIVE_COPY): records placed on the
ranks by hand, the entries, their all-gather, the cells and first minima on every rank and the gather of the picks each rank holds,
against the host twin pdmpc_choose_host — chosen, cell costs and picked records as bytes."""
import numpy as np
import pytest

from pdmpc import abi
from pdmpc.backend import COLLECTIVE_COPY, COLLECTIVE_RCCL, BackendError, Choice, Group, choose_host_call
from pdmpc.config import Config, ScenarioType

from test_choice import ARENA_OVERFLOW, ERR_HIP, EXHAUSTED, OK, lean
from test_sweep import ERR_INVALID, HP, _bits

pytestmark = pytest.mark.gpu

REC = abi.VEHICLE_OUT_DTYPE.itemsize
ENTRY = 16  # bytes of a record's entry in the exchange
COUNTERS = 4  # status counters of the block the host reads (int32 each)
ERR_NO_DEVICE = -2
WORLDS = [2, 4]


@pytest.fixture(scope="module", params=WORLDS)
def group(request):
    options = Config(scenario_type=ScenarioType.commonroad, Hp=HP, max_vehicles=16, max_nodes=1 << 10)
    g = Group(options, n_devices=request.param, devices=[0] * request.param)
    assert g.collective == "copy"
    yield g
    g.close()


def records(rng, n):
    """n records of distinct payload bytes, every status OK and a final cost that is a multiple of 2^-20 (sums of them are exact)."""
    recs = abi.out_array(n)
    raw = recs.view(np.uint8).reshape(n, -1)
    raw[:] = rng.integers(0, 256, raw.shape, dtype=np.uint8)
    raw[:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)  # (no two records alike)
    recs["status"] = OK
    recs["path_nodes"][:, HP, 4] = rng.integers(1 << 20, 1 << 24, n) / float(1 << 20)
    return recs


def host_block_bytes(choice):
    """what a choice writes for the host: counters, chosen (padded to 8 bytes), cell costs, picked records"""
    head = COUNTERS * 4 + 4 * choice.n_graphs
    return (head + 7) // 8 * 8 + 8 * choice.n_cells + REC * choice.n_picks


def assert_group_is_host(g, recs, rank_of, choice, ctx):
    chosen, cost, picks = g.debug_choose(recs, rank_of, choice)
    want_chosen, want_cost = choose_host_call(*lean(recs, HP), choice)
    assert chosen.tolist() == want_chosen.tolist(), ctx
    assert np.array_equal(_bits(cost), _bits(want_cost)), ctx
    assert len(picks) == choice.n_picks
    for i in range(choice.n_picks):
        gr = int(choice.pick_graph[i])
        slot = int(choice.pick_slot[choice.pick_offset[i] + (0 if gr < 0 else want_chosen[gr])])
        assert picks[i].tobytes() == recs[slot].tobytes(), (ctx, i)
    # (f) one host wait; what reached the host is the block; a rank put its entries and a header into the one collective
    x = g.last_exchange()
    held = np.bincount(np.where(np.asarray(rank_of) < 0, 0, rank_of), minlength=g.n_devices)
    assert x["host_waits"] == 1 and x["replans"] == 0, (ctx, x)
    assert x["host_bytes"] == host_block_bytes(choice), (ctx, x)
    assert x["collective_bytes"] == ENTRY * (max(int(held.max()), 1) + 1), (ctx, x)
    return chosen, cost, picks


def test_equal_minima_on_different_ranks_give_the_smaller_index(group):
    """(a) 130 candidates; equal minima at 3 and 67, then at 0 and 129, the HIGHER rank holding the lower index."""
    world = group.n_devices
    rng = np.random.default_rng(1)
    cands = 130
    for first, second in ((3, 67), (0, 129)):
        recs = records(rng, cands + 130)
        rank_of = rng.integers(0, world, len(recs)).astype(np.int32)
        rank_of[first], rank_of[second] = world - 1, 0
        recs["path_nodes"][[first, second], HP, 4] = 0.25
        cells = [[c] for c in range(cands)]
        pick = (0, list(range(cands, 2 * cands)))
        chosen, cost, _ = assert_group_is_host(group, recs, rank_of, Choice(cells, [cands], [pick, pick]), "tie %d/%d" % (first, second))
        assert chosen.tolist() == [first] and cost[first] == cost[second] == 0.25


def test_a_cell_over_three_ranks_adds_in_list_order(group):
    """(b) the order of addition is the list's, not the ranks': costs for which the reverse order gives another cell cost after round(., 8)."""
    world = group.n_devices
    cost = [1e16, 1.0, -1e16, 1.0]
    forward, backward = [0, 1, 2, 3], [3, 2, 1, 0]
    _, twin = choose_host_call([OK] * 4, cost, Choice([forward, backward], [2]))
    assert twin.tolist() == [1.0, 0.0]  # the host twin: the order matters after the rounding
    rng = np.random.default_rng(2)
    recs = records(rng, 12)
    recs["path_nodes"][:4, HP, 4] = cost
    # slots 0..3 on three ranks (two with world 2), ranks NOT in list order: a sum by rank would add in another order
    first = [2, 0, 1, 0] if world > 2 else [1, 0, 1, 0]
    rank_of = np.array(first + [int(r) for r in rng.integers(0, world, 8)], dtype=np.int32)
    _, got, _ = assert_group_is_host(group, recs, rank_of, Choice([forward, backward], [2], [(0, [4, 5])]), "order of addition")
    assert got.tolist() == [1.0, 0.0]
    # sums that differ below the rounding: the first candidate
    recs["path_nodes"][4:8, HP, 4] = (1.0, 1.0 - 1e-9, 0.5, 0.5 - 2e-9)
    chosen, _, _ = assert_group_is_host(group, recs, rank_of, Choice([[4, 6], [5, 7]], [2]), "below the rounding")
    assert chosen.tolist() == [0]


def test_edge_inputs(group):
    """(c) all candidates +inf, a graph without candidates, stray cells, pick_graph == -1, a rank that holds no slot and one that
    holds no pick, a record on every rank."""
    world = group.n_devices
    rng = np.random.default_rng(3)
    n = 40
    recs = records(rng, n)
    rank_of = rng.integers(0, world - 1, n).astype(np.int32)  # the last rank holds no slot
    rank_of[[5, 6, 7]] = -1  # ... and three records are on every rank
    recs["status"][[0, 1, 2]] = EXHAUSTED
    cells = [[0], [1, 9], [2]] + [[10, 5, 11], [12], [6, 13]] + [[20, 21], [], [7]]  # graph 0: all infinite; graph 1; (graph 2: empty); strays
    picks = [(0, [30, 31, 32]), (1, [5, 33, 34]), (-1, [6]), (-1, [35]), (1, [36, 37, 7])]
    choice = Choice(cells, graph_offset=[0, 3, 6, 6], picks=picks)
    chosen, cost, _ = assert_group_is_host(group, recs, rank_of, choice, "edges")
    assert chosen[0] == 0 and np.isinf(cost[:3]).all() and chosen[2] == 0
    # cells in front of the first graph as well, and no pick at all
    assert_group_is_host(group, recs, rank_of, Choice([[3], [4, 5]] + cells, graph_offset=[2, 5, 8, 8]), "cells in front, no pick")
    # every pick held by rank 0: the other ranks hold none
    rank0 = np.zeros(n, dtype=np.int32)
    rank0[20:] = rng.integers(1, world, n - 20)
    assert_group_is_host(group, recs, rank0, Choice([[25], [26]], [2], [(0, [3, 4]), (-1, [5])]), "one rank holds every pick")
    # nothing at all
    assert_group_is_host(group, recs, rank_of, Choice([]), "the empty choice")


def test_a_status_that_is_no_planning_result_fails_the_choice_wherever_it_is(group):
    """(d) ... also on a record that no cell lists, on any rank; the group goes on afterwards."""
    world = group.n_devices
    rng = np.random.default_rng(4)
    choice = Choice([[0], [1]], [2], [(0, [0, 1])])
    for bad in (ARENA_OVERFLOW, ERR_HIP, -7):
        for where, rank in ((29, world - 1), (2, 0), (17, -1)):
            recs = records(rng, 30)
            rank_of = rng.integers(0, world, 30).astype(np.int32)
            rank_of[where] = rank
            recs["status"][where] = bad
            with pytest.raises(BackendError) as e:
                group.debug_choose(recs, rank_of, choice)
            assert e.value.status == ERR_HIP, (bad, where)
            assert group.last_exchange()["host_waits"] == 1
    recs = records(rng, 30)
    assert_group_is_host(group, recs, rng.integers(0, world, 30).astype(np.int32), choice, "after the failures")


def test_refusals_come_before_anything_is_launched(group):
    world = group.n_devices
    rng = np.random.default_rng(5)
    recs = records(rng, 8)
    ok_ranks = np.zeros(8, dtype=np.int32)
    good = Choice([[0], [1]], [2], [(0, [0, 1])])
    for bad_rank in (world, -2):
        ranks = ok_ranks.copy()
        ranks[3] = bad_rank
        with pytest.raises(BackendError) as e:
            group.debug_choose(recs, ranks, good)
        assert e.value.status == ERR_INVALID
    for bad_choice in (Choice([[0], [8]], [2]), Choice([[0], [1]], [2], [(0, [0])]), Choice([[0], [1]], [2], [(2, [0, 1])])):
        with pytest.raises(BackendError) as e:
            group.debug_choose(recs, ok_ranks, bad_choice)
        assert e.value.status == ERR_INVALID
    # nothing has been launched on the group, so no bank's records are resident: a choice on a bank, and a fetch, are refused
    with pytest.raises(BackendError) as e:
        group.choose_resident(0, 8, good)
    assert e.value.status == ERR_INVALID
    with pytest.raises(BackendError) as e:
        group.fetch_records_at([0])
    assert e.value.status == ERR_INVALID


def test_sizes_beyond_one_grid_stride_of_every_kernel(group):
    """(e) 1 300 records (1 100 of them on one rank: more than the 1 024 lanes of the entries kernel), 70 graphs (the cells pass has
    64 wavefronts), 4 200 cells of no graph (more than 64 x 64), 1 300 picks (the gather has 256 workgroups)."""
    world = group.n_devices
    rng = np.random.default_rng(6)
    n = 1300
    recs = records(rng, n)
    recs["status"][rng.integers(0, n, 60)] = EXHAUSTED
    rank_of = np.full(n, world - 1, dtype=np.int32)
    rank_of[rng.permutation(n)[:200]] = rng.integers(-1, world - 1, 200)
    sizes = [int(s) for s in rng.integers(1, 9, 70)]
    sizes[11], sizes[40] = 130, 65
    cells, picks = [], []
    for g, size in enumerate(sizes):
        for c in range(size):
            cells.append([int(s) for s in rng.integers(0, n, int(rng.integers(1, 6)))])
    n_graph_cells = len(cells)
    cells += [[int(s) for s in rng.integers(0, n, 2)] for _ in range(4200)]  # cells of no graph: more than 64 wavefronts of them
    for i in range(n):
        if i % 10 == 0:
            picks.append((-1, [int(rng.integers(0, n))]))
        else:
            g = int(rng.integers(0, 70))
            picks.append((g, [int(s) for s in rng.integers(0, n, sizes[g])]))
    assert len(picks) == 1300 and len(cells) - n_graph_cells > 64 * 64
    assert_group_is_host(group, recs, rank_of, Choice(cells, sizes, picks), "beyond one grid stride")


def test_the_exchange_grows_with_the_entries_not_with_the_records(group):
    """(f) bytes into the collective: 16 per record a rank holds (and a header), whatever a record's size."""
    world = group.n_devices
    rng = np.random.default_rng(7)
    seen = []
    for n in (world * 8, world * 64):
        recs = records(rng, n)
        rank_of = (np.arange(n) % world).astype(np.int32)
        choice = Choice([[c] for c in range(8)], [8], [(0, list(range(8)))] * 3)
        assert_group_is_host(group, recs, rank_of, choice, n)
        seen.append(group.last_exchange())
    assert seen[1]["collective_bytes"] - seen[0]["collective_bytes"] == ENTRY * 56  # 56 more records per rank
    assert seen[1]["collective_bytes"] < REC  # ... all of a rank's entries are less than ONE record
    assert seen[0]["host_bytes"] == seen[1]["host_bytes"] == 3 * REC + 8 * 8 + (COUNTERS * 4 + 4 + 7) // 8 * 8


def _fresh_pair():
    options = Config(scenario_type=ScenarioType.commonroad, Hp=HP, max_vehicles=16, max_nodes=1 << 10)
    g = Group(options, n_devices=2, devices=[0, 0], collective=COLLECTIVE_COPY)
    assert g.collective == "copy"
    return g


def test_every_buffer_of_a_choice_grows_and_the_small_choice_still_holds():
    """The smallest choice (1 graph, 2 cells, 1 pick) on a fresh group of 2 logical ranks, then one that outgrows everything the first call
    left, then the small one again: each equal to the host twin, the picked records byte for byte."""
    rng = np.random.default_rng(8)
    small = Choice([[0], [1]], [2], [(0, [0, 1])])
    small_recs, small_ranks = records(rng, 2), np.array([0, 1], dtype=np.int32)
    # The first call asks for 12 list words, blocks of 2 entries (32 bytes; 64 received), 40 bytes of chosen and cell costs, 2 placed records
    # per rank and a host block of 40 bytes + 1 record.  A buffer grows to 3/2 of what is asked, and of 64 elements at least (DevBuf and
    # PinnedBuf, csrc/hip_host.hpp): 96 words, 96 and 96 bytes, 96 bytes, 96 records, 60 bytes + 1.5 records.  So 100 records per rank
    # (101 placed, blocks of 101 entries = 1 616 bytes), 100 cells in 2 graphs (315 list words, 824 bytes of chosen and cell costs) and
    # 4 picks (a host block beyond 4 records) outgrow each of them.
    n = 200
    large_recs, large_ranks = records(rng, n), (np.arange(n) % 2).astype(np.int32)
    large = Choice([[c] for c in range(100)], [50, 50], [(0, list(range(100, 150))), (1, list(range(150, 200))), (-1, [7]), (-1, [150])])
    assert host_block_bytes(large) > 4 * REC > 1.5 * host_block_bytes(small)
    g = _fresh_pair()
    try:
        assert_group_is_host(g, small_recs, small_ranks, small, "small, fresh group")
        assert_group_is_host(g, large_recs, large_ranks, large, "large, every buffer grows")
        assert_group_is_host(g, small_recs, small_ranks, small, "small, after the growth")
    finally:
        g.close()


def test_groups_come_and_go_and_a_refused_create_leaves_a_working_library():
    """Three groups made and destroyed in one process, a refused create in between (a device listed twice with the RCCL collective: an
    argument refusal, nothing is launched), and the group made after it plans a 2-vehicle step as the single handle does."""
    import problems
    from pdmpc.backend import Handle
    from test_gpu_parity import assert_records_equal

    options, mpa, iters = problems.problem_set("interx", 11, 2, Hp=HP, max_vehicles=8, max_nodes=1 << 14)
    preds = [[] for _ in iters]
    single = Handle(options)
    single.upload_mpa(mpa)
    ref = single.plan_step(iters, preds, None)
    single.close()
    for round_ in range(3):
        g = Group(options, n_devices=2, devices=[0, 0], collective=COLLECTIVE_COPY)
        try:
            g.upload_mpa(mpa)
            assert_records_equal(g.plan_step(iters, preds, None), ref, "group %d" % round_)
        finally:
            g.close()
        if round_ == 1:
            with pytest.raises(BackendError) as e:
                Group(options, n_devices=2, devices=[0, 0], collective=COLLECTIVE_RCCL)
            assert e.value.status == ERR_NO_DEVICE
            assert str(e.value).endswith("pdmpc_group_create: a device listed twice needs PDMPC_COLLECTIVE_COPY (RCCL has one rank per device)")
