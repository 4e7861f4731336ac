"""tests/audit_twin.py is the reference the device audit is held to (tests/test_gpu_audit.py), so it is pinned first: graphs of at most
8 nodes written out literally, every expected figure counted by hand; then an oracle-built graph."""
import numpy as np
import pytest

import audit_twin as tw
import fixtures as fx

S = tw.SENTINEL


def full(**nonzero):
    out = dict.fromkeys(tw.KEYS, 0)
    out.update(nonzero)
    return out


def both(raw):
    return tw.audit(raw), tw.audit(raw, reverse="membership")


def test_a_clean_triangle_has_only_sizes():
    raw = tw.make_raw([[1, 2], [0, 2], [0, 1]], 4, entry=0)
    want = full(nodes=3, edges_l0=6, max_degree_l0=2, bfs_levels_l0=1, has_entry=1)
    assert both(raw) == (want, want)


def test_a_duplicate_id_is_one_unsorted_entry():
    raw = tw.make_raw([[1, 1, 2], [0], [0]], 4, entry=0)
    # 5 slots are edges; the second 1 is not above its predecessor; 1 and 2 still find 0's row listing them
    want = full(nodes=3, edges_l0=5, unsorted_entries=1, max_degree_l0=3, bfs_levels_l0=1, has_entry=1)
    assert both(raw) == (want, want)


def test_a_descending_pair_is_one_unsorted_entry_and_hides_both_ids_from_the_binary_search():
    raw = tw.make_raw([[2, 1], [0], [0]], 4, entry=0)
    # row 0 = [2, 1, S, S]: a lower-bound search for 1 ends at slot 0 (holds 2), for 2 at slot 2 (holds S): 1 -> 0 and 2 -> 0 look one-way
    lb, mem = both(raw)
    assert mem == full(nodes=3, edges_l0=4, unsorted_entries=1, max_degree_l0=2, bfs_levels_l0=1, has_entry=1)
    assert lb == full(nodes=3, edges_l0=4, unsorted_entries=1, asymmetric_edges_l0=2, max_degree_l0=2, bfs_levels_l0=1, has_entry=1)


def test_a_hole_followed_by_two_ids_is_one_hole():
    raw = tw.make_raw([[1, S, 2, 3], [0], [0], [0]], 4, entry=0)
    # only the 2 sits behind a sentinel.  Row 0 = [1, S, 2, 3]: the binary search finds 1 (slot 0) and 3 (slot 3), but for 2 it ends at
    # slot 1 (S): 2 -> 0 looks one-way to it, and to it alone
    lb, mem = both(raw)
    assert mem == full(nodes=4, edges_l0=6, holes=1, max_degree_l0=3, bfs_levels_l0=1, has_entry=1)
    assert lb == full(nodes=4, edges_l0=6, holes=1, asymmetric_edges_l0=1, max_degree_l0=3, bfs_levels_l0=1, has_entry=1)


def test_a_self_loop_finds_its_reverse_edge_in_its_own_row():
    raw = tw.make_raw([[0, 1], [0]], 4, entry=0)
    want = full(nodes=2, edges_l0=3, self_loops=1, max_degree_l0=2, bfs_levels_l0=1, has_entry=1)
    assert both(raw) == (want, want)


@pytest.mark.parametrize("bad", [2, 0xFFFFFFFE])
def test_an_id_of_n_or_above_is_out_of_range_and_nothing_else(bad):
    raw = tw.make_raw([[1, bad], [0]], 4, entry=0)
    want = full(nodes=2, edges_l0=3, out_of_range_ids=1, max_degree_l0=2, bfs_levels_l0=1, has_entry=1)
    assert both(raw) == (want, want)


def test_an_edge_to_a_deleted_row_dangles_and_is_not_asymmetric():
    raw = tw.make_raw([[1, 2], [0], []], 4, dead_rows=[2], entry=0)
    # 2 is deleted: 2 live nodes; 0 -> 2 is out of range, not asymmetric although row 2 is empty; the BFS still steps onto row 2
    want = full(nodes=2, edges_l0=3, out_of_range_ids=1, max_degree_l0=2, bfs_levels_l0=1, has_entry=1)
    assert both(raw) == (want, want)


def test_the_row_of_a_deleted_owner_is_walked_like_any_other():
    raw = tw.make_raw([[1, 2], [0], [0, 1]], 4, dead_rows=[2], entry=0)
    # edges 2 + 1 + 2; 0 -> 2 dangles; 2 -> 0 finds 2 in row 0; 2 -> 1 does not find 2 in row 1
    want = full(nodes=2, edges_l0=5, out_of_range_ids=1, asymmetric_edges_l0=1, max_degree_l0=2, bfs_levels_l0=1, has_entry=1)
    assert both(raw) == (want, want)


def test_the_bfs_walks_through_a_deleted_row_but_never_counts_it_unreachable():
    raw = tw.make_raw([[1], [2], [], [], []], 4, dead_rows=[1, 4], entry=0)
    # 0 -> 1 (deleted: dangles) -> 2 (row 2 does not list 1: asymmetric); 3 is cut off, 4 is too but is deleted; 2 is two steps away
    want = full(nodes=3, edges_l0=2, out_of_range_ids=1, asymmetric_edges_l0=1, unreachable_l0=1, max_degree_l0=1, bfs_levels_l0=2, has_entry=1)
    assert both(raw) == (want, want)


TRI = [[1, 2], [0, 2], [0, 1]]


def test_an_upper_layer_one_way_edge():
    raw = tw.make_raw(TRI, 4, up_rows=[[1], []], su=4, level=[1, 1, 0], entry=0, max_layer=1)
    want = full(nodes=3, up_rows=2, edges_l0=6, edges_up=1, asymmetric_edges_up=1, max_degree_l0=2, max_degree_up=1, bfs_levels_l0=1,
                max_layer=1, has_entry=1)
    assert both(raw) == (want, want)


def test_an_upper_layer_edge_to_a_node_below_the_layer_is_a_level_violation_only():
    raw = tw.make_raw(TRI, 4, up_rows=[[2], []], su=4, level=[1, 1, 0], entry=0, max_layer=1)
    want = full(nodes=3, up_rows=2, edges_l0=6, edges_up=1, level_violations=1, max_degree_l0=2, max_degree_up=1, bfs_levels_l0=1,
                max_layer=1, has_entry=1)
    assert both(raw) == (want, want)


def test_upper_layers_are_looked_up_layer_by_layer():
    # node 0 lives on layers 1 and 2, node 1 on layer 1 only: 0 -> 1 on layer 1 is mutual; on layer 2 it is a level violation
    raw = tw.make_raw(TRI, 4, up_rows=[[1], [1], [0]], su=4, level=[2, 1, 0], entry=0, max_layer=2)
    want = full(nodes=3, up_rows=3, edges_l0=6, edges_up=3, level_violations=1, max_degree_l0=2, max_degree_up=1, bfs_levels_l0=1,
                max_layer=2, has_entry=1)
    assert both(raw) == (want, want)


def test_rows_of_one_id_above_the_limits_overflow_and_a_limit_of_zero_is_the_stride():
    star = [[1, 2, 3], [0], [0], [0]]
    ups = [[1, 2], [0], [0]]
    raw = tw.make_raw(star, 4, up_rows=ups, su=4, level=[1, 1, 1, 0], entry=0, max_layer=1, m=1, m0=2)
    # row 0 holds m0 + 1 = 3 ids on layer 0 and m + 1 = 2 on layer 1
    want = full(nodes=4, up_rows=3, edges_l0=6, edges_up=4, degree_overflow_rows=2, max_degree_l0=3, max_degree_up=2, bfs_levels_l0=1,
                max_layer=1, has_entry=1)
    assert both(raw) == (want, want)
    raw = tw.make_raw(star, 4, up_rows=ups, su=4, level=[1, 1, 1, 0], entry=0, max_layer=1, m=0, m0=0)
    want["degree_overflow_rows"] = 0
    assert both(raw) == (want, want)


PATH5 = [[1], [0, 2], [1, 3], [2, 4], [3]]


def test_a_path_of_five_nodes_has_four_levels_from_its_end_and_two_from_its_middle():
    want = full(nodes=5, edges_l0=8, max_degree_l0=2, bfs_levels_l0=4, has_entry=1)
    assert both(tw.make_raw(PATH5, 4, entry=0)) == (want, want)
    want["bfs_levels_l0"] = 2
    assert both(tw.make_raw(PATH5, 4, entry=2)) == (want, want)


def test_two_components():
    raw = tw.make_raw([[1], [0], [3, 4], [2, 4], [2, 3]], 4, entry=0)
    want = full(nodes=5, edges_l0=8, unreachable_l0=3, max_degree_l0=2, bfs_levels_l0=1, has_entry=1)
    assert both(raw) == (want, want)


def test_a_node_behind_a_one_way_edge_is_reached():
    raw = tw.make_raw([[1], [0, 2], []], 4, entry=0)
    want = full(nodes=3, edges_l0=3, asymmetric_edges_l0=1, max_degree_l0=2, bfs_levels_l0=2, has_entry=1)
    assert both(raw) == (want, want)


def test_without_an_entry_point_every_live_row_is_unreachable():
    want = full(nodes=3, edges_l0=6, unreachable_l0=3, max_degree_l0=2)
    assert both(tw.make_raw(TRI, 4)) == (want, want)
    # ... and a deleted row is not a live one (its edges now dangle: 0 -> 2 and 1 -> 2)
    want = full(nodes=2, edges_l0=6, out_of_range_ids=2, unreachable_l0=2, max_degree_l0=2)
    assert both(tw.make_raw(TRI, 4, dead_rows=[2])) == (want, want)


def test_an_entry_point_with_an_empty_row_reaches_only_itself():
    want = full(nodes=2, unreachable_l0=1, has_entry=1)
    assert both(tw.make_raw([[], []], 4, entry=0)) == (want, want)


def test_an_empty_image_has_no_sizes():
    raw = tw.make_raw([], 4, max_layer=3)
    assert both(raw) == (full(max_layer=3), full(max_layer=3))


def test_is_canonical_tells_when_the_two_look_ups_agree():
    assert tw.is_canonical([1, 5, S, S]) and tw.is_canonical([S, S]) and tw.is_canonical([0, 1, 2, 3])
    assert not tw.is_canonical([1, 1, S, S]) and not tw.is_canonical([2, 1, S, S]) and not tw.is_canonical([1, S, 2, S])


def test_an_oracle_built_graph_is_clean_and_its_sizes_are_the_csr_sizes(orc):
    """n = 600, dim 32, the recipe of build_oracle in tests/test_gpu_parity.py"""
    n, dim, m, m0 = 600, 32, 16, 32
    rng = np.random.default_rng(4100)
    data = rng.standard_normal((n, dim)).astype(np.float32)
    lv = fx.draw_levels(n, m, seed=41)
    oix = orc.Index(dim, orc.L2SQ, kernel=orc.K_AVX_FMA, m=m, m0=m0, ef_construction=100)
    for i in range(n):
        assert oix.insert(i, data[i], int(lv[i])) == orc.OK
    ex = oix.export()
    raw = tw.raw_from_export(ex, 32, 16, m=m, m0=m0)
    a, mem = both(raw)
    assert a == mem
    for key in ("asymmetric_edges_l0", "asymmetric_edges_up", "unsorted_entries", "self_loops", "out_of_range_ids", "holes", "level_violations",
                "degree_overflow_rows"):
        assert a[key] == 0, (key, a)
    assert a["nodes"] == n and a["edges_l0"] == ex["l0_neighbors"].size and a["edges_up"] == ex["up_neighbors"].size > 0
    assert a["up_rows"] == int(ex["level"].sum()) == len(ex["up_offsets"]) - 1
    assert a["max_layer"] == ex["max_layer"] == int(lv.max()) and a["has_entry"] == 1 and a["bfs_levels_l0"] >= 2
    rows = [set(ex["l0_neighbors"][int(ex["l0_offsets"][i]):int(ex["l0_offsets"][i + 1])].tolist()) for i in range(n)]
    assert a["max_degree_l0"] == max(len(r) for r in rows) <= m0 and 0 < a["max_degree_up"] <= m
    seen = todo = {ex["entry_point"]}
    while todo:
        seen, todo = seen | todo, set().union(*(rows[u] for u in todo)) - seen - todo
    assert a["unreachable_l0"] == n - len(seen)
