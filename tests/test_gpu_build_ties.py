"""Device builds and writes on TIE-HEAVY corpora (fixtures.lattice_rows, fixtures.duplicate_groups; the oracle-only half is
tests/test_tie_fixtures.py) against the oracle's restatement of the reference's sequential insertion.

Every other write-path test draws Gaussian rows: no two distances are equal, so the (score, id) order of the beam, the strict < of
select_diverse and -- above all -- the slack of the build searches' register beam never decide anything.  Here a handful of distinct
distances covers thousands of pairs: in hundreds of inserts per case more rows tie with the worst entry of the oracle's W than a
192-entry beam holds (asserted on the oracle before the device is touched).  The device counts the nodes whose build search evicted a
tie past the beam's slack (hvx_index_last_write_tie_overflows) and promises the reference's rows only for calls whose count is 0.

What is asserted, per case:
  * h (always, before the row comparison): rows that differ from the oracle's come with a count > 0.  A divergence with a count of 0
    is a failure of its own and is reported as such.
  * with a count of 0 -- the header's precondition -- rows, entry point, levels and, where the corpus fits the search path's widest beam
    (832 entries), 16 searches equal the oracle's.
  * the audit, on every sequential build; a call with a count above 0 is held to h and the audit, and the comparison's outcome is printed.
Measured on an MI355X: every case equals the oracle; only "l2_dense" has a count above 0 (28 one node at a time, 27 batched)."""
import time

import numpy as np
import pytest

import fixtures as fx
from test_gpu_build_bf16 import AUDIT_KEYS
from test_gpu_build_wide import assert_rows_equal, assert_searches_equal
from test_gpu_delete import assert_same_graph

pytestmark = pytest.mark.gpu

SEARCH_BEAM_MAX = 832  # the widest beam of the search path's re-run ladder: a corpus of at most this many rows is searched exactly


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


@pytest.fixture(autouse=True)
def runtime(request):
    t0 = time.perf_counter()
    yield
    print(f"[runtime] {request.node.name}: {time.perf_counter() - t0:.2f} s (oracle builds are shared and counted where they first run)")


def shape_of(name):
    _, n, dim, _, metric, m, m0, efc, kern, _, _, _ = fx.TIE_CASES[name]
    return n, dim, metric, m, m0, efc, kern


def tie_queries(c, dim, nz):
    """8 rows of the corpus and 8 fresh lattice points: the searches tie as the inserts did"""
    rows = c["data"][np.random.default_rng(3).permutation(c["data"].shape[0])[:8]]
    return np.vstack([rows, fx.lattice_rows(8, dim, nz, seed=977)]).astype(np.float32)


def audit_clean(a, n, m, m0, unreachable_max):
    print("audit:", a)
    assert a["nodes"] == n and a["has_entry"] == 1
    for key in AUDIT_KEYS:
        assert a[key] <= (unreachable_max if key == "unreachable_l0" else 0), (key, a)
    assert a["max_degree_l0"] <= m0 and a["max_degree_up"] <= m, a


def held_to_the_oracle(label, ties, compare):
    """Invariant h, then the header's promise: with no flagged build search the graph is the oracle's.  compare() raises AssertionError
    where the device's graph is not the oracle's.  Returns whether they were equal."""
    try:
        compare()
        diff = None
    except AssertionError as e:
        diff = str(e).splitlines()[0] if str(e) else "differs"
    print(f"[ties] {label}: flagged nodes {ties}, rows equal the oracle's: {diff is None}" + ("" if diff is None else f" ({diff})"))
    assert diff is None or ties > 0, f"{label}: rows differ from the oracle's with NO flagged build search (the count misses a divergence): {diff}"
    return diff is None


def sequential_build_case(orc, hv, name, link_mode, want_path, dtype=None, generic_kernel=None):
    n, dim, metric, m, m0, efc, kern = shape_of(name)
    c = fx.tie_case(orc, name)  # asserts the tie-prone (and full-row) counts on the oracle first
    kw = {}
    if dtype is not None:
        kw["dtype"] = dtype
    if generic_kernel is not None:
        kw["float_kernel"] = generic_kernel
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=c["ids"], vectors=c["data"], levels=c["levels"], m=m, m0=m0,
                                                ef_construction=efc, sequential=True, link_mode=link_mode, **kw)
    assert st["nodes"] == n and st["batches"] == n - 1
    ties = gix.last_write_tie_overflows()
    g = gix.export_graph()
    equal = held_to_the_oracle(f"{name} link_mode={link_mode} dtype={'bf16' if dtype is not None else 'f32'} (oracle: {c['prone']} tie-prone inserts)",
                               ties, lambda: assert_rows_equal(g, c["ex"], n))
    path = gix.last_write_path()
    assert path == want_path, (path, want_path)
    # the oracle's own graph of these rows may leave nodes unreachable; a graph that is not the oracle's gets the 10 that
    # tests/test_gpu_build_bf16.py grants on top
    audit_clean(gix.audit_graph(), n, m, m0, unreachable_max=c["unreachable"] + (0 if equal else 10))
    if equal and n <= SEARCH_BEAM_MAX:  # (a 1 200-row lattice ties beyond the SEARCH path's widest beam: its re-run is another file's subject)
        nz = fx.TIE_CASES[name][3]
        assert_searches_equal(hv, gix, c["oix"], tie_queries(c, dim, nz))
    gix.close()
    return ties, equal


# ---- a. sequential narrow builds: ef_construction 160 and 100, L2 and cosine, both one-node link steps -------------------------------
@pytest.mark.parametrize("link_mode", [0, 1])
@pytest.mark.parametrize("name", ["l2_small", "cos_small", "l2_efc160", "l2_dense", "l2_prune", "cos_prune"])
def test_sequential_narrow_build_of_a_lattice_is_held_to_the_oracle(orc, hv, name, link_mode):
    """M 16 / M0 32, dim 128: invariant h, the audit, and with a count of 0 the oracle's rows, entry point and levels; the 380-row
    lattices also 16 searches (ids and score bits)."""
    sequential_build_case(orc, hv, name, link_mode, hv.WRITE_EAGER_STEPS if link_mode == 0 else hv.WRITE_ONE_WAVE)


# ---- b. sequential wide builds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link_mode", [0, 1])
def test_sequential_wide_build_of_a_lattice_equals_the_oracle(orc, hv, link_mode):
    """M 32 / M0 64: link_mode 0 runs the eager steps of csrc/hvx_build_wide_seq.hip (the `alive` replay among them), 1 the one-wavefront
    kernels."""
    sequential_build_case(orc, hv, "wide", link_mode, hv.WRITE_WIDE | (hv.WRITE_EAGER_STEPS if link_mode == 0 else hv.WRITE_ONE_WAVE))


# ---- c. bf16 builds of the same lattices against the SAME f32 oracle graph (rounding is the identity on them) --------------------------
@pytest.mark.parametrize("name", ["l2_small", "cos_small", "wide", "l2_efc160"])
def test_sequential_bf16_build_of_a_lattice_equals_the_f32_oracle(orc, hv, name):
    c = fx.tie_case(orc, name)
    assert np.array_equal(fx.round_bf16(c["data"]), c["data"])
    wide = shape_of(name)[4] > 32
    sequential_build_case(orc, hv, name, 0, hv.WRITE_EAGER_STEPS | (hv.WRITE_WIDE if wide else 0), dtype=hv.BF16)


# ---- d. generic builds: dim 100 under the scalar tree; Manhattan, narrow and M 32 / M0 64 ----------------------------------------------
@pytest.mark.parametrize("name,link_mode", [("scalar_100", 0), ("l1_prune", 0), ("l1_prune", 1), ("l1_wide", 0)])
def test_sequential_generic_build_of_a_lattice_equals_the_oracle(orc, hv, name, link_mode):
    """The GENERIC build search and the select / link kernels per metric and summation tree."""
    wide = shape_of(name)[4] > 32
    want = (hv.WRITE_WIDE if wide else 0) | (hv.WRITE_EAGER_STEPS if link_mode == 0 else hv.WRITE_ONE_WAVE)
    sequential_build_case(orc, hv, name, link_mode, want, generic_kernel=hv.KERNEL_SCALAR)


# ---- e. a live image over the duplicate-group corpus ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bf16", [("dup", False), ("dup_wide", False), ("dup", True)])
def test_a_live_image_over_duplicate_groups_follows_the_oracle_through_inserts_deletes_and_upserts(orc, hv, name, bf16):
    """Two exact-copy groups (20 and 80 rows: members tie at 0, and at equal distances with everything else) among lattice filler.  Two
    thirds built on the device with room to grow, the rest by one-node inserts, 40 sequential deletes (the entry point and members of
    both groups among them: the relink's "Mmax closest, then backfill" cuts through equal scores), 40 upserts into freed and live slots,
    then searches; assert_same_graph after each phase (a phase with flagged build searches is held to invariant h instead; the
    deletes search nothing and must always equal)."""
    n, dim, metric, m, m0, efc, _ = shape_of(name)
    c = fx.tie_case(orc, name)
    data, ids, lv, label = c["data"], c["ids"], c["levels"], c["label"]
    rng = np.random.default_rng(41)
    n0 = n * 2 // 3
    kw = {"dtype": hv.BF16} if bf16 else {}
    oix = fx.tie_oracle_factory(orc, name)()  # (a copy this test may change)
    for i in range(n0):
        assert oix.insert(int(ids[i]), data[i], int(lv[i])) == orc.OK
    gix, _ = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids[:n0], vectors=data[:n0], levels=lv[:n0], m=m, m0=m0,
                                               ef_construction=efc, sequential=True, reserve_rows=n - n0, reserve_upper_rows=int(lv[n0:].sum()), **kw)
    tag = f"{name}{' bf16' if bf16 else ''}"
    held_to_the_oracle(f"{tag} build of {n0}", gix.last_write_tie_overflows(), lambda: assert_same_graph(gix, oix, ids[:n0], ()))
    # one-node inserts of the rest
    for i in range(n0, n):
        assert oix.insert(int(ids[i]), data[i], int(lv[i])) == orc.OK
    st = gix.insert_batch(ids[n0:], data[n0:], lv[n0:], ef_construction=efc, sequential=True)
    assert st["nodes"] == n - n0 and gix.rows() == n
    want = (hv.WRITE_WIDE if m0 > 32 else 0) | hv.WRITE_EAGER_STEPS
    assert gix.last_write_path() == want, gix.last_write_path()
    same = held_to_the_oracle(f"{tag} inserts of {n - n0}", gix.last_write_tie_overflows(), lambda: assert_same_graph(gix, oix, ids, ()))
    if not same:  # (flagged build searches and other rows than the oracle's: the later phases have nothing to be compared with)
        gix.close()
        return
    # 40 sequential deletes: the entry point, 6 + 14 members of the two groups, 19 others
    ent = oix.entry()[0]
    pick = lambda mask, k: [int(x) for x in ids[rng.permutation(np.flatnonzero(mask))] if int(x) != ent][:k]
    dels = [ent] + pick(label == 0, 6) + pick(label == 1, 14) + pick(label == -1, 19)
    assert len(set(dels)) == 40
    for nid in dels:
        assert oix.delete(nid) == (orc.OK, True)
    dst = gix.delete_batch(np.asarray(dels, np.uint64))
    assert dst["deleted"] == 40 and gix.live_rows() == n - 40 == oix.count
    assert_same_graph(gix, oix, ids, set(dels))
    # 40 upserts: 20 freed slots, 20 live ones (members of the larger group among them); new vectors: fresh lattice points and, for
    # eight of them, the larger group's own vector (ties at 0 again)
    live = [int(x) for x in ids[rng.permutation(n)] if int(x) not in set(dels)]
    grp1 = [x for x in live if label[int(np.searchsorted(ids, x))] == 1]
    ups = dels[:20] + grp1[:6] + [x for x in live if x not in grp1[:6]][:14]
    assert len(set(ups)) == 40
    newv = fx.lattice_rows(40, dim, 2, seed=4242)
    newv[::5] = data[np.flatnonzero(label == 1)[0]]
    level_of = {int(ids[i]): int(lv[i]) for i in range(n)}
    for t, nid in enumerate(ups):
        if oix.is_live(nid):
            assert oix.delete(nid) == (orc.OK, True)
        assert oix.insert(nid, newv[t], level_of[nid]) == orc.OK
    st = gix.upsert_batch(np.asarray(ups, np.uint64), newv, ef_construction=efc)
    assert st["nodes"] == 40 and gix.live_rows() == n - 20 == oix.count
    assert gix.last_write_path() == want, gix.last_write_path()
    gone = set(dels[20:])
    if held_to_the_oracle(f"{tag} upserts of 40", gix.last_write_tie_overflows(), lambda: assert_same_graph(gix, oix, ids, gone)):
        assert_searches_equal(hv, gix, oix, np.vstack([tie_queries(c, dim, 2)[4:], newv[:4]]))
    gix.close()


# ---- f. batched builds: the invariants, and the count ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dup", "l2_prune"])
def test_batched_build_of_a_tie_corpus_passes_the_audit(orc, hv, name):
    """The default (batched) build, default link_mode: every structural audit counter 0; unreachable nodes at most the ORACLE's own
    count for the same rows (its graph of the duplicate corpus has unreachable nodes: closed cliques of equal rows) plus the 10 that
    tests/test_gpu_build_bf16.py grants batched appends.  The count is printed."""
    n, dim, metric, m, m0, efc, _ = shape_of(name)
    c = fx.tie_case(orc, name)
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=c["ids"], vectors=c["data"], levels=c["levels"], m=m, m0=m0,
                                                ef_construction=efc)
    assert st["nodes"] == n and st["batches"] < n - 1
    a = gix.audit_graph()
    print(f"[ties] batched {name}: unreachable on the device {a['unreachable_l0']}, in the oracle's graph {c['unreachable']}; flagged nodes "
          f"{gix.last_write_tie_overflows()}")
    audit_clean(a, n, m, m0, unreachable_max=c["unreachable"] + 10)
    gix.close()


# ---- g. the count itself ----------------------------------------------------------------------------------------------------------------
def test_the_tie_overflow_count_is_positive_on_the_large_lattice_and_zero_on_gaussian_rows(orc, hv):
    """1 200 x 128 at ef_construction 160: a lattice leaves flagged nodes, Gaussian rows of the same shape none -- the fixture reaches the
    device's path, not only its CPU proxy.

    Measured on an MI355X: the lattice with its non-zeros spread over all 128 coordinates ("l2_efc160": the oracle meets > 192 tied rows in
    1 006 of 1 200 inserts) flags NOTHING, batched or one node at a time.  The proxy counts rows that tie with W's worst entry; the
    device's beam evicts one only after more than 32 STRICTLY closer rows entered a full W, and that lattice has ~18 rows at distance 2 per
    row.  "l2_dense" (non-zeros within 32 coordinates, ~70 rows at distance 2) is the lattice this test holds to a count > 0 in both
    modes (measured: 28 one node at a time, 27 batched); the sparse one's counts are printed (measured: 0 and 0)."""
    n, dim, metric, m, m0, efc, _ = shape_of("l2_dense")
    c = fx.tie_case(orc, "l2_dense")
    counts = {}
    for kind, rows in (("lattice", c["data"]), ("sparse lattice", fx.tie_case(orc, "l2_efc160")["data"]),
                       ("gaussian", np.random.default_rng(5).standard_normal((n, dim)).astype(np.float32))):
        for mode, kw in (("one-node", dict(sequential=True)), ("batched", {})):
            gix, _ = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=c["ids"], vectors=rows, levels=c["levels"], m=m, m0=m0,
                                                       ef_construction=efc, **kw)
            counts[kind, mode] = gix.last_write_tie_overflows()
            gix.insert_batch(c["ids"][:0], rows[:0], c["levels"][:0])
            assert gix.last_write_tie_overflows() == 0  # a call that linked nothing
            gix.close()
    print(f"[ties] flagged nodes at 1 200 x 128, ef_construction 160 (oracle: {c['prone']} tie-prone inserts): {counts}")
    assert counts["lattice", "one-node"] > 0 and counts["lattice", "batched"] > 0
    assert all(v <= n for v in counts.values())  # one count per node at most
    assert counts["gaussian", "one-node"] == 0 and counts["gaussian", "batched"] == 0
