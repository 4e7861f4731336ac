"""hvx_shortest_path_batch_dense in plain Python, written as its kernels run it (helix-db_amd/csrc/hvx_shortest_path_dense.hip) and not
through shortest_path_twin.backward_levels: Python ints are the u64 words.  Per round and group: seen, cur and next per node, 64 level
bytes per node that are never cleared (they start dirty here), the group's `active` word and its `grew` words by level parity; init, then
per level push / commit / check in runs of RUN levels with the pinned "someone is still active" word read between runs, then the walk out.
Nothing here touches the library; tests/test_shortest_path_dense_host.py holds it to the literal twin."""
import numpy as np

import shortest_path_twin as twin

GROUP = 64
NODE_GROUP_BYTES = 3 * 8 + GROUP
DEFAULT_SCRATCH = 1 << 30
RUN = 4
OK = twin.OK
NO_NODE = twin.NO_NODE
DIRTY = 0xA5   # what a level byte holds before anyone writes it


def plan_rounds(n, b, scratch_bytes=0):
    """hvx_shortest_path_dense_plan.h's plan_rounds: None when the budget does not hold one group"""
    budget = scratch_bytes or DEFAULT_SCRATCH
    fit = budget // (max(n, 1) * NODE_GROUP_BYTES)
    if fit == 0:
        return None
    groups = (b + GROUP - 1) // GROUP
    per_round = max(min(fit, groups), 1)
    words = n * per_round
    return dict(groups=groups, groups_per_round=per_round, rounds=(groups + per_round - 1) // per_round, words=words, seen_off=0,
                cur_off=words * 8, next_off=words * 16, lvl_off=words * 24, bytes=words * NODE_GROUP_BYTES)


def round_of(plan, b, r):
    """(first group, groups, first request, requests) of round r"""
    group0 = r * plan["groups_per_round"]
    n_groups = min(plan["groups_per_round"], plan["groups"] - group0)
    request0 = group0 * GROUP
    return group0, n_groups, request0, min(b - request0, n_groups * GROUP)


def _rows(g, direction, allowed):
    """per node: the targets of its allowed arcs in `direction`, repeats included, in the rows' own order (outgoing rows first)"""
    allowed = set(int(x) for x in allowed)
    rows = [[] for _ in range(g.n)]
    for use_out in (True, False):
        if (use_out and direction == twin.DIR_IN) or (not use_out and direction == twin.DIR_OUT):
            continue
        off, tgt, lab = (g.out_off, g.out_tgt, g.out_lab) if use_out else (g.in_off, g.in_tgt, g.in_lab)
        off, tgt = off.tolist(), tgt.tolist()
        lab = None if lab is None or not allowed else lab.tolist()
        for u in range(g.n):
            for at in range(off[u], off[u + 1]):
                if lab is None or lab[at] in allowed:
                    rows[u].append(tgt[at])
    return rows


def answers(g, sources, targets, max_depth, direction=twin.DIR_OUT, allowed=(), scratch_bytes=0, stats=None):
    """the batch: ([paths], statuses u32 [b], sizes u64 [b][max_depth]); stats (a dict) receives rounds and the host waits of every round"""
    src, dst = [int(s) for s in sources], [int(t) for t in targets]
    b, n = len(src), g.n
    plan = plan_rounds(n, b, scratch_bytes)
    assert plan is not None, "the budget does not hold one group"
    back, fwd = _rows(g, twin.mirrored(direction), allowed), _rows(g, direction, allowed)
    groups, per_round = plan["groups"], plan["groups_per_round"]
    # the round's scratch: reused, and only the words are cleared
    seen, cur, nxt = ([[0] * n for _ in range(per_round)] for _ in range(3))
    lvl = [bytearray([DIRTY]) * (n * GROUP) for _ in range(per_round)]
    active, grew = [0] * groups, [[0] * groups, [0] * groups]
    dist, cnt, ran = [0] * b, [0] * b, [0] * b
    sizes = np.zeros((b, max_depth), np.uint64)
    paths, waits = [[] for _ in range(b)], []
    for r in range(plan["rounds"]):
        group0, n_groups, request0, n_requests = round_of(plan, b, r)
        for gl in range(n_groups):
            for v in range(n):
                seen[gl][v] = cur[gl][v] = nxt[gl][v] = 0
        # init
        live = False
        for i in range(n_requests):
            q, gl, bit = request0 + i, i // GROUP, 1 << (i % GROUP)
            none = src[q] == NO_NODE or dst[q] == NO_NODE
            dist[q], ran[q], cnt[q] = 0, 0, 0 if none else 1
            if none or src[q] == dst[q]:
                continue
            seen[gl][dst[q]] |= bit
            cur[gl][dst[q]] |= bit
            lvl[gl][dst[q] * GROUP + i % GROUP] = 0
            active[group0 + gl] |= bit
            live = True
        level, n_waits = 0, 0
        while live and level < max_depth:
            end = min(level + RUN, max_depth)
            still = False
            while level < end:
                level += 1
                for gl in range(n_groups):   # push: seen does not change
                    act = active[group0 + gl]
                    if not act:
                        continue
                    for u in range(n):
                        w = cur[gl][u] & act
                        if w:
                            for v in back[u]:
                                add = w & ~seen[gl][v]
                                if add:
                                    nxt[gl][v] |= add
                for gl in range(n_groups):   # commit
                    act = active[group0 + gl]
                    if not act:
                        continue
                    for v in range(n):
                        w = nxt[gl][v] & ~seen[gl][v] & act
                        seen[gl][v] |= w
                        cur[gl][v] = w
                        nxt[gl][v] = 0
                        grew[level & 1][group0 + gl] |= w
                        for k in range(GROUP):
                            if w >> k & 1:
                                lvl[gl][v * GROUP + k] = level
                                cnt[request0 + gl * GROUP + k] += 1
                still = False
                for i in range(n_requests):  # check: found before empty
                    q, gl, bit = request0 + i, i // GROUP, 1 << (i % GROUP)
                    if i % GROUP == 0:
                        grew[(level + 1) & 1][group0 + gl] = 0
                    if not active[group0 + gl] & bit:
                        continue
                    found = bool(cur[gl][src[q]] & bit)
                    ran[q] = level
                    sizes[q, level - 1] = cnt[q]
                    if found:
                        dist[q] = level
                    if found or not grew[level & 1][group0 + gl] & bit:
                        active[group0 + gl] &= ~bit
                    else:
                        still = True
            if level == max_depth:
                break
            n_waits += 1   # the host reads the pinned word
            live = still
        # walk out
        for i in range(n_requests):
            q, gl, k = request0 + i, i // GROUP, i % GROUP
            sizes[q, ran[q]:] = cnt[q]
            if dist[q] == 0:
                paths[q] = [src[q]] if src[q] == dst[q] and src[q] != NO_NODE else []
                continue
            c, path = src[q], []
            for step in range(dist[q]):
                path.append(c)
                want = dist[q] - 1 - step
                c = min(v for v in fwd[c] if seen[gl][v] >> k & 1 and lvl[gl][v * GROUP + k] == want)
            paths[q] = path + [c]
        waits.append(n_waits + 1)   # the round's last wait
    if stats is not None:
        stats.update(rounds=plan["rounds"], waits=waits)
    return paths, np.full(b, OK, np.uint32), sizes
