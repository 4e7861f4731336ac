"""shortest_path in plain Python / numpy: the reference's literal loop (crates/db/src/execution/interpreter/shortest_path.rs:16-96 --
queue, visited set, predecessor map, a node's neighbours its distinct allowed neighbours in ascending id order, the search over at the arc
that discovers the target), the characterisation the device kernel computes (levels from the target over the reversed arcs, then always
the smallest neighbour one level closer), and what hvx_shortest_path_batch reports beside the path: the sizes of the backward reach set
level by level and the overflow rule for a given max_reach.  Nothing here touches the library."""
from collections import deque

import numpy as np

OK, ERR_CANDIDATE_LIMIT = 0, 6
DIR_OUT, DIR_IN, DIR_BOTH = 0, 1, 2
NO_NODE = 0xFFFFFFFFFFFFFFFF   # an endpoint that resolved to no node


def _gather(off, nodes):
    """positions of every arc of the rows of `nodes`, row after row"""
    nodes = np.asarray(nodes, np.int64)
    starts, lens = off[nodes], off[nodes + 1] - off[nodes]
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    first = np.cumsum(lens) - lens
    return np.repeat(starts - first, lens) + np.arange(total)


class Graph:
    """A CSR in the arrays hvx_csr_import takes, with the incoming adjacency beside it."""

    def __init__(self, n, off, tgt, lab=None):
        self.n = int(n)
        self.out_off = np.asarray(off, np.int64)
        self.out_tgt = np.asarray(tgt, np.int64)
        self.out_lab = None if lab is None else np.asarray(lab, np.int64)
        owner = np.repeat(np.arange(self.n), np.diff(self.out_off))
        order = np.argsort(self.out_tgt, kind="stable")
        self.in_tgt = owner[order]
        self.in_lab = None if lab is None else self.out_lab[order]
        self.in_off = np.zeros(self.n + 1, np.int64)
        self.in_off[1:] = np.cumsum(np.bincount(self.out_tgt, minlength=self.n))
        self._plans = {}

    @classmethod
    def from_edges(cls, n, src, dst, lab=None):
        """from an edge list, rows ascending by target (stable: parallel edges keep their order)"""
        src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        order = np.lexsort((dst, src))
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum(np.bincount(src, minlength=n))
        return cls(n, off, dst[order], None if lab is None else np.asarray(lab)[order])

    def arrays(self):
        """(n, offsets u64, targets u64, labels u32 or None) as the library takes them"""
        return (self.n, self.out_off.astype(np.uint64), self.out_tgt.astype(np.uint64),
                None if self.out_lab is None else self.out_lab.astype(np.uint32))

    def arcs(self, nodes, direction, allowed=()):
        """every allowed arc target of the rows of `nodes` in `direction`, repeats included"""
        parts = []
        for use_out in (True, False):
            if (use_out and direction == DIR_IN) or (not use_out and direction == DIR_OUT):
                continue
            off, tgt, lab = (self.out_off, self.out_tgt, self.out_lab) if use_out else (self.in_off, self.in_tgt, self.in_lab)
            at = _gather(off, nodes)
            if lab is not None and len(allowed):
                at = at[np.isin(lab[at], np.asarray(list(allowed), np.int64))]
            parts.append(tgt[at])
        return np.concatenate(parts)

    def plan(self, direction, allowed=()):
        """(offsets, neighbours): every node's DISTINCT allowed neighbours in `direction`, ascending -- shortest_path_neighbors' BTreeSet
        for every node at once"""
        key = (int(direction), tuple(sorted(int(x) for x in allowed)))
        if key not in self._plans:
            us, vs = [], []
            for use_out in (True, False):
                if (use_out and direction == DIR_IN) or (not use_out and direction == DIR_OUT):
                    continue
                off, tgt, lab = (self.out_off, self.out_tgt, self.out_lab) if use_out else (self.in_off, self.in_tgt, self.in_lab)
                keep = np.ones(tgt.size, bool) if lab is None or not len(allowed) else np.isin(lab, np.asarray(list(allowed), np.int64))
                us.append(np.repeat(np.arange(self.n), np.diff(off))[keep])
                vs.append(tgt[keep])
            pair = np.unique(np.concatenate(us) * self.n + np.concatenate(vs))
            off = np.zeros(self.n + 1, np.int64)
            off[1:] = np.cumsum(np.bincount(pair // self.n, minlength=self.n))
            self._plans[key] = (off, pair % self.n)
        return self._plans[key]


def literal(g, source, target, max_depth, direction=DIR_OUT, allowed=()):
    """execute_shortest_path for resolved endpoints: the path as a list, source first; [] when none has at most max_depth arcs"""
    if source == target:
        return [int(source)]
    off, nbr = g.plan(direction, allowed)
    queue, visited, predecessor = deque([int(source)]), np.zeros(g.n, bool), {}
    visited[source] = True
    found = False
    for _depth in range(max_depth):
        level_len = len(queue)
        if level_len == 0:
            break
        for _ in range(level_len):
            current = queue.popleft()
            row = nbr[off[current]:off[current + 1]]
            for neighbor in row[~visited[row]].tolist():   # ascending; the ones visited.insert() accepts
                visited[neighbor] = True
                predecessor[neighbor] = current
                if neighbor == target:
                    found = True
                    break
                queue.append(neighbor)
            if found:
                break
        if found:
            break
    if not found:
        return []
    path, current = [int(target)], int(target)
    while current != source:
        current = predecessor[current]
        path.append(current)
    return path[::-1]


def mirrored(direction):
    return {DIR_OUT: DIR_IN, DIR_IN: DIR_OUT, DIR_BOTH: DIR_BOTH}[direction]


def backward_levels(g, source, target, max_depth, direction=DIR_OUT, allowed=(), max_reach=None):
    """Level-synchronous search from the target over the reversed arcs, as the kernel's Phase A runs it: ends when the source is in the set
    (that level completes), a level comes up empty, max_depth levels are done or the set outgrows max_reach.
    Returns (level of every node or -1, overflowed, sizes [max_depth])."""
    level = np.full(g.n, -1, np.int64)
    level[target] = 0
    cur, reach, sizes, overflow = np.array([target], np.int64), 1, [], False
    for d in range(1, max_depth + 1):
        if cur.size == 0:
            break
        new = np.unique(g.arcs(cur, mirrored(direction), allowed))
        new = new[level[new] < 0]
        reach += new.size
        if max_reach is not None and reach > max_reach:
            overflow = True
            sizes.append(max_reach + 1)
            break
        level[new] = d
        sizes.append(reach)
        cur = new
        if level[source] >= 0:
            break
    sizes += [0 if overflow else reach] * (max_depth - len(sizes))
    return level, overflow, sizes


def lexicographic(g, source, target, max_depth, direction=DIR_OUT, allowed=()):
    """the lexicographically smallest shortest path: levels from the target, then from the source always the smallest neighbour one
    level closer"""
    if source == target:
        return [int(source)]
    level, _, _ = backward_levels(g, source, target, max_depth, direction, allowed)
    if level[source] < 0:
        return []
    off, nbr = g.plan(direction, allowed)
    path, c = [int(source)], int(source)
    while c != target:
        row = nbr[off[c]:off[c + 1]]
        c = int(row[level[row] == level[c] - 1].min())
        path.append(c)
    return path


def answer(g, source, target, max_depth, direction=DIR_OUT, allowed=(), max_reach=16384):
    """what hvx_shortest_path_batch reports for one request: (path, status, sizes [max_depth])"""
    if source == NO_NODE or target == NO_NODE:
        return [], OK, [0] * max_depth
    if source == target:
        return [int(source)], OK, [1] * max_depth
    _, overflow, sizes = backward_levels(g, source, target, max_depth, direction, allowed, max_reach)
    if overflow:
        return [], ERR_CANDIDATE_LIMIT, sizes
    return literal(g, source, target, max_depth, direction, allowed), OK, sizes


def answers(g, sources, targets, max_depth, direction=DIR_OUT, allowed=(), max_reach=16384):
    """the batch: ([paths], statuses u32 [b], sizes u64 [b][max_depth])"""
    out = [answer(g, int(s), int(t), max_depth, direction, allowed, max_reach) for s, t in zip(sources, targets)]
    return ([p for p, _, _ in out], np.array([s for _, s, _ in out], np.uint32),
            np.array([z for _, _, z in out], np.uint64).reshape(len(out), max_depth))
