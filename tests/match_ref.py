"""The definition of shared-footage search (include/vq_amd.h, vq_index_match_runs) restated in numpy, shared by
tests/test_match_runs.py (over the C oracle's distances on the exported rows) and tests/test_match_runs_cpu.py (hand-made
distance tables).  Everything here works on a distance table ``dist`` [m][n] float32 — d(i, r) as vq_index_search reports it —
and integers; the only floating-point arithmetic is the fp32 comparison with max_dist and the fp64 chain of mean_dist."""
import numpy as np

EMPTY = dict(group=-1, hits=0, span=0, q_first=-1, row_first=-1, row_last=-1, mean_dist=np.float32(np.inf))


def order_of(rows, pos, tie):
    """The rows of a group in ascending (position, tie) order.  pos / tie: per row of the index."""
    return sorted((int(r) for r in rows), key=lambda r: (int(pos[r]), int(tie[r])))


def hit_table(dist, max_dist):
    """hit(i, r): d(i, r) <= max_dist in fp32, inclusive; a NaN distance never hits."""
    with np.errstate(invalid="ignore"):
        return np.asarray(dist, dtype=np.float32) <= np.float32(max_dist)


def diagonal_runs(cells, max_miss):
    """cells: the hit flags of one diagonal by ascending i (index 0 = its first cell).  -> [(first, last, hits)] of its runs: cut at
    every stretch of more than max_miss consecutive non-hits, each piece trimmed to its first and last hit."""
    idx = np.flatnonzero(cells)
    if len(idx) == 0:
        return []
    cuts = np.flatnonzero(np.diff(idx) - 1 > max_miss)               # a gap of more than max_miss misses behind hit number c
    starts = np.concatenate([[0], cuts + 1])
    ends = np.concatenate([cuts, [len(idx) - 1]])
    return [(int(idx[a]), int(idx[b]), int(b - a + 1)) for a, b in zip(starts, ends)]


def group_runs(hit, order, min_len, max_miss):
    """Every run of one group with at least min_len hits, as (hits, span, delta, s).  hit [m][n] bool; order: the group's rows in
    (position, tie) order."""
    m, L = hit.shape[0], len(order)
    H = hit[:, np.asarray(order, dtype=np.int64)] if L else np.zeros((m, 0), dtype=bool)
    ii, jj = np.nonzero(H)
    out = []
    for delta in np.unique(jj - ii).tolist():                        # diagonals without a hit hold no run
        i0, i1 = max(0, -delta), min(m - 1, L - 1 - delta)
        i = np.arange(i0, i1 + 1)
        for first, last, hits in diagonal_runs(H[i, i + delta], max_miss):
            if hits >= min_len:
                out.append((hits, last - first + 1, delta, i0 + first))
    return out


def best_run(hit, order, min_len, max_miss):
    """The group's run with the smallest (-hits, span, delta, s), or None."""
    runs = group_runs(hit, order, min_len, max_miss)
    return min(runs, key=lambda r: (-r[0], r[1], r[2], r[3])) if runs else None


def run_slot(dist, hit, order, g, run):
    """The answer's slot for group g's best run."""
    hits, span, delta, s = run
    total = 0.0
    last_row = -1
    for i in range(s, s + span):                                     # the fp64 chain over the hit cells, i ascending
        r = order[i + delta]
        if hit[i, r]:
            total = total + float(dist[i][r])
            last_row = r
    return dict(group=g, hits=hits, span=span, q_first=s, row_first=order[s + delta], row_last=last_row,
                mean_dist=np.float32(np.float64(total) / np.float64(hits)))


def answer(dist, labels, pos, tie, max_dist, min_len, max_miss, k, allowed=None):
    """-> (the k slots in the C layout, unused ones EMPTY; the number of allowed groups with a run)."""
    dist = np.asarray(dist, dtype=np.float32)
    labels = np.asarray(labels)
    hit = hit_table(dist, max_dist)
    found = []
    for g in range(int(labels.max()) + 1 if len(labels) else 0):
        if allowed is not None and g not in allowed:
            continue
        order = order_of(np.flatnonzero(labels == g), pos, tie)
        run = best_run(hit, order, min_len, max_miss)
        if run is not None:
            found.append((g, run, order))
    found.sort(key=lambda t: (-t[1][0], t[1][1], t[0]))
    slots = [run_slot(dist, hit, order, g, run) for g, run, order in found[:k]]
    return slots + [dict(EMPTY) for _ in range(k - len(slots))], len(found)


def as_arrays(slots):
    """The slots as the seven arrays of the C call."""
    ints = {name: np.array([s[name] for s in slots], dtype=np.int32) for name in ("group", "hits", "span", "q_first", "row_first", "row_last")}
    ints["mean_dist"] = np.array([s["mean_dist"] for s in slots], dtype=np.float32)
    return ints
