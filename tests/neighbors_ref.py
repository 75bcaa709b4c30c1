"""Library neighbours (vq_index_neighbors) restated in numpy over the C oracle's distances, and the main fixture of
tests/test_neighbors.py.  TEST INFRASTRUCTURE ONLY.

The definition (include/vq_amd.h): for an asked row r the eligible set is S(r) = {c != r} (exclude = 0) or {c : group(c) !=
group(r)} (exclude = 1); line r holds the first min(k, |S(r)|) rows of S(r) by (d(r, c), tie(c)) ascending, d by the oracle's
fixed-order fp64 chain with the stored row r as the query, tie the row number or the id rank; unused slots are -1 / +inf."""
import numpy as np

from oracle import knn_oracle


def distance_table(stored, rows=None):
    """The oracle's distances d[i][c] of asked row rows[i] (None: every row) to every stored row c."""
    stored = np.ascontiguousarray(stored, dtype=np.float32)
    rows = range(len(stored)) if rows is None else rows
    return np.stack([knn_oracle.distances(stored, stored[r]) for r in rows]) if len(stored) else np.empty((0, 0), np.float32)


def eligible(n, rows, groups):
    """bool [m][n]: may column c appear in the line of asked row rows[i]?  groups None: every row but the row itself."""
    rows = np.asarray(rows, dtype=np.int64)
    if groups is None:
        return np.arange(n)[None, :] != rows[:, None]
    groups = np.asarray(groups)
    return groups[None, :] != groups[rows][:, None]


def neighbors(stored, k, *, rows=None, groups=None, tie=None, table=None):
    """(ids int32 [m][k], dist float32 [m][k]) of the definition.  table: distance_table(stored, rows), when the caller has it."""
    n = len(stored)
    rows = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    d = distance_table(stored, rows) if table is None else table
    ok = eligible(n, rows, groups)
    tie = np.arange(n) if tie is None else np.asarray(tie)
    ids = np.full((len(rows), k), -1, dtype=np.int32)
    dist = np.full((len(rows), k), np.inf, dtype=np.float32)
    for i in range(len(rows)):
        order = np.lexsort((tie, d[i]))
        order = order[ok[i][order]][:k]
        ids[i, :len(order)] = order
        dist[i, :len(order)] = d[i][order]
    return ids, dist


def brute_force(stored, k, rows, groups=None, tie=None):
    """The same by a double loop over python floats of the oracle's distances: what `neighbors` is checked against."""
    n = len(stored)
    out_i, out_d = [], []
    for r in rows:
        d = knn_oracle.distances(stored, stored[r])
        cand = []
        for c in range(n):
            if (c == r) if groups is None else (groups[c] == groups[r]):
                continue
            cand.append((float(d[c]), int(c if tie is None else tie[c]), c))
        cand.sort()
        cand = cand[:k]
        out_i.append([c for _, _, c in cand] + [-1] * (k - len(cand)))
        out_d.append([np.float32(x) for x, _, _ in cand] + [np.float32(np.inf)] * (k - len(cand)))
    return np.array(out_i, dtype=np.int32).reshape(len(rows), k), np.array(out_d, dtype=np.float32).reshape(len(rows), k)


def close_gap_rows(table, ok, k, width, below=None):
    """How many asked rows have their k-th and `below`-th (default k + 1) largest eligible SCORES (1 - d) closer than `width`.
    below = k + 1: the rows whose rank k no bound of a quarter of `width` can separate from rank k + 1 by the scores alone.
    below = C + 1 (the re-score's candidate count + 1): the rows whose proof cannot close, because the best key outside the
    candidates is not a bound's width below the k-th exact score."""
    below = k + 1 if below is None else below
    count = 0
    for d, e in zip(table, ok):
        s = np.sort(1.0 - d[e].astype(np.float64))[::-1]
        if len(s) >= below and s[k - 1] - s[below - 1] < width:
            count += 1
    return count


# ---- the main fixture: dim 256, 2,341 rows = two 2,048-row ranges (the second ragged) and ten 256-row resident tiles (the last
# holds 37 rows) ----
MAIN_N, MAIN_DIM, MAIN_SEED = 2341, 256, 20260611
CLUSTER = 40


def main_groups():
    """Group label per row: a 1-row group; two groups interleaved row by row; a 300-row contiguous group that covers the whole
    tile of rows 256 .. 511 (every score of that diagonal tile is struck); 58 groups of 25 rows; a group straddling rows
    2,047 | 2,048; a last group ending in the ragged tile."""
    g = np.empty(MAIN_N, dtype=np.int64)
    g[0] = 0
    g[1:250] = 2 + (np.arange(1, 250) & 1)          # groups 2 and 3, row by row
    g[250:550] = 1
    g[550:2000] = 4 + (np.arange(1450) // 25)       # groups 4 .. 61
    g[2000:2100] = 62
    g[2100:] = 63
    return g


def main_fixture(seed=MAIN_SEED):
    """(vectors fp32 [n][dim] as handed to add_batch, groups [n], ids [n] as strings f"video{g}_{i}", plants): unit Gaussian
    rows plus
      - 12 rows copied bit for bit into another group, 4 within their own group, one triple across three groups;
      - a cluster of 40 rows in 40 different groups, pairwise within 1e-5 in score: inside the scan's error bound."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((MAIN_N, MAIN_DIM)).astype(np.float32)
    g = main_groups()
    cross = [(5, 300), (6, 301), (260, 10), (400, 2050), (560, 900), (600, 2330), (2047, 1000), (2048, 700), (2340, 3), (2310, 130),
             (1500, 0), (1999, 2000)]                # (source, copy): different groups
    within = [(251, 549), (2001, 2099), (2101, 2339), (12, 14)]     # the same group (12 and 14: both in the interleaved group 2)
    triple = (1234, 21, 520)                 # rows 21 < 520, ids "video3_10" > "video1_270": the two tie orders differ
    for s, c in cross + within:
        v[c] = v[s]
    v[triple[1]] = v[triple[0]]
    v[triple[2]] = v[triple[0]]
    cluster = [550 + 25 * i + 7 for i in range(CLUSTER)]            # one row in each of the groups 4 .. 43
    base = rng.standard_normal(MAIN_DIM)
    base /= np.linalg.norm(base)
    for r in cluster:
        v[r] = (base + 1e-4 * rng.standard_normal(MAIN_DIM)).astype(np.float32)
    within_pos = np.zeros(MAIN_N, dtype=np.int64)
    seen = {}
    for r in range(MAIN_N):
        within_pos[r] = seen.get(g[r], 0)
        seen[g[r]] = within_pos[r] + 1
    ids = [f"video{g[r]}_{within_pos[r]}" for r in range(MAIN_N)]   # "video1_10" sorts before "video1_2"
    plants = {"cross": cross, "within": within, "triple": triple, "cluster": cluster}
    return v, g, ids, plants
