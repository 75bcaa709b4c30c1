"""The definition of zero-shot labelling (include/vq_amd.h, vq_index_label_rows) restated in numpy, shared by
tests/test_label_rows.py (over the C oracle's distances) and tests/test_label_rows_cpu.py (over hand-made distances)."""
import numpy as np


def distances(stored, prompts):
    """D [P][n]: knn_oracle.distances of every prompt to every exported row (the plain search's fp32 distance)."""
    from oracle import knn_oracle
    stored = np.ascontiguousarray(stored, dtype=np.float32)
    return np.stack([knn_oracle.distances(stored, p) for p in np.ascontiguousarray(prompts, dtype=np.float32)])


def row_labels(D, max_dist=np.inf):
    """D float32 [P][n] -> (L int32 [n], best float32 [n]): the smallest (d, j) per row; best > max_dist unlabels."""
    D = np.asarray(D, dtype=np.float32)
    L = np.argmin(D, axis=0).astype(np.int32)                 # the first of equal minima: the smaller j
    best = D[L, np.arange(D.shape[1])]
    return np.where(best > np.float32(max_dist), np.int32(-1), L).astype(np.int32), best


def group_tags(L, best, groups, tie, n_groups, m):
    """groups: dense label per row, tie: per row.  -> tags, votes, show rows int32 [G][m] (-1 / 0 / -1 unused), unlabelled [G]"""
    L, groups, tie = np.asarray(L), np.asarray(groups), np.asarray(tie)
    tags = np.full((n_groups, m), -1, dtype=np.int32)
    votes = np.zeros((n_groups, m), dtype=np.int32)
    show = np.full((n_groups, m), -1, dtype=np.int32)
    unl = np.zeros(n_groups, dtype=np.int32)
    for g in range(n_groups):
        rows = np.flatnonzero(groups == g)
        lab = L[rows]
        unl[g] = int((lab < 0).sum())
        count = np.bincount(lab[lab >= 0]) if (lab >= 0).any() else np.zeros(0, dtype=np.int64)
        order = sorted(np.flatnonzero(count).tolist(), key=lambda j: (-count[j], j))[:m]
        for t, j in enumerate(order):
            mine = rows[lab == j]
            tags[g, t], votes[g, t] = j, count[j]
            show[g, t] = min(mine.tolist(), key=lambda r: (best[r], tie[r]))
    return tags, votes, show, unl
