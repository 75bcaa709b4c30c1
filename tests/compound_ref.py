"""The definition of the compound search (include/vq_amd.h, vq_index_search_compound) restated in numpy, shared by
tests/test_compound_search.py (over the C oracle's distances, ``label_ref.distances``) and tests/test_compound_search_cpu.py
(over hand-made distances)."""
import numpy as np


def row_distance(D_terms, clause_of):
    """D_terms float32 [m][n], clause_of [m] (clause number or -1) -> D float32 [n]: max over the clauses of the min over a
    clause's terms.  float32 compares only: no arithmetic."""
    D_terms = np.asarray(D_terms, dtype=np.float32)
    clause_of = np.asarray(clause_of)
    clauses = sorted(set(int(c) for c in clause_of if c >= 0))
    assert clauses == list(range(len(clauses))) and clauses, "clause numbers 0 .. C-1, C >= 1"
    return np.max(np.stack([np.min(D_terms[clause_of == c], axis=0) for c in clauses]), axis=0)


def struck(D_terms, clause_of, margin):
    """bool [n]: some veto term j has d(j, r) < float32(D(r) + margin) — one float32 addition, a strict compare."""
    D_terms = np.asarray(D_terms, dtype=np.float32)
    clause_of = np.asarray(clause_of)
    D = row_distance(D_terms, clause_of)
    with np.errstate(over="ignore", invalid="ignore"):
        lim = (D + np.float32(margin)).astype(np.float32)
    out = np.zeros(D.shape, dtype=bool)
    for j in np.flatnonzero(clause_of < 0):
        out |= D_terms[j] < lim
    return out


def compound_answer(D_terms, clause_of, margin, tie, k):
    """-> (rows int32 [k], dist float32 [k], term_dist float32 [k][m]): the first k rows that are not struck by (D, tie)
    ascending; unused slots are -1 / inf / inf."""
    D_terms = np.asarray(D_terms, dtype=np.float32)
    m, n = D_terms.shape
    D = row_distance(D_terms, clause_of)
    keep = np.flatnonzero(~struck(D_terms, clause_of, margin))
    order = keep[np.lexsort((np.asarray(tie)[keep], D[keep]))][:k]
    rows = np.full(k, -1, dtype=np.int32)
    dist = np.full(k, np.inf, dtype=np.float32)
    term_dist = np.full((k, m), np.inf, dtype=np.float32)
    rows[:len(order)] = order
    dist[:len(order)] = D[order]
    term_dist[:len(order)] = D_terms[:, order].T
    return rows, dist, term_dist
