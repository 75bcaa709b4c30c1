"""SimpleVideoIndex drives its device matrix through searches, adds and a removal in one life: every answer against the numpy
restatements of the families' own suites over the embeddings and metadata the index holds at that moment.  Small on purpose
(3 videos x 40 frames, dim 64): what can go wrong here is the bookkeeping between the calls — ids that stay -position, ranks
cleared by an add and kept by a removal, labels and positions that follow the rows — not a kernel."""
import math

import numpy as np
import pytest

from oracle import knn_oracle
from test_distinct_search import greedy_distinct, video_rows
from test_sequence_search import dense_labels, sequence_answer
from test_set_search import _expected as set_answer


def _unit_query(q):
    return (q / (np.linalg.norm(q) + 1e-10)).astype(np.float32)


class _Truth:
    """What the index holds now, as the restatements want it."""

    def __init__(self, sv):
        self.md = sv.metadata
        self.stored = np.stack(sv.embeddings)
        self.names = [md["video_name"] for md in sv.metadata]
        self.positions = [int(round(md["timestamp"] * 1000)) for md in sv.metadata]
        self.labels, self.keys = dense_labels(self.names)
        self.tie = -np.arange(len(self.names))                   # search's tie rule: the larger position first

    def order(self, q):
        dist = knn_oracle.distances(self.stored, _unit_query(q))
        return np.argsort(-dist, kind="stable")[::-1].tolist(), dist      # the reference's reversed argsort of the similarities

    def frames(self, rows, dist):
        return [dict(self.md[r], score=float(np.float32(1.0) - dist[r])) for r in rows]


def _check_search(sv, q, k):
    t = _Truth(sv)
    order, dist = t.order(q)
    assert order == np.lexsort((t.tie, dist)).tolist()
    got = sv.search(q, k)
    assert got == t.frames(order[:k], dist)
    return order, dist


def _check_moments(sv, q, k, gap_s):
    t = _Truth(sv)
    order, dist = t.order(q)
    want = greedy_distinct(order, t.names, t.positions, k, math.ceil(gap_s * 1000))
    assert sv.search_moments(q, k, gap_s) == t.frames(want, dist), gap_s
    return want, order


@pytest.mark.gpu
def test_searches_adds_and_a_removal_interleaved(gpu_lib):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    vecs, video, frame = video_rows(120, 64, seed=1201, lengths=[40])
    for a, b in ((3, 47), (3, 95), (10, 60), (11, 100), (12, 101), (55, 110), (20, 21), (70, 69)):
        vecs[b] = vecs[a]                                         # eight exact duplicates, across and inside videos: ties decide
    sv = SimpleVideoIndex()
    for e, v, f in zip(vecs, video, frame):
        sv.add_frame(e, f"v{v}.mp4", f * 0.5)
    q = vecs[3] * np.float32(3.0)                                 # bit-equal distances to frames 3, 47 and 95
    # 1, 2: a plain search (no ranks on the device), then moments (ranks, labels and positions uploaded)
    order, dist = _check_search(sv, q, 10)
    assert order[:3] == [95, 47, 3] and dist[95] == dist[47] == dist[3]
    want, order = _check_moments(sv, q, 10, 1.0)
    assert want != order[:10]                                     # the gap dropped a neighbour
    dev = sv._dev
    # 3, 4: five frames of a new video, one more duplicate among them; the plain search orders ties on the host again
    for i in range(5):
        sv.add_frame(vecs[3] if i == 2 else vecs[30 + i] + np.float32(0.01), "v3.mp4", i * 0.5)
    order, _ = _check_search(sv, q, 10)
    assert order[:4] == [122, 95, 47, 3] and sv._dev is dev and sv._pushed == 125
    # 5, 6: the middle video goes; the ids stay -position, the ranks stay valid, labels and positions follow the rows
    assert sv.remove_video("v1.mp4") == 40 and sv._dev is dev and sv._pushed == 85
    assert dev._ids == [-i for i in range(85)] and dev._row_of == {-i: i for i in range(85)} and dev.size() == 85
    for gap_s in (0.0, 1.0, 1000.0):
        want, order = _check_moments(sv, q, 6, gap_s)
    assert len(want) == 3 and order[:3] == [82, 55, 3]            # one moment per video; v2's duplicate moved from 95 to 55
    # 7: a storyboard of three stored frames of v2.mp4, a second apart, the first a duplicate of a frame of v0.mp4
    t = _Truth(sv)
    steps = [vecs[100] * np.float32(2.0), vecs[102], vecs[104]]
    step_dist = [knn_oracle.distances(t.stored, _unit_query(s)) for s in steps]
    for max_gap_s, min_gap_s in ((3.0, 0.0), (1.0, 1.0), (0.4, 0.0)):
        lo, hi = max(1, math.ceil(min_gap_s * 1000)), math.floor(max_gap_s * 1000)
        want, _, _ = sequence_answer(step_dist, t.labels, t.positions, t.tie, lo, hi, 3)
        got = sv.search_storyboard(steps, 3, max_gap_s, min_gap_s)
        assert got == [{"video_name": t.keys[g], "score": float(np.float32(1.0) - d), "timestamps": [t.md[r]["timestamp"] for r in c],
                        "frame_ids": [t.md[r]["frame_id"] for r in c]} for g, d, c in want], (max_gap_s, min_gap_s)
    assert sv.search_storyboard(steps, 3, 3.0)[0]["video_name"] == "v2.mp4" and sv.search_storyboard(steps, 3, 0.4) == []
    # 8: more like v0.mp4, among the videos left
    g0 = t.keys.index("v0.mp4")
    want = set_answer(t.stored, t.stored[t.labels == g0], t.labels.astype(np.int64), np.arange(85), 3, set(range(len(t.keys))) - {g0})
    got = sv.similar_videos("v0.mp4", 3)
    assert got == [{"video_name": t.keys[g], "score": float(np.float32(1.0) - d)} for g, d, _ in want] and len(got) == 2
    # ... and the plain search and the moments once more, on the index as all of that left it
    _check_search(sv, q, 10)
    _check_moments(sv, q, 10, 2.0)
    assert sv._dev is dev
