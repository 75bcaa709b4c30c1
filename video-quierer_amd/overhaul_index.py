"""Drop-in for the live system's brute-force index, ``SimpleVideoIndex``
(reference video_search_overhaul.py:23-106) — SURVEY.md §8f "next" #2 — on the
same device scan as indexes.hnsw:

* ``add_frame(embedding, video_name, timestamp)`` appends the embedding AS GIVEN
  (the reference does not normalise stored rows, :31-38);
* ``search(query, k)`` = top-k of ``E @ (q / (||q|| + 1e-10))`` in descending
  similarity, ``np.argsort(sim)[::-1][:k]`` (:40-64), i.e. ties resolve to the
  LARGER frame id; results are the metadata dicts plus ``'score'`` (float);
* ``save_to_disk`` / ``load_from_disk`` keep the reference's pickle layout
  ``{embeddings, metadata, video_hashes, version}`` (:66-106).

Scores come back as ``1 - (1 - dot)`` from the distance the scan returns, so
they equal the reference's fp32 dot to ~1e-7 (not bit-for-bit).  Rows are pushed
to the GPU lazily, at the first search after an add.
"""
from __future__ import annotations

import logging
import math
import pickle
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np

from video_quierer_amd import _lib
from video_quierer_amd.indexes.hnsw import MODE_AUTO, HNSWIndex, host_tie_order

logger = logging.getLogger(__name__)


def _unit_query(q) -> np.ndarray:
    q = np.asarray(q)
    return (q / (np.linalg.norm(q) + 1e-10)).astype(np.float32)          # reference :50-51


class SimpleVideoIndex:
    def __init__(self):
        self.embeddings: List[np.ndarray] = []
        self.metadata: List[Dict] = []
        self.video_hashes: Dict = {}
        self._dev = None          # HNSWIndex used as the raw device matrix; its ids are -position (see _sync_device)
        self._pushed = 0
        self._ranked_dev = None   # the device matrix that holds the id ranks of all its rows (_device)
        # one callable each for the index's life: the device matrix keeps its labels and positions while they stay the same
        self._group_fn = self._video_of_row_id
        self._pos_fn = self._timestamp_ms_of_row_id

    def add_frame(self, embedding: np.ndarray, video_name: str, timestamp: float):
        self.embeddings.append(embedding.astype(np.float32))
        self.metadata.append({"video_name": video_name, "timestamp": timestamp,
                              "frame_id": len(self.embeddings) - 1})

    def _sync_device(self) -> None:
        n = len(self.embeddings)
        if self._dev is not None and self._pushed > n:      # list was replaced/shrunk: rebuild
            self._dev.close()
            self._dev, self._pushed = None, 0
        if n == self._pushed:
            return
        block = np.ascontiguousarray(np.vstack(self.embeddings[self._pushed:]), dtype=np.float32)
        if self._dev is None:
            self._dev = HNSWIndex(dimension=block.shape[1])
        # stored as given; ids = -frame position: the scan's (distance, id) tie rule then yields the larger frame first,
        # like the reference's reversed argsort
        self._dev._append_stored(block, [-i for i in range(self._pushed, n)])
        self._pushed = n
        if self._ranked_dev is self._dev:
            # the id ranks no longer cover the index, and `search` orders ties on the host
            _lib.check(_lib.load().vq_index_set_id_ranks(self._dev._h, None, 0))
            self._ranked_dev = None

    def _device(self, ranks: bool = False) -> HNSWIndex:
        """The device matrix with every frame pushed.  ``ranks``: with the id order (larger frame first, as `search` orders
        ties) as ranks on the device, where the grouped families run their walks.  A removal keeps them (a stable
        compaction), an add clears them (_sync_device), a reloaded or rebuilt index is another device matrix."""
        self._sync_device()
        dev = self._dev
        # rows are stored as given: the library measures |row|^2 of what it holds and only takes its fp16 scan
        # while the matrix is near-unit (include/vq_amd.h vq_index_add), so un-normalised embeddings stay exact
        dev.search_mode = MODE_AUTO
        if ranks and self._ranked_dev is not dev:
            with dev.lock:
                dev._sync_tie_order()
            self._ranked_dev = dev
        return dev

    def remove_video(self, video_name: str) -> int:
        """Drop one video: its embeddings, metadata and ``video_hashes`` entry (so the next scan of the library re-processes
        it, video_search_overhaul.py:391-402, without its old frames staying behind).  Frames already on the device are
        removed there in place (vq_index_remove_rows); the surviving metadata dicts stay as stored, ``frame_id`` included.
        Returns the number of frames removed."""
        self.video_hashes.pop(video_name, None)
        pos = [i for i, md in enumerate(self.metadata) if md.get("video_name") == video_name]
        if not pos:
            return 0
        on_dev = np.array([i for i in pos if i < self._pushed], dtype=np.int64)
        if self._dev is not None and len(on_dev):
            with self._dev.lock:
                # before the lists shrink: the removal labels the rows added since the last grouped search, by their old positions
                self._dev._remove_rows(on_dev)
                # rows keep their order, so the ids stay -position (the tie rule of search) without new ranks
                self._pushed -= len(on_dev)
                self._dev._replace_ids([-i for i in range(self._pushed)])
        gone = set(pos)
        self.embeddings = [e for i, e in enumerate(self.embeddings) if i not in gone]
        self.metadata = [md for i, md in enumerate(self.metadata) if i not in gone]
        return len(pos)

    def search(self, query_embedding: np.ndarray, k: int = 5) -> List[Dict]:
        if not self.embeddings:
            return []
        dev = self._device()
        unit = np.ascontiguousarray(_unit_query(query_embedding)[None, :])
        n = len(self.embeddings)
        # ties on the host: no ranks are kept on the device for this search (an add would have to upload them again)
        best = host_tie_order(lambda fetch: dev._raw_search(unit, fetch), min(k, n), n, lambda row: -row)[0]
        results = []
        for d, neg in best:
            md = self.metadata[-neg].copy()
            md["score"] = float(np.float32(1.0) - d)
            results.append(md)
        return results

    def _video_of_row_id(self, node_id: int) -> str:
        return self.metadata[-node_id]["video_name"]          # device ids are -position (see _sync_device)

    def _timestamp_ms_of_row_id(self, node_id: int) -> int:
        return int(round(self.metadata[-node_id]["timestamp"] * 1000))

    def search_moments(self, query_embedding: np.ndarray, k: int = 5, min_gap_s: float = 2.0) -> List[Dict]:
        """The k best distinct moments: ``search``'s exhaustive list (the same normalisation, scores and tie order), walked in
        order, with every frame dropped that lies less than ``min_gap_s`` seconds from an already kept frame of the same video
        (``HNSWIndex.search_distinct``: exact).  Positions are ``round(timestamp * 1000)`` ms, the gap ``ceil(min_gap_s *
        1000)`` ms, groups the video names.  Results are ``search``'s dicts ``{'video_name', 'timestamp', 'frame_id', 'score'}``."""
        if min_gap_s < 0:
            raise ValueError(f"min_gap_s must be >= 0, got {min_gap_s}")
        if not self.embeddings:
            return []
        dev = self._device(ranks=True)
        unit = np.ascontiguousarray(_unit_query(query_embedding)[None, :])
        with dev.lock:                                # the query as normalised above, not normalised again
            res = dev._distinct_many(unit, k, int(math.ceil(min_gap_s * 1000)), self._group_fn, self._pos_fn, given=True)[0]
        results = []
        for r in res:
            md = self.metadata[-r["id"]].copy()
            md["score"] = float(r["score"])
            results.append(md)
        return results

    def search_diverse(self, query_embedding: np.ndarray, k: int = 5, max_similarity: float = 0.95) -> List[Dict]:
        """The k best frames no two of which look alike: ``search``'s exhaustive list (the same normalisation, dicts and tie
        order), walked in order, with every frame dropped whose cosine similarity to an already kept frame is above
        ``max_similarity`` (``HNSWIndex.search_diverse`` with ``min_dist = float32(1) - float32(max_similarity)``: exact)."""
        if not max_similarity <= 1:                               # (NaN too)
            raise ValueError(f"max_similarity must be <= 1, got {max_similarity}")
        if not self.embeddings:
            return []
        dev = self._device(ranks=True)
        unit = np.ascontiguousarray(_unit_query(query_embedding)[None, :])
        with dev.lock:                                # the query as normalised above, not normalised again
            res = dev._diverse_many(unit, k, np.float32(1) - np.float32(max_similarity), given=True)[0]
        results = []
        for r in res:
            md = self.metadata[-r["id"]].copy()
            md["score"] = float(r["score"])
            results.append(md)
        return results

    def search_compound(self, all_of, k: int = 5, none_of=(), margin: float = 0.0) -> List[Dict]:
        """The k best frames that match ALL of several prompts and none of the vetoed ones ("a dog AND a beach, NOT at night";
        text prompts through ``extract_text_features``): ``search``'s dicts, ``'score'`` being the similarity of the frame's
        WORST clause, plus ``'term_scores'`` (the frame's similarity to every vector: ``all_of``'s in order, then
        ``none_of``'s).  An entry of ``all_of`` is one vector or a sequence of alternatives; a frame is dropped when a
        ``none_of`` vector scores above the frame's score minus ``margin`` (``HNSWIndex.search_compound``: exact).  Every
        vector is normalised as ``search`` does; ties between frames as ``search``."""
        terms, clause_of = HNSWIndex._compound_terms(all_of, none_of)
        mg = np.float32(margin)
        if mg != mg:
            raise ValueError("margin is NaN")
        if not self.embeddings or k <= 0:
            return []
        dev = self._device(ranks=True)
        unit = np.ascontiguousarray(np.stack([_unit_query(q) for q in terms]))
        with dev.lock:                                # the terms as normalised above, not normalised again
            res = dev._compound(unit, clause_of, k, mg, given=True)
        results = []
        for r in res:
            md = self.metadata[-r["id"]].copy()
            md["score"] = float(r["score"])
            md["term_scores"] = [float(np.float32(1.0) - d) for d in r["term_distances"]]
            results.append(md)
        return results

    def search_storyboard(self, step_embeddings, k: int = 5, max_gap_s: float = 10.0, min_gap_s: float = 0.0) -> List[Dict]:
        """The k videos that show the steps IN ORDER (text prompts through ``extract_text_features``, or the frames of a clip):
        ``[{'video_name', 'score', 'timestamps', 'frame_ids'}]``, best first.  One frame of the video per step, each
        ``min_gap_s`` .. ``max_gap_s`` seconds after the one before (``HNSWIndex.search_sequence``: exact; ``score`` is one
        minus the mean distance along the video's cheapest such chain, videos without a chain do not appear).  Every step is
        normalised as ``search`` does; positions are ``round(timestamp * 1000)`` ms, the gaps ``max(1, ceil(min_gap_s *
        1000))`` and ``floor(max_gap_s * 1000)`` ms, groups the video names; ties between frames as ``search``."""
        steps = list(step_embeddings)
        if not steps:
            raise ValueError("search_storyboard needs at least one step")
        if len(steps) > HNSWIndex.SEQ_MAX_STEPS:
            raise ValueError(f"a storyboard holds at most {HNSWIndex.SEQ_MAX_STEPS} steps, got {len(steps)}")
        if min_gap_s < 0 or max_gap_s < min_gap_s:
            raise ValueError(f"the gaps must satisfy 0 <= min_gap_s <= max_gap_s, got {min_gap_s}, {max_gap_s}")
        lo, hi = max(1, int(math.ceil(min_gap_s * 1000))), int(math.floor(max_gap_s * 1000))
        if hi < lo:
            raise ValueError(f"max_gap_s {max_gap_s} leaves no admissible gap in whole milliseconds")
        if not self.embeddings or k <= 0:
            return []
        dev = self._device(ranks=True)
        unit = np.ascontiguousarray(np.stack([_unit_query(q) for q in steps]))
        with dev.lock:                                # the steps as normalised above, not normalised again
            res = dev._search_sequence(unit, k, lo, hi, None, self._group_fn, self._pos_fn, given=True)
        return [{"video_name": r["group"], "score": float(r["score"]),
                 "timestamps": [self.metadata[-i]["timestamp"] for i in r["chain"]],
                 "frame_ids": [self.metadata[-i]["frame_id"] for i in r["chain"]]} for r in res]

    def search_spans(self, query_embedding: np.ndarray, k: int = 5, min_similarity: float = 0.25, max_gap_s: Optional[float] = None,
                     max_len_s: Optional[float] = None) -> List[Dict]:
        """Where in which video does the query happen, from when to when: ``[{'video_name', 'start', 'end', 'peak', 'frames',
        'score', 'mass'}]``, the k videos with the best time span, best first.  A frame adds its similarity above
        ``min_similarity`` to a span and costs it what it lacks; a span is a run of consecutive frames of one video, neighbours
        at most ``max_gap_s`` seconds apart and the whole at most ``max_len_s`` long (``None``: no limit), and a video answers
        with its span of the largest sum (``mass``; ``HNSWIndex.search_spans`` with ``max_distance = float32(1) -
        float32(min_similarity)``: exact).  ``start`` / ``end`` / ``peak`` are the timestamps in seconds of the span's first,
        last and best frame, ``frames`` the number of frames in it, ``score`` their mean similarity.  The query is normalised
        as ``search`` does; positions are ``round(timestamp * 1000)`` ms, the limits ``floor(x * 1000)`` ms, groups the video
        names; ties between frames as ``search``."""
        tau = np.float32(1) - np.float32(min_similarity)
        if tau != tau:
            raise ValueError("min_similarity is NaN")
        for name, x in (("max_gap_s", max_gap_s), ("max_len_s", max_len_s)):
            if x is not None and not x >= 0:                      # (NaN too)
                raise ValueError(f"{name} must be >= 0 or None, got {x}")
        gap = None if max_gap_s is None else int(math.floor(max_gap_s * 1000))
        span = None if max_len_s is None else int(math.floor(max_len_s * 1000))
        tau, gap, span = HNSWIndex._span_args(tau, gap, span)
        if not self.embeddings or k <= 0:
            return []
        dev = self._device(ranks=True)
        unit = np.ascontiguousarray(_unit_query(query_embedding)[None, :])
        with dev.lock:                                # the query as normalised above, not normalised again
            res = dev._search_spans(unit, k, tau, gap, span, None, self._group_fn, self._pos_fn, given=True)[0]
        stamp = lambda i: self.metadata[-i]["timestamp"]
        return [{"video_name": r["group"], "start": stamp(r["start_id"]), "end": stamp(r["end_id"]), "peak": stamp(r["peak_id"]),
                 "frames": r["frames"], "score": r["score"], "mass": r["mass"]} for r in res]

    def similar_videos(self, video_name: str, k: int = 5, keyframes: Optional[int] = None) -> List[Dict]:
        """The k indexed videos most similar to ``video_name``, itself excluded: ``[{'video_name', 'score'}]``, best first.
        Every stored frame of the video takes its best match in the other video; ``score`` is the mean of those cosine
        scores (``HNSWIndex.similar_groups``: exact, a re-encode or a cut scores close to 1 where the reference's file-hash
        comparison, video_search_overhaul.py:143-147, sees two different files).  ``keyframes=m`` compares the video's m
        keyframes (``video_summary``) instead of all its frames, which also lifts the 4,096-frame limit.  ``KeyError`` for
        an unknown video."""
        if not self.embeddings:
            raise KeyError(video_name)
        res = self._device(ranks=True).similar_groups(video_name, k, group_of=self._group_fn, keyframes=keyframes)
        return [{"video_name": r["group"], "score": float(r["score"])} for r in res]

    def find_reuse(self, video_name: str, k: int = 5, min_similarity: float = 0.9, min_seconds: float = 3.0, max_miss: int = 1) -> List[Dict]:
        """The k indexed videos that contain footage of ``video_name`` (a re-upload, a trailer, a shared intro, a reused news
        clip), itself excluded, and where: ``[{'video_name', 'frames', 'score', 'start', 'end', 'query_start', 'query_end'}]``,
        the longest match first.  A frame of ``video_name`` matches a frame of another video when their cosine similarity is
        at least ``min_similarity``; a match is a stretch in which frame after frame of the one video matches frame after
        frame of the other, with at most ``max_miss`` consecutive frames in between that do not (``HNSWIndex.shared_runs_of``
        on the embeddings as stored: exact).  ``frames`` is the number of matching frames, ``score`` their mean similarity,
        ``start`` / ``end`` the timestamps of the match in the found video, ``query_start`` / ``query_end`` in ``video_name``.
        A match needs at least ``min_seconds`` of ``video_name``'s own frame interval worth of matching frames (at least one).
        Frames are taken in timestamp order (``round(timestamp * 1000)`` ms), ties between frames as ``search``.  ``KeyError``
        for an unknown video, ``ValueError`` for a video of more than 4,096 frames."""
        if not min_similarity <= 1:                               # (NaN too)
            raise ValueError(f"min_similarity must be <= 1, got {min_similarity}")
        if min_seconds < 0 or int(max_miss) < 0:
            raise ValueError(f"min_seconds and max_miss must be >= 0, got {min_seconds}, {max_miss}")
        stamps = sorted(md["timestamp"] for md in self.metadata if md.get("video_name") == video_name)
        if not stamps:
            raise KeyError(video_name)
        interval = (stamps[-1] - stamps[0]) / (len(stamps) - 1) if len(stamps) > 1 and stamps[-1] > stamps[0] else 1.0
        min_len = max(1, int(math.ceil(min_seconds / interval - 1e-9)))
        res = self._device(ranks=True).shared_runs_of(video_name, k, max_distance=np.float32(1) - np.float32(min_similarity), min_len=min_len,
                                                      max_miss=max_miss, group_of=self._group_fn, position_of=self._pos_fn)
        out = []
        for r in res:
            first, last = self.metadata[-r["first"]], self.metadata[-r["last"]]
            out.append({"video_name": r["group"], "frames": r["hits"], "score": float(r["score"]), "start": first["timestamp"],
                        "end": last["timestamp"], "query_start": stamps[r["query_first"]], "query_end": stamps[r["query_first"] + r["span"] - 1]})
        return out

    def find_reuse_warped(self, video_name: str, k: int = 5, min_similarity: Optional[float] = None, max_frames: Optional[int] = None) -> List[Dict]:
        """``find_reuse`` for footage at ANOTHER PACE — a re-upload at another frame rate, a slow-motion replay, a video sampled
        with other settings — where the matching frames leave the diagonal ``find_reuse`` reads: the k indexed videos that
        show ``video_name`` under a monotone time warp, itself excluded, ``[{'video_name', 'score', 'start', 'end'}]``, the
        best first.  Every frame of ``video_name``, in timestamp order, is paired with one or more consecutive frames of the
        other video (``HNSWIndex.align_group`` on the embeddings as stored: exact); ``score`` is the mean cosine similarity
        over ``video_name``'s frames along the best such pairing, ``start`` / ``end`` the timestamps in the found video where
        it begins and ends.  Videos whose score is below ``min_similarity`` do not appear (``None``: no limit).  ``KeyError``
        for an unknown video, ``ValueError`` for a video of more than 4,096 frames unless ``max_frames`` thins it out."""
        if min_similarity is not None and not min_similarity <= 1:    # (NaN too)
            raise ValueError(f"min_similarity must be <= 1, got {min_similarity}")
        if not any(md.get("video_name") == video_name for md in self.metadata):
            raise KeyError(video_name)
        max_distance = None if min_similarity is None else np.float32(1) - np.float32(min_similarity)
        res = self._device(ranks=True).align_group(video_name, k, max_distance, group_of=self._group_fn, position_of=self._pos_fn,
                                                   max_frames=max_frames)
        return [{"video_name": r["group"], "score": float(r["score"]), "start": self.metadata[-r["start_id"]]["timestamp"],
                 "end": self.metadata[-r["end_id"]]["timestamp"]} for r in res]

    def _other_video_neighbors(self, per_frame: int):
        """The library's neighbour table: for every stored frame its ``per_frame`` nearest frames of OTHER videos
        (``HNSWIndex.neighbors(other_groups=True)`` on the embeddings as stored: exact, ties between frames as ``search``).
        (rows int32 [n][per_frame], distances float32 [n][per_frame]); row r is frame r of ``metadata``."""
        return self._device(ranks=True).neighbors(per_frame, other_groups=True, group_of=self._group_fn)

    def related_videos(self, k: int = 5, per_frame: int = 3) -> Dict[str, List[Dict]]:
        """For every indexed video the k other videos its frames land in most: each frame votes for the videos of its
        ``per_frame`` nearest frames of other videos.  ``{video_name: [{'video_name', 'votes', 'share', 'score'}]}`` with
        ``votes`` the number of (frame, neighbour) pairs that landed in that video, ``share`` = votes over the video's filled
        neighbour slots, ``score`` the mean cosine similarity of those pairs; ordered by votes descending, then mean distance
        ascending, then name.  One neighbour table over the whole library (exact)."""
        if k <= 0 or per_frame <= 0:
            raise ValueError(f"k and per_frame must be at least 1, got {k}, {per_frame}")
        if not self.embeddings:
            return {}
        rows, dist = self._other_video_neighbors(int(per_frame))
        names = [md["video_name"] for md in self.metadata]
        tally: Dict[str, Dict[str, List]] = {}
        filled: Dict[str, int] = {}
        for r, (rr, dd) in enumerate(zip(rows.tolist(), dist.tolist())):
            mine = tally.setdefault(names[r], {})
            for c, d in zip(rr, dd):
                if c < 0:
                    continue
                filled[names[r]] = filled.get(names[r], 0) + 1
                cell = mine.setdefault(names[c], [0, 0.0])
                cell[0] += 1
                cell[1] += d
        out = {}
        for name, mine in tally.items():
            order = sorted(mine.items(), key=lambda kv: (-kv[1][0], kv[1][1] / kv[1][0], kv[0]))[:k]
            out[name] = [{"video_name": other, "votes": v, "share": v / filled[name], "score": 1.0 - s / v} for other, (v, s) in order]
        return out

    def duplicate_frames(self, min_similarity: float = 0.97) -> List[Dict]:
        """Every frame whose nearest frame of another video is at least ``min_similarity`` similar (cosine):
        ``[{'video_name', 'timestamp', 'other_video', 'other_timestamp', 'score'}]`` in frame order.  The same neighbour
        table as ``related_videos`` at one neighbour per frame (exact)."""
        if not min_similarity <= 1:                               # (NaN too)
            raise ValueError(f"min_similarity must be <= 1, got {min_similarity}")
        if not self.embeddings:
            return []
        rows, dist = self._other_video_neighbors(1)
        out = []
        for r in np.flatnonzero(rows[:, 0] >= 0).tolist():
            score = np.float32(1.0) - dist[r, 0]
            if score >= min_similarity:
                a, b = self.metadata[r], self.metadata[int(rows[r, 0])]
                out.append({"video_name": a["video_name"], "timestamp": a["timestamp"], "other_video": b["video_name"],
                            "other_timestamp": b["timestamp"], "score": float(score)})
        return out

    def video_summary(self, video_name: str, k: int = 5, max_radius: Optional[float] = None, chronological: bool = False) -> List[Dict]:
        """The k frames that show what is in ``video_name`` (a poster frame and a thumbnail strip): ``search``'s metadata dicts
        ``{'video_name', 'timestamp', 'frame_id'}`` plus ``'rank'`` (selection order: rank 0 is the frame most like the video as
        a whole), ``'radius'`` (every frame of the video lies within this cosine distance of one of the keyframes up to this
        one) and ``'members'`` (the frames this keyframe stands for).  ``HNSWIndex.summarize_group`` on the embeddings as
        stored: exact greedy farthest-point selection, ties between frames as ``search``; ``max_radius`` stops early.  In
        selection order, or by timestamp with ``chronological=True``.  ``KeyError`` for an unknown video."""
        if not self.embeddings:
            raise KeyError(video_name)
        res = self._device(ranks=True).summarize_group(video_name, k, max_radius=max_radius, group_of=self._group_fn)
        results = []
        for r in res:
            md = self.metadata[-r["id"]].copy()
            md.update(rank=r["rank"], radius=float(r["radius"]), members=r["members"])
            results.append(md)
        if chronological:
            results.sort(key=lambda md: md["timestamp"])
        return results

    def tag_videos(self, tag_embeddings, tags=None, top: int = 3, max_distance: Optional[float] = None) -> Dict[str, List[Dict]]:
        """Auto-tags for every video from a vocabulary of prompts (text prompts through ``extract_text_features``):
        ``{video_name: [{'tag', 'frames', 'share', 'timestamp', 'frame_id', 'score'}]}``, the ``top`` most voted tags of each
        video, most voted first.  Every frame votes for the prompt it is closest to (``HNSWIndex.label_groups``: exact; each
        prompt normalised as ``search`` normalises its query); ``frames`` is the number of the video's frames that voted for
        the tag, ``share`` that number over all the video's frames, ``timestamp`` / ``frame_id`` / ``score`` those of the
        frame that shows the tag best (ties between frames as ``search``).  ``tags`` names the embeddings (default: their
        indices).  ``max_distance``: frames farther than this cosine distance from every prompt vote for nothing."""
        embs = list(tag_embeddings)
        if not embs:
            raise ValueError("tag_videos needs at least one tag embedding")
        names = list(range(len(embs))) if tags is None else list(tags)
        if len(names) != len(embs):
            raise ValueError(f"{len(names)} tag names for {len(embs)} embeddings")
        if not self.embeddings:
            return {}
        dev = self._device(ranks=True)
        unit = np.ascontiguousarray(np.stack([_unit_query(q) for q in embs]))
        with dev.lock:                                # the prompts as normalised above, not normalised again
            res = dev._label_groups(unit, top, self._group_fn, max_distance, given=True)
        out = {}
        for video, found in res.items():
            out[video] = []
            for r in found:
                md = self.metadata[-r["id"]]
                out[video].append({"tag": names[r["label"]], "frames": r["votes"], "share": r["share"], "timestamp": md["timestamp"],
                                   "frame_id": md["frame_id"], "score": float(np.float32(1.0) - r["distance"])})
        return out

    def topics(self, k: int, top_videos: int = 3, **kw) -> List[Dict]:
        """The ``k`` themes of the whole library, nobody's prompts needed (a browse page: a poster frame per theme):
        ``[{'topic', 'video_name', 'timestamp', 'frame_id', 'score', 'size', 'share', 'videos'}]``, one entry per non-empty
        cluster of ``HNSWIndex.cluster(k, **kw)`` (exact spherical k-means over all frames; ``seed``, ``max_iter``, ``init``
        pass through), the largest first (equal sizes: the smaller cluster number).  ``video_name`` / ``timestamp`` /
        ``frame_id`` / ``score`` are those of the frame closest to the theme's centre, ``size`` its frames, ``share`` that
        over all frames, ``videos`` the ``top_videos`` videos with the most frames in it as ``{'video_name', 'frames'}``
        (more frames first, then library order).  The per-video counts are ``tag_videos``' vote on the final centres, which
        labels every frame as the clustering did; a video enters a theme's list when the theme is among its 16 most voted."""
        if int(top_videos) < 0:
            raise ValueError(f"top_videos must be >= 0, got {top_videos}")
        if not self.embeddings:
            return []
        dev = self._device(ranks=True)
        with dev.lock:                                # one lock for both calls: the same rows; the centres as returned, not normalised again
            res = dev.cluster(k, **kw)
            tagged = dev._label_groups(res["centroids"], dev.LABEL_MAX_TAGS, self._group_fn, None, given=True)
        votes: Dict[int, List] = {}
        for video, found in tagged.items():
            for r in found:
                votes.setdefault(r["label"], []).append((video, r["votes"]))
        n = len(self.embeddings)
        out = []
        for c in sorted((c for c in res["clusters"] if c["size"] > 0), key=lambda c: (-c["size"], c["cluster"])):
            md = self.metadata[-c["id"]]
            best = sorted(votes.get(c["cluster"], []), key=lambda vv: -vv[1])[:int(top_videos)]          # stable: library order on equal counts
            out.append({"topic": c["cluster"], "video_name": md["video_name"], "timestamp": md["timestamp"], "frame_id": md["frame_id"],
                        "score": float(c["score"]), "size": c["size"], "share": c["size"] / n,
                        "videos": [{"video_name": v, "frames": f} for v, f in best]})
        return out

    def video_chapters(self, video_name: str, k: int = 8, penalty: float = 0.0, max_frames: Optional[int] = None) -> List[Dict]:
        """Where ``video_name`` changes subject: at most k chapters in time order, ``[{'start', 'end', 'frames', 'spread',
        'poster'}]``.  ``start`` / ``end`` are the timestamps of a chapter's first and last frame, ``frames`` its number of
        frames, ``spread`` the mean cosine distance of its frames to its mean direction, ``poster`` ``search``'s metadata dict
        ``{'video_name', 'timestamp', 'frame_id'}`` of the frame most like the chapter as a whole.  ``HNSWIndex.segment_group``
        on the embeddings as stored: the optimal contiguous split, exact; ``penalty`` per chapter gives fewer chapters,
        ``max_frames`` caps a chapter's length.  Positions are ``round(timestamp * 1000)`` ms, groups the video names, ties
        between frames as ``search``.  ``KeyError`` for an unknown video."""
        if not self.embeddings:
            raise KeyError(video_name)
        res = self._device(ranks=True).segment_group(video_name, k, penalty=penalty, max_len=max_frames, group_of=self._group_fn,
                                                      position_of=self._pos_fn)
        return [{"start": self.metadata[-r["first"]]["timestamp"], "end": self.metadata[-r["last"]]["timestamp"], "frames": r["frames"],
                 "spread": float(r["spread"]), "poster": self.metadata[-r["show"]].copy()} for r in res]

    def save_to_disk(self, cache_path: Path):
        try:
            with open(cache_path, "wb") as f:
                pickle.dump({"embeddings": self.embeddings, "metadata": self.metadata,
                             "video_hashes": self.video_hashes, "version": "1.0"}, f)
            logger.info(f"Saved {len(self.embeddings)} embeddings to {cache_path}")
            return True
        except Exception as e:
            logger.error(f"Failed to save cache: {e}")
            return False

    def load_from_disk(self, cache_path: Path) -> bool:
        try:
            cache_path = Path(cache_path)
            if not cache_path.exists():
                return False
            with open(cache_path, "rb") as f:
                data = pickle.load(f)
            self.embeddings = data.get("embeddings", [])
            self.metadata = data.get("metadata", [])
            self.video_hashes = data.get("video_hashes", {})
            if self._dev is not None:
                self._dev.close()
            self._dev, self._pushed = None, 0
            logger.info(f"Loaded {len(self.embeddings)} embeddings from {cache_path}")
            return True
        except Exception as e:
            logger.error(f"Failed to load cache: {e}")
            return False
