"""The reference's ``core.frame_extractor`` (reference src/core/frame_extractor.py) over decoded frames: the samplers
(:23-237) choose which frames of a video go on, :class:`OptimizedFrameExtractor` (:240-362) resizes them, drops the
low-quality ones and hands the rest to the encoder.

  * :class:`UniformFrameSampler` — every ``interval``-th frame (index arithmetic only);
  * :class:`AdaptiveFrameSampler` — a frame is kept when its scene-change score against the frame before it exceeds
    a threshold.  The score (grey MSE + 0.01 * chi-square of the grey histograms, reference :168-186) is computed on
    the GPU for every consecutive pair of a batch (``FramePreprocessor.scene_change_scores``); the keep/drop rule
    (:func:`select_scene_changes`) is host code;
  * :class:`HybridFrameSampler` — both, merged by timestamp.

  * :class:`OptimizedFrameExtractor` — a sampler plus the post-processing of its records: resize to ``frame_size``,
    quality verdict and compaction, one GPU pass per chunk of a video (``FramePreprocessor.postprocess_list``);
  * :func:`choose_optimal_strategy` — the reference's duration heuristic.

The samplers take frames (``sample``), an iterable of frame chunks of one video (``sample_chunks``, or chunk by chunk
``iter_chunks``) or, for the reference's call shape, a path plus a ``reader`` that decodes it (``extract_frames``).
Records are the reference's dicts.  Importing this module needs neither OpenCV, torch nor a GPU; the default scorer and
the default preprocessor bind the GPU when first used.  ``install_dropin()`` registers it as ``core.frame_extractor``.
"""
import logging
import time
from typing import Any, Callable, Dict, Iterable, Iterator, List, Optional, Tuple

import numpy as np

logger = logging.getLogger(__name__)

Record = Dict[str, Any]
Reader = Callable[[str], Tuple[float, Iterable[np.ndarray]]]


def _batch(frames) -> np.ndarray:
    """An array [n, h, w, 3], or a list of equal-size frames, as one uint8 array."""
    if isinstance(frames, (list, tuple)):
        if not frames:
            return np.empty((0, 0, 0, 3), np.uint8)
        a = np.stack([np.asarray(f) for f in frames])
    else:
        a = np.asarray(frames)
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4 or a.shape[3] != 3 or a.dtype != np.uint8:
        raise ValueError(f"expected uint8 frames [n, h, w, 3], got {a.dtype} {a.shape}")
    return a


def cv2_reader(video_path: str, chunk: int = 64):
    """Default ``reader``: (fps, generator of uint8 [<= chunk, h, w, 3] BGR arrays) from ``cv2.VideoCapture``.
    Untested in this repository: OpenCV is not installed where its tests run, so only the ImportError is covered."""
    try:
        import cv2
    except ImportError as e:
        raise ImportError("decoding a video file needs OpenCV (cv2), which is not installed: pass reader=") from e
    video = cv2.VideoCapture(video_path)
    if not video.isOpened():
        raise ValueError(f"Cannot open video: {video_path}")

    def chunks():
        try:
            ok = True
            while ok:
                got = []
                while ok and len(got) < chunk:
                    ok, frame = video.read()
                    if ok:
                        got.append(frame)
                if got:
                    yield np.stack(got)
        finally:
            video.release()
    return video.get(cv2.CAP_PROP_FPS), chunks()


def select_scene_changes(scores, fps: float, threshold: float = 30.0, min_interval: float = 0.5, max_frames: int = 3600,
                         state: Optional[dict] = None) -> Tuple[List[int], dict]:
    """The keep/drop rule of the reference's adaptive sampler (:117-160) over per-frame scene-change scores.

    ``scores[j]`` belongs to frame ``state['seen'] + j`` of the video and compares it with the frame before it.  The
    video's first frame is always taken.  A later frame is examined only when at least ``int(min_interval * fps)``
    frames lie between it and the last taken one, and taken when its score is strictly greater than ``threshold``.
    Nothing is taken once ``max_frames`` are.  Returns the taken frame numbers (counted from the start of the video)
    and the state to pass with the video's next chunk: ``{'seen', 'last_taken', 'taken'}``; a video fed in chunks
    gives the frame numbers it gives in one piece."""
    gap = int(min_interval * fps)
    st = dict(state) if state is not None else {"seen": 0, "last_taken": -gap, "taken": 0}
    picked: List[int] = []
    for s in scores:
        number = st["seen"]
        st["seen"] = number + 1
        if st["taken"] >= max_frames:
            continue
        if number == 0 or (number - st["last_taken"] >= gap and s > threshold):
            picked.append(number)
            st["last_taken"] = number
            st["taken"] += 1
    return picked, st


class _ChunkedSampler:
    """sample / sample_chunks / extract_frames in terms of ``_start(fps)`` and ``_feed(run, chunk, fps, video_path)``."""

    def sample(self, frames, fps: float, video_path: Optional[str] = None) -> List[Record]:
        """Records of the frames taken from ``frames`` (an array [n, h, w, 3] or a list of equal-size frames)."""
        return self.sample_chunks([frames], fps, video_path, _copy=False)

    def sample_chunks(self, chunks: Iterable, fps: float, video_path: Optional[str] = None, _copy: bool = True) -> List[Record]:
        """:meth:`sample` of one video that arrives as consecutive chunks of frames; the same records as in one piece
        (their ``'frame'`` is a copy, so a record does not keep its whole chunk alive)."""
        out: List[Record] = []
        for recs in self.iter_chunks(chunks, fps, video_path, _copy):
            out.extend(recs)
        return out

    def iter_chunks(self, chunks: Iterable, fps: float, video_path: Optional[str] = None, _copy: bool = True) -> Iterator[List[Record]]:
        """:meth:`sample_chunks` chunk by chunk: yields the records of each chunk as soon as it has been fed, so a
        caller can post-process them and let the chunk's full-size frames go.  Concatenated, the lists are
        ``sample_chunks``'s records.  With ``_copy=False`` a record's ``'frame'`` is a view into its chunk."""
        run = self._start(fps)
        for chunk in chunks:
            a = _batch(chunk)
            if len(a):
                yield self._feed(run, a, fps, video_path, _copy)
            if run["taken"] >= self.max_frames:
                break                                    # the reference stops decoding here

    def extract_frames(self, video_path: str, reader: Optional[Reader] = None) -> List[Record]:
        """The reference's call shape.  ``reader(video_path) -> (fps, iterable of frame chunks)``; the default decodes
        with OpenCV (:func:`cv2_reader`) and raises ImportError where OpenCV is missing."""
        fps, chunks = (reader or cv2_reader)(video_path)
        return self.sample_chunks(chunks, fps, video_path)


def _record(a: np.ndarray, local: int, number: int, fps: float, video_path, copy: bool) -> Record:
    return {"frame": a[local].copy() if copy else a[local], "timestamp": number / fps, "frame_number": number,
            "video_path": video_path}


class UniformFrameSampler(_ChunkedSampler):
    """Frames 0, interval, 2 * interval, ... with ``interval = max(1, int(fps / sample_rate))``, at most ``max_frames``
    (reference :23-88)."""

    def __init__(self, sample_rate: float = 1.0, max_frames: int = 3600):
        self.sample_rate = sample_rate
        self.max_frames = max_frames

    def _start(self, fps):
        return {"seen": 0, "taken": 0, "interval": max(1, int(fps / self.sample_rate))}

    def _feed(self, run, a, fps, video_path, copy):
        out, base = [], run["seen"]
        first = -base % run["interval"]                  # first frame of this chunk that is a multiple of the interval
        for local in range(first, len(a), run["interval"]):
            if run["taken"] >= self.max_frames:
                break
            out.append(_record(a, local, base + local, fps, video_path, copy))
            run["taken"] += 1
        run["seen"] = base + len(a)
        return out


class AdaptiveFrameSampler(_ChunkedSampler):
    """Frames whose scene-change score exceeds ``threshold``, at least ``min_interval`` seconds apart, the first frame
    always (reference :90-186).  ``scorer(frames, prev) -> scores[n]`` scores frame i against frame i - 1 and frame 0
    against ``prev`` (None: score 0.0); the default is ``FramePreprocessor.scene_change_scores`` on the GPU, created
    when first needed."""

    def __init__(self, threshold: float = 30.0, min_interval: float = 0.5, max_frames: int = 3600,
                 scorer: Optional[Callable] = None):
        self.threshold = threshold
        self.min_interval = min_interval
        self.max_frames = max_frames
        self._scorer = scorer

    def _score(self, frames, prev):
        if self._scorer is None:
            from ..preprocess import FramePreprocessor
            pre = FramePreprocessor()
            self._scorer = lambda f, p: pre.scene_change_scores(f, p)[0]
        return self._scorer(frames, prev)

    def _start(self, fps):
        return {"taken": 0, "prev": None, "state": None}

    def _feed(self, run, a, fps, video_path, copy):
        scores = np.asarray(self._score(a, run["prev"]), dtype=np.float64)
        base = run["state"]["seen"] if run["state"] else 0
        picked, run["state"] = select_scene_changes(scores, fps, self.threshold, self.min_interval, self.max_frames, run["state"])
        run["taken"] = run["state"]["taken"]
        run["prev"] = a[-1].copy() if copy else a[-1]
        out = []
        for number in picked:
            rec = _record(a, number - base, number, fps, video_path, copy)
            rec["scene_change_score"] = 0.0 if number == 0 else float(scores[number - base])
            out.append(rec)
        return out


class HybridFrameSampler(_ChunkedSampler):
    """Uniform and adaptive sampling of the same frames, merged by timestamp (reference :189-237): uniform with
    ``max_frames // 2`` and adaptive ``(scene_threshold, 0.5, max_frames // 2)``; every record is tagged with its
    ``sampling_method``."""

    def __init__(self, base_sample_rate: float = 0.5, scene_threshold: float = 25.0, max_frames: int = 3600,
                 scorer: Optional[Callable] = None):
        self.uniform_sampler = UniformFrameSampler(base_sample_rate, max_frames // 2)
        self.adaptive_sampler = AdaptiveFrameSampler(scene_threshold, 0.5, max_frames // 2, scorer=scorer)

    def sample_chunks(self, chunks: Iterable, fps: float, video_path: Optional[str] = None, _copy: bool = True) -> List[Record]:
        samplers = (self.uniform_sampler, self.adaptive_sampler)
        runs = [s._start(fps) for s in samplers]
        found: List[List[Record]] = [[], []]
        for chunk in chunks:                             # one pass over the frames feeds both samplers
            a = _batch(chunk)
            live = [i for i, s in enumerate(samplers) if runs[i]["taken"] < s.max_frames]
            if not live:
                break
            for i in live:
                if len(a):
                    found[i].extend(samplers[i]._feed(runs[i], a, fps, video_path, _copy))
        merged: Dict[float, Record] = {}
        for rec in found[0]:
            rec["sampling_method"] = "uniform"
            merged[rec["timestamp"]] = rec
        for rec in found[1]:
            # The reference also lets an adaptive record replace a uniform one of the same timestamp when the nearest
            # existing timestamp is more than 0.5 s away; for a timestamp that is already a key the nearest one is
            # itself, at distance 0, so that clause never fires: an adaptive record only ever fills a new timestamp.
            if rec["timestamp"] not in merged:
                rec["sampling_method"] = "adaptive"
                merged[rec["timestamp"]] = rec
        return sorted(merged.values(), key=lambda rec: rec["timestamp"])

    def iter_chunks(self, chunks: Iterable, fps: float, video_path: Optional[str] = None, _copy: bool = True) -> Iterator[List[Record]]:
        """The merge of :meth:`sample_chunks` chunk by chunk.  Two records share a timestamp only when they are the
        same frame, hence in the same chunk, and timestamps grow from chunk to chunk: merging inside each chunk and
        concatenating gives the records ``sample_chunks`` gives."""
        samplers = (self.uniform_sampler, self.adaptive_sampler)
        runs = [s._start(fps) for s in samplers]
        for chunk in chunks:
            a = _batch(chunk)
            live = [i for i, s in enumerate(samplers) if runs[i]["taken"] < s.max_frames]
            if not live:
                break
            if not len(a):
                continue
            merged: Dict[float, Record] = {}
            for i in live:
                for rec in samplers[i]._feed(runs[i], a, fps, video_path, _copy):
                    if rec["timestamp"] not in merged:      # live is in (uniform, adaptive) order: uniform wins
                        rec["sampling_method"] = ("uniform", "adaptive")[i]
                        merged[rec["timestamp"]] = rec
            yield sorted(merged.values(), key=lambda rec: rec["timestamp"])


class OptimizedFrameExtractor:
    """The reference's main frame extraction class (:240-362): a sampler chosen by ``strategy`` plus the
    post-processing of its records — resize to ``frame_size``, quality filter — done per chunk of the video in one GPU
    pass (``preprocessor.postprocess_list``; the default :class:`~video_quierer_amd.preprocess.FramePreprocessor` is
    created when first needed).  ``frame_size`` keeps the reference's quirk: a frame is resized unless
    ``frame.shape[:2] == frame_size``, and then to width ``frame_size[0]``, height ``frame_size[1]``."""

    def __init__(self, sample_rate: float = 1.0, strategy: str = "uniform", max_frames_per_video: int = 3600,
                 frame_size: Optional[tuple] = (224, 224), quality_filter: bool = True, preprocessor=None):
        self.sample_rate = sample_rate
        self.max_frames_per_video = max_frames_per_video
        self.frame_size = frame_size
        self.quality_filter = quality_filter
        self._preprocessor = preprocessor
        if strategy == "uniform":
            self.sampler = UniformFrameSampler(sample_rate, max_frames_per_video)
        elif strategy == "adaptive":
            self.sampler = AdaptiveFrameSampler(max_frames=max_frames_per_video)
        elif strategy == "hybrid":
            self.sampler = HybridFrameSampler(sample_rate * 0.7, max_frames=max_frames_per_video)
        else:
            raise ValueError(f"Unknown strategy: {strategy}")

    @property
    def preprocessor(self):
        if self._preprocessor is None:
            from ..preprocess import FramePreprocessor
            self._preprocessor = FramePreprocessor()
        return self._preprocessor

    def _post(self, records: List[Record], start: Optional[float], always_resize: bool = False) -> List[Record]:
        """Post-process records in runs of equal frame shape, order preserved; survivors get the resized frame and,
        with ``start``, the seconds since ``start`` at which their batch finished as ``'processing_time'``."""
        out: List[Record] = []
        a = 0
        while a < len(records):
            shape = np.asarray(records[a]["frame"]).shape
            b = a + 1
            while b < len(records) and np.asarray(records[b]["frame"]).shape == shape:
                b += 1
            kept, keep, _ = self.preprocessor.postprocess_list([rec["frame"] for rec in records[a:b]], self.frame_size or None,
                                                               bool(self.quality_filter), always_resize=always_resize)
            done = None if start is None else time.perf_counter() - start
            j = 0
            for rec, ok in zip(records[a:b], keep):
                if ok:
                    rec["frame"] = np.array(kept[j])        # its own memory: a record does not keep its batch alive
                    if done is not None:
                        rec["processing_time"] = done
                    out.append(rec)
                    j += 1
            a = b
        return out

    def process_records(self, records: List[Record]) -> List[Record]:
        """The post-processing of :meth:`extract_frames` for records a caller already has (any sampler's): low-quality
        ones are dropped, ``'frame'`` becomes the resized frame.  Runs of equal frame shape go through together."""
        return self._post(list(records), None)

    def extract_frames(self, video_path: str, reader: Optional[Reader] = None) -> List[Record]:
        """Extract and preprocess frames from a video (reference :268-299).  Each chunk's records are post-processed as
        they appear, so at most one chunk of full-size frames is held (the reference holds every sampled frame of the
        video at full size: 3,600 frames of 1080p are 22 GB).  ``'processing_time'`` is the time since the call began
        at which the record's chunk was finished; it does not decrease along the list."""
        start = time.perf_counter()
        fps, chunks = (reader or cv2_reader)(video_path)
        out: List[Record] = []
        for recs in self.sampler.iter_chunks(chunks, fps, video_path, _copy=False):
            out.extend(self._post(recs, start))
        total = time.perf_counter() - start
        logger.info("Frame extraction completed: %d frames in %.2fs (%.1f fps)", len(out), total, len(out) / total if total > 0 else 0.0)
        return out

    def extract_frames_generator(self, video_path: str, reader: Optional[Reader] = None) -> Iterator[Record]:
        """Memory-efficient extraction (reference :318-362): frames 0, interval, 2 * interval, ... with
        ``interval = max(1, int(fps / sample_rate))``, always resized when ``frame_size`` is set; a low-quality frame
        is skipped without counting towards ``max_frames_per_video``.  Records carry no ``'processing_time'``."""
        fps, chunks = (reader or cv2_reader)(video_path)
        interval = max(1, int(fps / self.sample_rate))
        seen = count = 0
        for chunk in chunks:
            if count >= self.max_frames_per_video:
                break
            a = _batch(chunk)
            recs = [_record(a, local, seen + local, fps, video_path, False) for local in range(-seen % interval, len(a), interval)]
            seen += len(a)
            for rec in self._post(recs, None, always_resize=True):
                if count >= self.max_frames_per_video:
                    break
                count += 1
                yield rec


def cv2_probe(video_path: str) -> Optional[Tuple[float, int]]:
    """Default ``probe`` of :func:`choose_optimal_strategy`: (fps, frame_count) from ``cv2.VideoCapture``, or None
    when the file does not open."""
    try:
        import cv2
    except ImportError as e:
        raise ImportError("probing a video file needs OpenCV (cv2), which is not installed: pass probe=") from e
    video = cv2.VideoCapture(video_path)
    if not video.isOpened():
        return None
    try:
        return video.get(cv2.CAP_PROP_FPS), int(video.get(cv2.CAP_PROP_FRAME_COUNT))
    finally:
        video.release()


def choose_optimal_strategy(video_path: str, probe: Optional[Callable] = None) -> str:
    """The reference's heuristic (:365-388): 'uniform' under 5 minutes (and for a file that does not open), 'adaptive'
    over an hour, 'hybrid' between.  ``probe(video_path) -> (fps, frame_count)`` or None; the default uses OpenCV."""
    got = (probe or cv2_probe)(video_path)
    if got is None:
        return "uniform"
    fps, frame_count = got
    duration = int(frame_count) / fps if fps > 0 else 0
    if duration < 300:
        return "uniform"
    if duration > 3600:
        return "adaptive"
    return "hybrid"
