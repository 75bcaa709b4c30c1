"""CPU (`-m "not gpu"`): the frame samplers of video_quierer_amd.core.frame_extractor — the adaptive keep/drop rule
(reference src/core/frame_extractor.py:117-160), its chunked form, the records, the uniform and hybrid samplers and
the readers.  No GPU: the adaptive sampler gets a fake scorer."""
import os
import re
import sys

import numpy as np
import pytest

from video_quierer_amd.core.frame_extractor import (AdaptiveFrameSampler, HybridFrameSampler, UniformFrameSampler,
                                                    select_scene_changes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rule_loop(scores, fps, threshold, min_interval, max_frames):
    """The reference's loop, frame by frame: read a frame while fewer than max_frames are kept; keep the first one;
    keep a later one when it is far enough from the last kept frame and its score is above the threshold."""
    gap = int(min_interval * fps)
    kept, last, number = [], -gap, 0
    while len(kept) < max_frames and number < len(scores):
        if number == 0:
            kept.append(0)
            last = 0
        elif number - last >= gap:
            if scores[number] > threshold:
                kept.append(number)
                last = number
        number += 1
    return kept


def test_select_hand_cases():
    s = [0.0] * 40
    s[14] = 99.0                                    # inside the 15-frame interval after frame 0: not examined
    assert select_scene_changes(s, 30, 30.0, 0.5)[0] == [0]
    s[15] = 99.0                                    # exactly 15 frames after frame 0: examined and taken
    assert select_scene_changes(s, 30, 30.0, 0.5)[0] == [0, 15]
    s[16:30] = [99.0] * 14                          # 16..29 are closer than 15 to frame 15
    assert select_scene_changes(s, 30, 30.0, 0.5)[0] == [0, 15]
    s[30] = 99.0
    assert select_scene_changes(s, 30, 30.0, 0.5)[0] == [0, 15, 30]
    # a score equal to the threshold is not taken
    assert select_scene_changes([0.0, 30.0, 30.000001], 0, 30.0, 0.5)[0] == [0, 2]
    # fps = 0: interval 0, every frame is examined
    assert select_scene_changes([5.0, 31.0, 31.0, 2.0, 31.0], 0, 30.0, 0.5)[0] == [0, 1, 2, 4]
    # max_frames = 3 stops after three (frame 0 counts)
    assert select_scene_changes([50.0] * 10, 0, 30.0, 0.5, max_frames=3)[0] == [0, 1, 2]
    assert select_scene_changes([50.0] * 10, 0, 30.0, 0.5, max_frames=0)[0] == []
    # the first frame is taken whatever its score
    assert select_scene_changes([-1.0], 30, 30.0, 0.5)[0] == [0]
    picked, state = select_scene_changes([], 30)
    assert picked == [] and state["seen"] == 0 and state["taken"] == 0


def random_cases():
    rng = np.random.default_rng(20261018)
    for _ in range(200):
        n = int(rng.integers(0, 200))
        fps = [0, 1, 23.976, 30, 60][int(rng.integers(0, 5))]
        min_interval = float(rng.choice([0.0, 0.1, 0.5, 1.0, 2.5]))
        threshold = float(rng.choice([0.0, 10.0, 25.0, 30.0, 60.0]))
        max_frames = int(rng.choice([0, 1, 2, 3, 10, 3600]))
        # scores around the threshold, some exactly on it
        scores = rng.uniform(0.0, 2.0 * threshold + 1.0, n)
        scores[rng.random(n) < 0.1] = threshold
        yield rng, scores, fps, threshold, min_interval, max_frames


def test_select_matches_the_literal_loop_and_chunks_match_one_shot():
    seen_nonempty = 0
    for rng, scores, fps, threshold, min_interval, max_frames in random_cases():
        want = rule_loop(list(scores), fps, threshold, min_interval, max_frames)
        got, state = select_scene_changes(scores, fps, threshold, min_interval, max_frames)
        assert got == want
        assert state["seen"] == len(scores) and state["taken"] == len(want)
        seen_nonempty += len(want) > 1
        # cut at random points (chunks of length 1 included) and carry the state
        cuts = sorted(set(rng.integers(0, len(scores) + 1, int(rng.integers(0, 8))).tolist() + [0, len(scores)]))
        if len(scores) > 3:
            cuts = sorted(set(cuts + [1, 2]))                  # two chunks of length 1 at the start
        chunked, st = [], None
        for a, b in zip(cuts[:-1], cuts[1:]):
            part, st = select_scene_changes(scores[a:b], fps, threshold, min_interval, max_frames, state=st)
            chunked += part
        assert chunked == want
    assert seen_nonempty > 50


def frames_of(n, h=4, w=5):
    """Frame i is filled with the value i, so a frame identifies itself."""
    return np.stack([np.full((h, w, 3), i, np.uint8) for i in range(n)])


class FakeScorer:
    """Scores from a table indexed by frame number (the frame's fill value); records what it was given."""

    def __init__(self, table):
        self.table, self.calls = table, []

    def __call__(self, frames, prev):
        self.calls.append((int(frames[0, 0, 0, 0]), len(frames), None if prev is None else int(np.asarray(prev)[0, 0, 0])))
        s = np.array([self.table[int(f[0, 0, 0])] for f in frames], dtype=np.float64)
        if prev is None:
            s[0] = 0.0
        return s


def test_adaptive_sample_chunks_records_and_prev():
    table = np.zeros(40)
    table[[3, 9, 10, 17, 31]] = [45.0, 80.0, 90.0, 31.0, 30.0]
    frames = frames_of(40)
    scorer = FakeScorer(table)
    sampler = AdaptiveFrameSampler(threshold=30.0, min_interval=0.5, max_frames=3600, scorer=scorer)
    fps = 12.0                                                # interval int(0.5 * 12) = 6
    recs = sampler.sample_chunks([frames[0:7], frames[7:8], frames[8:25], frames[25:40]], fps, video_path="v.mp4")
    # every chunk after the first gets the frame before it as prev
    assert scorer.calls == [(0, 7, None), (7, 1, 6), (8, 17, 7), (25, 15, 24)]
    assert [r["frame_number"] for r in recs] == [0, 9, 17]    # 3 is too close to 0, 10 too close to 9, 31 is not > 30
    for r in recs:
        assert set(r) == {"frame", "timestamp", "frame_number", "video_path", "scene_change_score"}
        assert r["timestamp"] == r["frame_number"] / fps and r["video_path"] == "v.mp4"
        assert r["frame"].shape == (4, 5, 3) and int(r["frame"][0, 0, 0]) == r["frame_number"]
    assert [r["scene_change_score"] for r in recs] == [0.0, 80.0, 31.0]
    # one piece: the same records; a list of frames is accepted
    one = AdaptiveFrameSampler(scorer=FakeScorer(table)).sample(list(frames), fps, video_path="v.mp4")
    assert [(r["frame_number"], r["scene_change_score"]) for r in one] == [(0, 0.0), (9, 80.0), (17, 31.0)]
    # max_frames ends the stream early: later chunks are not scored
    short = FakeScorer(table)
    recs = AdaptiveFrameSampler(max_frames=2, scorer=short).sample_chunks([frames[0:12], frames[12:40]], fps)
    assert [r["frame_number"] for r in recs] == [0, 9] and len(short.calls) == 1
    assert AdaptiveFrameSampler(scorer=FakeScorer(table)).sample(frames[:0], fps) == []


def test_uniform_indices():
    frames = frames_of(50)
    recs = UniformFrameSampler(sample_rate=2.0, max_frames=3600).sample(frames, fps=25.0, video_path="u")     # int(12.5) = 12
    assert [r["frame_number"] for r in recs] == [0, 12, 24, 36, 48]
    for r in recs:
        assert set(r) == {"frame", "timestamp", "frame_number", "video_path"}
        assert r["timestamp"] == r["frame_number"] / 25.0 and int(r["frame"][0, 0, 0]) == r["frame_number"]
    assert [r["frame_number"] for r in UniformFrameSampler(1.0, max_frames=3).sample(frames, 10.0)] == [0, 10, 20]
    # sample_rate above fps: the interval is clamped to 1
    assert [r["frame_number"] for r in UniformFrameSampler(100.0).sample(frames[:4], 10.0)] == [0, 1, 2, 3]
    # chunks that do not line up with the interval
    chunked = UniformFrameSampler(2.0).sample_chunks([frames[0:5], frames[5:13], frames[13:14], frames[14:50]], 25.0)
    assert [r["frame_number"] for r in chunked] == [0, 12, 24, 36, 48]


def test_hybrid_merge_prefers_uniform_on_a_shared_timestamp():
    table = np.zeros(60)
    table[[20, 27, 45]] = [50.0, 26.0, 25.0]                   # 20: also a uniform frame; 27: adaptive only; 45: not > 25
    frames = frames_of(60)
    hy = HybridFrameSampler(base_sample_rate=0.5, scene_threshold=25.0, max_frames=3600, scorer=FakeScorer(table))
    assert hy.uniform_sampler.max_frames == 1800 and hy.adaptive_sampler.max_frames == 1800
    assert hy.adaptive_sampler.threshold == 25.0 and hy.adaptive_sampler.min_interval == 0.5
    recs = hy.sample(frames, fps=10.0, video_path="h")         # uniform interval int(10 / 0.5) = 20; adaptive interval 5
    assert [(r["frame_number"], r["sampling_method"]) for r in recs] == [(0, "uniform"), (20, "uniform"), (27, "adaptive"),
                                                                           (40, "uniform")]
    assert "scene_change_score" not in recs[1]                 # the uniform record won, not the adaptive one of frame 20
    assert recs[2]["scene_change_score"] == 26.0
    assert [r["timestamp"] for r in recs] == sorted(r["timestamp"] for r in recs)
    chunked = hy.sample_chunks([frames[:21], frames[21:28], frames[28:]], 10.0, "h")
    assert [(r["frame_number"], r["sampling_method"]) for r in chunked] == [(r["frame_number"], r["sampling_method"]) for r in recs]


def test_extract_frames_readers(monkeypatch):
    frames = frames_of(30)
    table = np.zeros(30)
    table[12] = 40.0
    opened = []

    def reader(path):
        opened.append(path)
        return 10.0, iter([frames[:8], frames[8:]])

    recs = AdaptiveFrameSampler(scorer=FakeScorer(table)).extract_frames("clip.mp4", reader=reader)
    assert [r["frame_number"] for r in recs] == [0, 12] and recs[1]["video_path"] == "clip.mp4"
    assert [r["frame_number"] for r in UniformFrameSampler(1.0).extract_frames("clip.mp4", reader=reader)] == [0, 10, 20]
    hy = HybridFrameSampler(scorer=FakeScorer(table)).extract_frames("clip.mp4", reader=reader)
    assert [(r["frame_number"], r["sampling_method"]) for r in hy] == [(0, "uniform"), (12, "adaptive"), (20, "uniform")]
    assert opened == ["clip.mp4"] * 3
    # no reader and no OpenCV: an ImportError that names the way out
    monkeypatch.setitem(sys.modules, "cv2", None)
    for sampler in (UniformFrameSampler(), AdaptiveFrameSampler(scorer=FakeScorer(table)), HybridFrameSampler()):
        with pytest.raises(ImportError, match="reader="):
            sampler.extract_frames("clip.mp4")


def test_module_imports_without_gpu_or_opencv():
    import subprocess
    code = ("import sys; sys.modules['cv2'] = None; sys.modules['torch'] = None\n"
            "import video_quierer_amd.core.frame_extractor as m; print(sorted(n for n in dir(m) if n.endswith('Sampler')))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "AdaptiveFrameSampler" in out.stdout and "HybridFrameSampler" in out.stdout


def test_python_constants_match_the_kernel_header():
    from video_quierer_amd import preprocess
    text = open(os.path.join(ROOT, "video-quierer_amd", "csrc", "preproc_kernels.h")).read()
    ppt = int(re.search(r"constexpr int SC_PPT = (\d+);", text).group(1))
    threads = int(re.search(r"constexpr int RS_THREADS = (\d+);", text).group(1))
    assert re.search(r"constexpr int SC_TILE = RS_THREADS \* SC_PPT;", text)
    assert preprocess.SCENE_TILE_PIXELS == ppt * threads
    assert preprocess.SCENE_CHUNK_FRAMES == int(re.search(r"constexpr int SC_CHUNK_FRAMES = (\d+);", text).group(1))
    assert preprocess.SCENE_CHUNK_FRAMES >= 8
