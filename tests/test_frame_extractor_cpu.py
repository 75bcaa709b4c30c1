"""CPU (`-m "not gpu"`): OptimizedFrameExtractor, extract_frames_generator, choose_optimal_strategy and the host plan of
the post-processing pass (video_quierer_amd.core.frame_extractor, vq_frame_postprocess_plan).  No GPU: the extractor
gets a fake preprocessor made of the two CPU oracles, the adaptive sampler a scorer that reads scores from a table."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from oracle.cv_resize_oracle import resize_linear_u8
from oracle.quality_oracle import is_low_quality
from video_quierer_amd.core.frame_extractor import (AdaptiveFrameSampler, HybridFrameSampler, OptimizedFrameExtractor,
                                                    UniformFrameSampler, choose_optimal_strategy)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 12, 10
SIZE = (8, 6)                 # frame_size = (width, height): resized frames are 6 rows x 8 columns


class OraclePreprocessor:
    """postprocess_list restated with the CPU oracles; records the size of every call."""

    def __init__(self):
        self.calls = []

    def postprocess_list(self, frames, frame_size=(224, 224), quality_filter=True, keep_on_device=False, always_resize=False):
        frames = [np.asarray(f) for f in frames]
        self.calls.append((len(frames), frames[0].shape))
        out = []
        for f in frames:
            if frame_size and (always_resize or f.shape[:2] != tuple(frame_size)):
                f = resize_linear_u8(f, frame_size[0], frame_size[1])
            out.append(f)
        keep = np.array([not (quality_filter and is_low_quality(f)) for f in out], bool)
        kept = [f for f, k in zip(out, keep) if k]
        return (np.stack(kept) if kept else np.empty((0,) + out[0].shape, np.uint8)), keep, None


def clip(n, bad=()):
    """n <= 60 frames of H x W: noise (kept by the quality filter), the ones in `bad` nearly black (dropped: mean
    brightness under 20, resized or not).  Pixel (0, 0) of frame i holds i, so a frame identifies itself to the scorer."""
    rng = np.random.default_rng([20261019, n])
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    for i in bad:
        frames[i] = 3
    frames[:, 0, 0, :] = np.arange(n, dtype=np.uint8)[:, None]
    return frames


class TableScorer:
    def __init__(self, table):
        self.table = table

    def __call__(self, frames, prev):
        s = np.array([self.table[int(f[0, 0, 0])] for f in frames], dtype=np.float64)
        if prev is None:
            s[0] = 0.0
        return s


def reader_of(frames, fps, cuts):
    edges = [0] + list(cuts) + [len(frames)]
    return lambda path: (fps, iter([frames[a:b] for a, b in zip(edges[:-1], edges[1:])]))


def expected(records, frame_size=SIZE, quality_filter=True):
    """The reference's loop (:279-293) over sampler records, with the oracles."""
    out = []
    for rec in records:
        f = rec["frame"]
        if frame_size and f.shape[:2] != tuple(frame_size):
            f = resize_linear_u8(f, frame_size[0], frame_size[1])
        if quality_filter and is_low_quality(f):
            continue
        out.append(dict(rec, frame=f))
    return out


def same_records(got, want, extra=("processing_time",)):
    assert [r["frame_number"] for r in got] == [r["frame_number"] for r in want]
    for g, w in zip(got, want):
        assert set(g) == set(w) | set(extra)
        assert np.array_equal(g["frame"], w["frame"]) and g["frame"].dtype == np.uint8
        for key in set(w) - {"frame"}:
            assert g[key] == w[key], key


def test_constructor_builds_the_references_samplers():
    ex = OptimizedFrameExtractor()
    assert (ex.sample_rate, ex.max_frames_per_video, ex.frame_size, ex.quality_filter) == (1.0, 3600, (224, 224), True)
    assert type(ex.sampler) is UniformFrameSampler and (ex.sampler.sample_rate, ex.sampler.max_frames) == (1.0, 3600)
    ex = OptimizedFrameExtractor(2.5, "uniform", 17, None, False)
    assert (ex.sampler.sample_rate, ex.sampler.max_frames, ex.frame_size, ex.quality_filter) == (2.5, 17, None, False)
    ex = OptimizedFrameExtractor(sample_rate=2.0, strategy="adaptive", max_frames_per_video=40)
    assert type(ex.sampler) is AdaptiveFrameSampler
    assert (ex.sampler.threshold, ex.sampler.min_interval, ex.sampler.max_frames) == (30.0, 0.5, 40)
    ex = OptimizedFrameExtractor(sample_rate=2.0, strategy="hybrid", max_frames_per_video=40)
    assert type(ex.sampler) is HybridFrameSampler
    assert ex.sampler.uniform_sampler.sample_rate == 2.0 * 0.7 and ex.sampler.uniform_sampler.max_frames == 20
    assert (ex.sampler.adaptive_sampler.threshold, ex.sampler.adaptive_sampler.max_frames) == (25.0, 20)
    with pytest.raises(ValueError, match="Unknown strategy: fast"):
        OptimizedFrameExtractor(strategy="fast")


@pytest.mark.parametrize("cuts", [(), (7,), (1, 2, 20, 21, 39), tuple(range(1, 60))])
def test_extract_frames_uniform(cuts):
    frames = clip(60, bad=(0, 12, 40))
    pre = OraclePreprocessor()
    ex = OptimizedFrameExtractor(sample_rate=2.5, frame_size=SIZE, preprocessor=pre)            # interval int(10 / 2.5) = 4
    recs = ex.extract_frames("u.mp4", reader=reader_of(frames, 10.0, cuts))
    want = expected(UniformFrameSampler(2.5).sample(frames, 10.0, "u.mp4"))
    assert [r["frame_number"] for r in want] == [n for n in range(0, 60, 4) if n not in (0, 12, 40)]
    same_records(recs, want)
    assert all(r["frame"].shape == (6, 8, 3) for r in recs)
    times = [r["processing_time"] for r in recs]
    assert times == sorted(times) and times[0] >= 0.0
    # a call never holds more than one chunk's full-size frames
    edges = [0] + list(cuts) + [60]
    assert max(n for n, _ in pre.calls) <= max(b - a for a, b in zip(edges[:-1], edges[1:]))
    assert all(shape == (H, W, 3) for _, shape in pre.calls)
    if len(cuts) > 1:
        assert len(pre.calls) > 1


def test_extract_frames_adaptive_and_switches():
    table = np.zeros(60)
    table[[9, 10, 17, 31, 50]] = [80.0, 90.0, 31.0, 30.0, 45.0]
    frames = clip(60, bad=(17,))
    for cuts in ((), (5, 6, 30)):
        ex = OptimizedFrameExtractor(strategy="adaptive", frame_size=SIZE, preprocessor=OraclePreprocessor())
        ex.sampler._scorer = TableScorer(table)
        recs = ex.extract_frames("a.mp4", reader=reader_of(frames, 12.0, cuts))
        want = expected(AdaptiveFrameSampler(scorer=TableScorer(table)).sample(frames, 12.0, "a.mp4"))
        assert [r["frame_number"] for r in want] == [0, 9, 50]                                  # 17 is taken, then dropped as flat
        same_records(recs, want)
        assert [r["scene_change_score"] for r in recs] == [0.0, 80.0, 45.0]
    # quality_filter=False keeps the flat frame; frame_size=None leaves the frames as they are
    ex = OptimizedFrameExtractor(strategy="adaptive", frame_size=None, quality_filter=False, preprocessor=OraclePreprocessor())
    ex.sampler._scorer = TableScorer(table)
    recs = ex.extract_frames("a.mp4", reader=reader_of(frames, 12.0, (8,)))
    assert [r["frame_number"] for r in recs] == [0, 9, 17, 50]
    assert all(np.array_equal(r["frame"], frames[r["frame_number"]]) for r in recs)
    # the reference's quirk: a frame whose shape[:2] equals frame_size is not resized, whatever cv2's (width, height) order says
    ex = OptimizedFrameExtractor(frame_size=(H, W), quality_filter=False, preprocessor=OraclePreprocessor())
    recs = ex.extract_frames("q.mp4", reader=reader_of(frames, 1.0, ()))
    assert recs[0]["frame"].shape == (H, W, 3)
    ex = OptimizedFrameExtractor(frame_size=(W, H), quality_filter=False, preprocessor=OraclePreprocessor())
    assert np.array_equal(ex.extract_frames("q.mp4", reader=reader_of(frames, 1.0, ()))[3]["frame"], frames[3])


def test_extract_frames_hybrid_streams_what_sample_gives():
    table = np.zeros(60)
    table[[20, 27, 45, 46]] = [50.0, 26.0, 25.0, 70.0]
    frames = clip(60, bad=(27, 40))
    want = expected(HybridFrameSampler(0.7 * 0.7, max_frames=3600, scorer=TableScorer(table)).sample(frames, 10.0, "h.mp4"))
    assert [(r["frame_number"], r["sampling_method"]) for r in want] == [(0, "uniform"), (20, "uniform"), (46, "adaptive")]
    for cuts in ((), (21, 28), tuple(range(1, 60, 3))):
        pre = OraclePreprocessor()
        ex = OptimizedFrameExtractor(sample_rate=0.7, strategy="hybrid", frame_size=SIZE, preprocessor=pre)
        ex.sampler.adaptive_sampler._scorer = TableScorer(table)
        same_records(ex.extract_frames("h.mp4", reader=reader_of(frames, 10.0, cuts)), want)
    # the per-chunk generator of a sampler, concatenated, is its sample_chunks
    hy = HybridFrameSampler(0.49, scorer=TableScorer(table))
    chunks = [frames[:21], frames[21:28], frames[:0], frames[28:]]
    flat = [r for recs in hy.iter_chunks(chunks, 10.0, "h.mp4") for r in recs]
    whole = hy.sample_chunks(chunks, 10.0, "h.mp4")
    assert [(r["frame_number"], r["sampling_method"], r["timestamp"]) for r in flat] == \
           [(r["frame_number"], r["sampling_method"], r["timestamp"]) for r in whole]


def test_process_records_groups_runs_of_one_shape():
    pre = OraclePreprocessor()
    ex = OptimizedFrameExtractor(frame_size=SIZE, preprocessor=pre)
    rng = np.random.default_rng(5)
    shapes = [(H, W), (H, W), (9, 7), (H, W), (6, 8), (6, 8)]
    recs = [{"frame": rng.integers(0, 256, s + (3,), dtype=np.uint8), "timestamp": float(i), "frame_number": i, "video_path": None}
            for i, s in enumerate(shapes)]
    recs[1]["frame"][:] = 3                                                                     # dark and flat: dropped
    want = expected([dict(r) for r in recs])
    got = ex.process_records([dict(r) for r in recs])
    same_records(got, want, extra=())
    assert [r["frame_number"] for r in got] == [0, 2, 3, 4, 5]
    assert pre.calls == [(2, (H, W, 3)), (1, (9, 7, 3)), (1, (H, W, 3)), (2, (6, 8, 3))]
    assert ex.process_records([]) == []


def test_extract_frames_generator():
    frames = clip(50, bad=(0, 12, 13))
    for cuts in ((), (5, 13, 14, 30)):
        ex = OptimizedFrameExtractor(sample_rate=2.0, max_frames_per_video=3, frame_size=SIZE, preprocessor=OraclePreprocessor())
        got = list(ex.extract_frames_generator("g.mp4", reader=reader_of(frames, 25.0, cuts)))  # interval int(12.5) = 12
        # frames 0 and 12 are low quality and do not count; three good ones end it
        assert [r["frame_number"] for r in got] == [24, 36, 48]
        for r in got:
            assert set(r) == {"frame", "timestamp", "frame_number", "video_path"}
            assert r["timestamp"] == r["frame_number"] / 25.0 and r["video_path"] == "g.mp4"
            assert np.array_equal(r["frame"], resize_linear_u8(frames[r["frame_number"]], *SIZE))
    ex = OptimizedFrameExtractor(sample_rate=2.0, max_frames_per_video=2, frame_size=SIZE, preprocessor=OraclePreprocessor())
    assert [r["frame_number"] for r in ex.extract_frames_generator("g", reader=reader_of(frames, 25.0, (30,)))] == [24, 36]
    # sample_rate above fps: interval 1; quality_filter=False counts every frame
    ex = OptimizedFrameExtractor(sample_rate=100.0, max_frames_per_video=4, frame_size=SIZE, quality_filter=False,
                                 preprocessor=OraclePreprocessor())
    assert [r["frame_number"] for r in ex.extract_frames_generator("g", reader=reader_of(frames, 25.0, (2,)))] == [0, 1, 2, 3]
    # the generator always resizes when frame_size is set: a 12 x 10 frame and frame_size (12, 10) give 10 rows x 12 columns
    ex = OptimizedFrameExtractor(max_frames_per_video=1, frame_size=(H, W), quality_filter=False, preprocessor=OraclePreprocessor())
    first = next(ex.extract_frames_generator("g", reader=reader_of(frames, 25.0, ())))
    assert first["frame"].shape == (W, H, 3) and np.array_equal(first["frame"], resize_linear_u8(frames[0], H, W))
    ex = OptimizedFrameExtractor(max_frames_per_video=1, frame_size=None, preprocessor=OraclePreprocessor())
    assert np.array_equal(next(ex.extract_frames_generator("g", reader=reader_of(frames, 25.0, ())))["frame"], frames[25])


def test_choose_optimal_strategy(monkeypatch):
    def probe(seconds, fps=25.0):
        return lambda path: (fps, seconds * fps)
    assert choose_optimal_strategy("v", probe(299.9)) == "uniform"
    assert choose_optimal_strategy("v", probe(300)) == "hybrid"
    assert choose_optimal_strategy("v", probe(3600)) == "hybrid"
    assert choose_optimal_strategy("v", probe(3600.1)) == "adaptive"
    assert choose_optimal_strategy("v", probe(3600.1, 10.0)) == "adaptive"
    assert choose_optimal_strategy("v", lambda path: (0.0, 10 ** 9)) == "uniform"               # fps = 0: duration 0
    assert choose_optimal_strategy("v", lambda path: (-1.0, 10 ** 9)) == "uniform"
    assert choose_optimal_strategy("v", lambda path: None) == "uniform"
    # the default probe: a cv2 whose capture does not open gives 'uniform'; one that does is asked for fps and frame count
    released = []

    class Capture:
        def __init__(self, path):
            self.path = path

        def isOpened(self):
            return self.path != "missing.mp4"

        def get(self, prop):
            return {5: 30.0, 7: 30.0 * 4000}[prop]

        def release(self):
            released.append(self.path)

    fake = types.SimpleNamespace(VideoCapture=Capture, CAP_PROP_FPS=5, CAP_PROP_FRAME_COUNT=7)
    monkeypatch.setitem(sys.modules, "cv2", fake)
    assert choose_optimal_strategy("missing.mp4") == "uniform"
    assert choose_optimal_strategy("long.mp4") == "adaptive" and released == ["long.mp4"]
    monkeypatch.setitem(sys.modules, "cv2", None)
    with pytest.raises(ImportError, match="probe="):
        choose_optimal_strategy("long.mp4")
    with pytest.raises(ImportError, match="reader="):
        OptimizedFrameExtractor(preprocessor=OraclePreprocessor()).extract_frames("long.mp4")
    with pytest.raises(ImportError, match="reader="):
        next(OptimizedFrameExtractor(preprocessor=OraclePreprocessor()).extract_frames_generator("long.mp4"))


def test_module_imports_without_gpu_opencv_or_torch():
    code = ("import sys; sys.modules['cv2'] = None; sys.modules['torch'] = None\n"
            "import video_quierer_amd.core.frame_extractor as m\n"
            "ex = m.OptimizedFrameExtractor(strategy='hybrid'); print(type(ex.sampler).__name__, m.choose_optimal_strategy('v', lambda p: (1.0, 400)))\n"
            "assert 'video_quierer_amd.preprocess' not in sys.modules and 'video_quierer_amd._lib' not in sys.modules")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["HybridFrameSampler", "hybrid"]


def test_install_dropin_registers_the_frame_extractor():
    code = ("import sys, video_quierer_amd\n"
            "video_quierer_amd.install_dropin(); video_quierer_amd.install_dropin()\n"
            "from core.frame_extractor import OptimizedFrameExtractor, choose_optimal_strategy\n"
            "import core.frame_extractor, video_quierer_amd.core.frame_extractor as own\n"
            "assert OptimizedFrameExtractor is own.OptimizedFrameExtractor is video_quierer_amd.OptimizedFrameExtractor\n"
            "assert core.frame_extractor is own and choose_optimal_strategy is own.choose_optimal_strategy\n"
            "assert len({id(m) for m in sys.modules.values() if getattr(m, '__file__', None) == own.__file__}) == 1\n"
            "print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_postprocess_plan_needs_no_device():
    from video_quierer_amd import _lib
    from video_quierer_amd.preprocess import POSTPROCESS_MAX_PIXELS, postprocess_plan
    lib = _lib.load()
    text = open(os.path.join(ROOT, "video-quierer_amd", "csrc", "preproc_kernels.h")).read()
    budget = int(re.search(r"constexpr int PP_LDS_BUDGET = (\d+);", text).group(1))
    red = int(re.search(r"constexpr int PP_RED_BYTES = (\d+);", text).group(1))
    assert POSTPROCESS_MAX_PIXELS == eval(re.search(r"constexpr int PP_MAX_PIXELS = ([^;]+);", text).group(1)) == 1 << 21
    assert budget <= 160 * 1024

    def lds_bytes(rows, out_w):                      # pp_lds_bytes: pixel rows padded to 16 bytes, grey rows, two halo rows
        return (rows + 2) * ((out_w * 3 + 15) // 16 * 16 + (out_w + 15) // 16 * 16) + red

    widths = list(range(1, 1025)) + [1025, 2048, 4096, 5000, 6000, 8192, 100000]
    unfused = 0
    for out_w in widths:
        for out_h in (1, 2, 31, 32, 33, 224, 1080, (1 << 21) // out_w):
            if out_h * out_w > POSTPROCESS_MAX_PIXELS:
                continue
            rows, bands, fused = postprocess_plan(out_h, out_w)
            assert rows >= 1 and bands == -(-out_h // rows), (out_h, out_w)
            if out_w <= 1024:
                assert fused
            if fused:
                assert lds_bytes(min(rows, out_h), out_w) <= lds_bytes(rows, out_w) <= budget
                assert rows == 32 or lds_bytes(rows + 1, out_w) > budget        # the most rows that fit, capped at 32
            else:
                assert lds_bytes(1, out_w) > budget and (rows, bands) == (out_h, 1)
                unfused += 1
    assert unfused and postprocess_plan(224, 224) == (32, 7, True)
    # bad arguments are refused with a message, not a crash
    r, b, f = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.vq_frame_postprocess_plan(0, 4, ctypes.byref(r), ctypes.byref(b), ctypes.byref(f)) == -1
    assert lib.vq_frame_postprocess_plan(4, 4, None, ctypes.byref(b), ctypes.byref(f)) == -1
    assert lib.vq_frame_postprocess_plan(2048, 1025, ctypes.byref(r), ctypes.byref(b), ctypes.byref(f)) == -1
    assert "2^21" in lib.vq_last_error().decode()
