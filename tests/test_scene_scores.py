"""GPU (`-m gpu`): vq_frame_scene_scores_u8 / FramePreprocessor.scene_change_scores — the scene-change score of
reference src/core/frame_extractor.py:168-186 for every consecutive pair of a batch — against a numpy restatement,
with `==` on all three arrays: every step is an exact integer or one correctly rounded fp64 operation in a fixed
order, so there is no tolerance.  Shapes are the smallest at which the kernel's paths differ (byte loads / 16-byte
loads, one tile / several, a partial last tile, one frame chunk / several)."""
import ctypes

import numpy as np
import pytest
import torch        # before the library binds the GPU: torch brings its own copy of the HIP runtime

from oracle.quality_oracle import bgr_to_gray
from video_quierer_amd.preprocess import SCENE_CHUNK_FRAMES as F, SCENE_TILE_PIXELS as TILE

pytestmark = pytest.mark.gpu


def restate(frames, prev=None):
    """(score, mse, hist_diff) float64 [n] of uint8 BGR frames [n, h, w, 3]; entry 0 is 0.0 without `prev`."""
    frames = np.asarray(frames)
    n, h, w = frames.shape[:3]
    greys = [bgr_to_gray(f) for f in frames]
    hists = [np.bincount(g.ravel(), minlength=256) for g in greys]
    if prev is not None:
        g = bgr_to_gray(prev)
        before = (g, np.bincount(g.ravel(), minlength=256))
    score, mse, chi = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        if i == 0 and prev is None:
            continue
        ga, ha = before if i == 0 else (greys[i - 1], hists[i - 1])
        gb, hb = greys[i], hists[i]
        s = int(((ga.astype(np.int64) - gb.astype(np.int64)) ** 2).sum())
        mse[i] = float(s) / float(h * w)
        c = 0.0
        for b in range(256):
            if ha[b] != 0:
                d = float(int(ha[b]) - int(hb[b]))
                c += d * d / float(ha[b])
        chi[i] = c
        score[i] = mse[i] + c * 0.01
    return score, mse, chi


def same(got, want):
    for g, w, name in zip(got, want, ("score", "mse", "hist_diff")):
        assert g.dtype == np.float64 and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, g[:8], w[:8])


@pytest.fixture(scope="module")
def pre(gpu_lib):
    from video_quierer_amd.preprocess import FramePreprocessor
    p = FramePreprocessor()
    yield p
    p.close()


def noise(seed, n, h, w):
    return np.random.default_rng([20261018, seed, n, h, w]).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def clip70():
    """70 frames of 37 x 53 and their restated scores, shared by the frame-count, prev, slice and device tests."""
    frames = noise(1, 70, 37, 53)
    return frames, restate(frames)


def test_geometry_constants():
    assert F >= 8 and TILE == 8192


@pytest.mark.parametrize("h,w", [(37, 53),             # 5,883 bytes: byte loads, a partial (only) tile
                                 (64, 64),             # 16-byte loads, half a tile
                                 (224, 224),           # 16-byte loads, seven tiles, the last one an eighth full
                                 (1, 1), (1, 7),
                                 (3, 2731),            # TILE + 1 pixels, byte loads: one pixel in the second tile
                                 (16, 513),            # TILE + 16 pixels, 16-byte loads: one group in the second tile
                                 (128, 128)])          # exactly two full tiles
def test_shapes(pre, h, w):
    assert (h, w) != (3, 2731) or h * w == TILE + 1
    assert (h, w) != (16, 513) or h * w == TILE + 16
    frames = noise(2, 5, h, w)
    same(pre.scene_change_scores(frames), restate(frames))
    same(pre.scene_change_scores(frames[1:], prev=frames[0]), [a[1:] for a in restate(frames)])


@pytest.mark.parametrize("n", [1, 2, 3, F, F + 1, 2 * F + 3, 70])
def test_frame_counts(pre, clip70, n):
    frames, want = clip70
    got = pre.scene_change_scores(frames[:n])
    same(got, [a[:n] for a in want])                   # scores of a prefix are a prefix of the scores
    assert got[0][0] == 0.0 and got[1][0] == 0.0 and got[2][0] == 0.0
    if n == 1:
        assert got[0].tolist() == [0.0]


@pytest.mark.parametrize("h,w", [(37, 53), (64, 64)])
def test_content(pre, h, w):
    rng = np.random.default_rng([5, h, w])
    npix = h * w
    black, white = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    # identical neighbours score exactly 0
    got = pre.scene_change_scores(np.stack([a, a, a, black, black]))
    assert got[0][[1, 2, 4]].tolist() == [0.0] * 3 and got[1][[1, 2, 4]].tolist() == [0.0] * 3 and got[2][[1, 2, 4]].tolist() == [0.0] * 3
    # black -> white -> black: every pixel differs by 255 and moves from one bin to another
    frames = np.stack([black, white, black])
    got = pre.scene_change_scores(frames)
    same(got, restate(frames))
    for i in (1, 2):
        assert got[1][i] == 65025.0 and got[2][i] == float(npix) and got[0][i] == 65025.0 + npix * 0.01
    # a slow ramp: a gradient that moves up by 1, 2, ... 9 grey levels per frame, so scores fall on both sides of 30
    grad = (np.arange(npix).reshape(h, w) * 100 // npix + 20).astype(np.int64)
    ramp = np.stack([np.repeat((grad + k * (k + 1) // 2)[..., None], 3, -1) for k in range(10)]).astype(np.uint8)
    want = restate(ramp)
    assert (want[0][1:] < 30).sum() >= 3 and (want[0][1:] > 30).sum() >= 3
    same(pre.scene_change_scores(ramp), want)
    # only two grey values, in changing proportions
    two = np.where(rng.random((6, h, w, 1)) < np.linspace(0.1, 0.9, 6)[:, None, None, None], 200, 17).astype(np.uint8).repeat(3, -1)
    same(pre.scene_change_scores(two), restate(two))
    # letterboxed frames: flat bars (whole waves of one grey value) above and below noise, the bars changing level
    bars = np.stack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(4)])
    for i, level in enumerate((9, 9, 200, 16)):
        bars[i, :h // 3] = level
        bars[i, -(h // 4):] = 255 - level
    same(pre.scene_change_scores(bars), restate(bars))
    # coloured pixels: the grey conversion's rounding matters
    same(pre.scene_change_scores(np.stack([a, a[..., ::-1], a])), restate(np.stack([a, a[..., ::-1], a])))


def test_constant_frames_fill_one_bin(pre):
    """300 x 300 frames of one grey value each: 90,000 pixels in one bin (more than a 16-bit count holds, and every lane
    of a wave adds to the same LDS word), 8,192 in a tile's bin."""
    levels = [0, 255, 7, 7, 130, 131, 255, 0, 64]
    frames = np.stack([np.full((300, 300, 3), v, np.uint8) for v in levels])
    want = restate(frames)
    got = pre.scene_change_scores(frames)
    same(got, want)
    assert got[1][1] == 65025.0 and got[2][1] == 90000.0 and got[0][1] == 65025.0 + 90000 * 0.01
    assert got[0][3] == 0.0 and got[1][5] == 1.0 and got[2][5] == 90000.0


def test_largest_frame(pre):
    """h * w = 2^24 exactly: 2^24 pixels in one bin, a squared-difference sum of 2^24 * 255^2, 2,048 tiles."""
    frames = np.zeros((2, 4096, 4096, 3), np.uint8)
    frames[1] = 255
    score, mse, chi = pre.scene_change_scores(frames)
    assert mse.tolist() == [0.0, 65025.0] and chi.tolist() == [0.0, float(1 << 24)]
    assert score[1] == 65025.0 + float(1 << 24) * 0.01


def test_prev(pre, clip70):
    frames, want = clip70
    frames, want = frames[:2 * F + 3], [a[:2 * F + 3] for a in want]
    for cut in (1, 2, F, F + 1):                       # the tail of a clip with the frame before it == the clip's tail
        same(pre.scene_change_scores(frames[cut:], prev=frames[cut - 1]), [a[cut:] for a in want])
    same(pre.scene_change_scores(frames[3], prev=frames[2]), [a[3:4] for a in want])        # one frame, one prev
    got = pre.scene_change_scores(frames[4:9])         # no prev: entry 0 is 0.0, the rest is unchanged
    assert got[0][0] == 0.0 and got[1][0] == 0.0 and got[2][0] == 0.0
    same([g[1:] for g in got], [a[5:9] for a in want])
    with pytest.raises(ValueError):
        pre.scene_change_scores(frames[:3], prev=frames[0, :5])
    assert [len(a) for a in pre.scene_change_scores(frames[:0])] == [0, 0, 0]


def test_host_slices(pre, clip70, monkeypatch):
    frames, want = clip70
    monkeypatch.setenv("VQ_AMD_SCENE_SLICE_BYTES", str(3 * 37 * 53 * 3 + 100))        # three frames per slice
    same(pre.scene_change_scores(frames[:10]), [a[:10] for a in want])                  # slices 3 + 3 + 3 + 1
    same(pre.scene_change_scores(frames[1:10], prev=frames[0]), [a[1:10] for a in want])
    monkeypatch.setenv("VQ_AMD_SCENE_SLICE_BYTES", "1")                                 # smaller than a frame: one per slice
    same(pre.scene_change_scores(frames[:5]), [a[:5] for a in want])
    wide = noise(3, 10, 64, 64)                                                         # the 16-byte-load kernel behind slices
    monkeypatch.setenv("VQ_AMD_SCENE_SLICE_BYTES", str(3 * 64 * 64 * 3))
    same(pre.scene_change_scores(wide), restate(wide))


def test_device_form(pre, clip70):
    for frames, want in (clip70, (noise(4, 2 * F + 3, 64, 64), None)):
        frames = frames[:2 * F + 3]
        want = [a[:2 * F + 3] for a in want] if want is not None else restate(frames)
        n, h, w = frames.shape[:3]
        d = torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        same(pre.scene_change_scores_device(d.data_ptr(), n, h, w), want)
        same(pre.scene_change_scores(frames), want)
        # the same bytes one byte off alignment: a uint8 tensor sliced [1:], viewed as frames
        flat = torch.empty(frames.size + 1, dtype=torch.uint8, device="cuda")
        off = flat[1:]
        off.copy_(d.reshape(-1))
        torch.cuda.synchronize()
        assert off.data_ptr() % 16 == 1
        same(pre.scene_change_scores_device(off.data_ptr(), n, h, w), want)
        # prev_ptr: a frame in another allocation, and the frame in front of the batch
        p = d[2].clone()
        torch.cuda.synchronize()
        same(pre.scene_change_scores_device(d[3:].data_ptr(), n - 3, h, w, prev_ptr=p.data_ptr()), [a[3:] for a in want])
        same(pre.scene_change_scores_device(off[3 * h * w * 3:].data_ptr(), n - 3, h, w, prev_ptr=off[2 * h * w * 3:].data_ptr()),
             [a[3:] for a in want])


def test_scratch_batches(pre, clip70, monkeypatch):
    """More frames than the partials' scratch budget holds go through in batches; a batch's first pair needs the frame
    before it.  A budget of one byte makes batches of one frame chunk (F frames), for host and device frames."""
    frames, want = clip70
    monkeypatch.setenv("VQ_AMD_SCENE_SCRATCH_BYTES", "1")
    same(pre.scene_change_scores(frames), want)                                        # 70 frames: F-frame batches
    same(pre.scene_change_scores(frames[1:2 * F + 2], prev=frames[0]), [a[1:2 * F + 2] for a in want])
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    same(pre.scene_change_scores_device(d.data_ptr(), 70, 37, 53), want)
    wide = noise(9, 2 * F + 3, 64, 64)
    same(pre.scene_change_scores(wide), restate(wide))


def test_calls_on_one_handle_are_independent(pre):
    """quality(), stretch() and scene_change_scores() share the handle's staging and scratch buffers."""
    frames = noise(6, 11, 90, 160)
    other = noise(7, 4, 224, 224)
    q0, s0, c0, c1 = pre.quality(frames), pre.stretch(frames), pre.scene_change_scores(frames), pre.scene_change_scores(other)
    same(c0, restate(frames))
    for _ in range(2):
        same(pre.scene_change_scores(frames), c0)
        q = pre.quality(frames)
        assert np.array_equal(q[0], q0[0]) and np.array_equal(q[1], q0[1])
        same(pre.scene_change_scores(other), c1)
        assert np.array_equal(pre.stretch(frames), s0)
        same(pre.scene_change_scores(frames), c0)


def test_errors(pre, gpu_lib):
    lib = gpu_lib.load()
    buf = np.zeros(64, np.uint8)
    out = np.full(4, -7.0)
    fp, dp = buf.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def rc_and_message(*args):
        rc = lib.vq_frame_scene_scores_u8(pre._h, *args)
        return rc, (lib.vq_last_error() or b"").decode()

    rc, msg = rc_and_message(fp, 1, 4097, 4096, 0, None, dp, None, None)                # h * w = 2^24 + 4096
    assert rc == -1 and "too large" in msg
    rc, msg = rc_and_message(fp, 65536, 1, 1, 0, None, dp, None, None)
    assert rc == -1 and "65535" in msg
    rc, msg = rc_and_message(fp, 1, 2, 2, 0, None, None, None, None)                    # no score array
    assert rc == -1 and "vq_frame_scene_scores_u8" in msg
    rc, msg = rc_and_message(None, 1, 2, 2, 0, None, dp, None, None)
    assert rc == -1 and msg
    assert rc_and_message(fp, 1, 0, 2, 0, None, dp, None, None)[0] == -1
    assert rc_and_message(None, 0, 2, 2, 0, None, None, None, None)[0] == 0             # n == 0: nothing to do
    assert out.tolist() == [-7.0] * 4                                                   # nothing was written
    with pytest.raises(ValueError):
        pre.scene_change_scores(np.zeros((2, 4, 4, 4), np.uint8))
    with pytest.raises(TypeError):
        pre.scene_change_scores(np.zeros((2, 4, 4, 3), np.float32))
    # mse / hist_diff are optional
    frames = noise(8, 3, 8, 8)
    sc = np.empty(3)
    assert lib.vq_frame_scene_scores_u8(pre._h, frames.ctypes.data_as(ctypes.c_void_p), 3, 8, 8, 0, None,
                                        sc.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None) == 0
    assert np.array_equal(sc, restate(frames)[0])


def four_scene_clip():
    """64 frames of 64 x 64: four scenes of 16 frames, grey levels 40 / 110 / 180 / 250 plus per-pixel noise in
    [-3, 3] (the same on all three channels, so grey == the value), hard cuts at frames 16, 32 and 48."""
    rng = np.random.default_rng(20261018)
    levels = np.repeat([40, 110, 180, 250], 16)
    v = np.clip(levels[:, None, None] + rng.integers(-3, 4, (64, 64, 64)), 0, 255).astype(np.uint8)
    return np.repeat(v[..., None], 3, -1)


def test_adaptive_sampler_end_to_end(pre):
    """AdaptiveFrameSampler on the four-scene clip takes exactly the cuts.  Restated scores of this clip (computed on
    the CPU): the largest score inside a scene is 8.47 (3.5x below the threshold of 30), the smallest score at a cut
    is 4948.7 (165x above it)."""
    from video_quierer_amd.core.frame_extractor import AdaptiveFrameSampler, select_scene_changes
    frames = four_scene_clip()
    want = restate(frames)[0]
    cuts = np.zeros(64, bool)
    cuts[[16, 32, 48]] = True
    assert want[~cuts].max() * 2 <= 30.0 <= want[cuts].min() / 2          # both margins are at least 2x
    recs = AdaptiveFrameSampler().sample(frames, fps=30)                      # the default scorer: a FramePreprocessor
    assert [r["frame_number"] for r in recs] == [0, 16, 32, 48]
    assert [r["frame_number"] for r in recs] == select_scene_changes(want, 30)[0]
    assert [r["scene_change_score"] for r in recs] == [0.0] + want[cuts].tolist()
    assert all(np.array_equal(r["frame"], frames[r["frame_number"]]) for r in recs)
    assert [r["timestamp"] for r in recs] == [0.0, 16 / 30, 32 / 30, 48 / 30]
    # in chunks of 10 frames: the same records
    chunked = AdaptiveFrameSampler().sample_chunks([frames[i:i + 10] for i in range(0, 64, 10)], fps=30)
    assert [(r["frame_number"], r["scene_change_score"]) for r in chunked] == [(r["frame_number"], r["scene_change_score"]) for r in recs]
