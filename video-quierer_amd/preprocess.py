"""GPU frame preprocessing in front of the encoder: Pillow-exact resize and the
frame-quality statistics of the reference's frame extractor, over ``vq_resampler_*`` / ``vq_frame_quality_u8``.

  * :meth:`FramePreprocessor.stretch` — ``transforms.Resize((S, S))`` of reference
    src/core/feature_extractor.py:54-61 (PIL bilinear, antialiased);
  * :meth:`FramePreprocessor.clip_processor` — the CLIP image processor of the live path
    (reference video_search_overhaul.py:129-135, :218-221): short edge → 224 bicubic, centre crop 224;
  * :meth:`FramePreprocessor.cv_resize` — ``cv2.resize(frame, frame_size)`` of reference
    src/core/frame_extractor.py:283-284 (OpenCV INTER_LINEAR; parity unpinned);
  * :meth:`FramePreprocessor.quality` / :meth:`is_low_quality` — reference
    src/core/frame_extractor.py:301-316;
  * :meth:`FramePreprocessor.postprocess` — resize, quality verdict and compaction of a batch in one device pass
    (``vq_frame_postprocess_u8``): the per-frame loop of reference src/core/frame_extractor.py:279-293;
  * :meth:`FramePreprocessor.scene_change_scores` — ``AdaptiveFrameSampler._calculate_frame_difference`` of
    reference src/core/frame_extractor.py:168-186 for every consecutive pair of a batch (the samplers on top of
    it: :mod:`video_quierer_amd.core.frame_extractor`).
"""
import ctypes
from ctypes import c_double, c_int, c_int64, c_void_p
from typing import Optional, Tuple

import numpy as np

from . import _lib

BILINEAR, BICUBIC = 2, 3            # PIL.Image.Resampling values (VQ_RESAMPLE_*)
CV_LINEAR = 100                     # cv2.resize's default INTER_LINEAR (VQ_RESAMPLE_CV_LINEAR)
# geometry of the scene-change pass (csrc/preproc_kernels.h SC_CHUNK_FRAMES / SC_TILE; tests read both and compare)
SCENE_CHUNK_FRAMES = 8              # frames one workgroup walks
SCENE_TILE_PIXELS = 8192            # pixels one workgroup owns
POSTPROCESS_MAX_PIXELS = 1 << 21    # out_h * out_w the integer quality verdict is proven for (PP_MAX_PIXELS)


def clip_processor_geometry(h: int, w: int, size: int = 224, crop: int = 224) -> Tuple[int, int, int, int]:
    """(resized_h, resized_w, crop_top, crop_left) of the CLIP image processor for an h x w frame."""
    rh, rw, top, left = c_int(), c_int(), c_int(), c_int()
    _lib.check(_lib.load().vq_clip_processor_geometry(int(h), int(w), int(size), int(crop), ctypes.byref(rh),
                                                      ctypes.byref(rw), ctypes.byref(top), ctypes.byref(left)))
    return rh.value, rw.value, top.value, left.value


def postprocess_plan(out_h: int, out_w: int) -> Tuple[int, int, bool]:
    """(band_rows, n_bands, fused) of the post-processing pass for an out_h x out_w output; needs no device."""
    rows, bands, fused = c_int(), c_int(), c_int()
    _lib.check(_lib.load().vq_frame_postprocess_plan(int(out_h), int(out_w), ctypes.byref(rows), ctypes.byref(bands),
                                                     ctypes.byref(fused)))
    return rows.value, bands.value, bool(fused.value)


def postprocess_size(h: int, w: int, frame_size, always_resize: bool = False) -> Tuple[int, int]:
    """(out_h, out_w) of the reference's resize step for an h x w frame (frame_extractor.py:283-284): no resize for
    ``frame_size`` None or — the reference's quirk — when ``(h, w) == tuple(frame_size)``; otherwise
    ``cv2.resize(frame, frame_size)``, whose dsize is (WIDTH, HEIGHT).  ``always_resize``: the generator's form
    (:342-343), which resizes whenever ``frame_size`` is set."""
    if frame_size is None or not tuple(frame_size):
        return int(h), int(w)
    fw, fh = int(frame_size[0]), int(frame_size[1])
    if fw <= 0 or fh <= 0:
        raise ValueError(f"frame_size must be positive, got {tuple(frame_size)}")
    if not always_resize and (int(h), int(w)) == (fw, fh):
        return int(h), int(w)
    return fh, fw


def _frames(frames) -> np.ndarray:
    a = np.asarray(frames)
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4 or a.shape[3] != 3:
        raise ValueError(f"expected uint8 frames [n, h, w, 3], got shape {a.shape}")
    if a.dtype != np.uint8:
        raise TypeError(f"expected uint8 pixels, got {a.dtype}")
    return np.ascontiguousarray(a)


def _frame_list(frames):
    """A list of separately allocated uint8 [h, w, 3] frames of one size → (contiguous arrays, h, w)."""
    arrs = [np.ascontiguousarray(f) for f in frames]
    if not arrs:
        return arrs, 0, 0
    h, w = arrs[0].shape[:2]
    for a in arrs:
        if a.dtype != np.uint8 or a.shape != (h, w, 3):
            raise ValueError(f"expected uint8 frames of one shape ({h}, {w}, 3), got {a.dtype} {a.shape}")
    return arrs, h, w


def _window(crop, out_h, out_w):
    """(top, left, h, w) of the crop; default: the whole resized frame."""
    return tuple(int(v) for v in crop) if crop is not None else (0, 0, int(out_h), int(out_w))


class FramePreprocessor:
    def __init__(self, device: Optional[int] = None):
        self.device = _lib.init(device)
        h = c_void_p()
        _lib.check(_lib.load().vq_resampler_create(ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().vq_resampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown: module globals may already be gone
            pass

    def set_stream(self, stream_ptr: Optional[int]):
        _lib.check(_lib.load().vq_resampler_set_stream(self._h, c_void_p(stream_ptr or 0)))

    def synchronize(self):
        _lib.check(_lib.load().vq_resampler_synchronize(self._h))

    # -- resize ---------------------------------------------------------------
    def resize(self, frames, out_h: int, out_w: int, filter: int = BILINEAR,
               crop: Optional[Tuple[int, int, int, int]] = None, keep_on_device: bool = False):
        """``Image.resize((out_w, out_h), filter)`` of every frame, then the window
        ``crop = (top, left, h, w)`` (default: the whole resized frame).  → uint8 [n, crop_h, crop_w, 3], or with
        ``keep_on_device`` the device address of that array (valid until the next call on this object)."""
        a = _frames(frames)
        n, h, w = a.shape[:3]
        top, left, ch, cw = _window(crop, out_h, out_w)
        out = None if keep_on_device else np.empty((n, ch, cw, 3), dtype=np.uint8)
        _lib.check(_lib.load().vq_resampler_run_u8(self._h, a.ctypes.data_as(c_void_p), n, h, w, int(filter), int(out_h),
                                                   int(out_w), top, left, ch, cw,
                                                   out.ctypes.data_as(c_void_p) if out is not None else None))
        if out is not None:
            return out
        ptr, nbytes = c_void_p(), c_int64()
        _lib.check(_lib.load().vq_resampler_device_output(self._h, ctypes.byref(ptr), ctypes.byref(nbytes)))
        return ptr.value

    def resize_list(self, frames, out_h: int, out_w: int, filter: int = BILINEAR,
                    crop: Optional[Tuple[int, int, int, int]] = None) -> np.ndarray:
        """:meth:`resize` for a list of separately allocated uint8 [h, w, 3] frames of one size (no stacking copy)."""
        arrs, h, w = _frame_list(frames)
        if not arrs:
            return np.empty((0, out_h, out_w, 3), np.uint8)
        top, left, ch, cw = _window(crop, out_h, out_w)
        out = np.empty((len(arrs), ch, cw, 3), dtype=np.uint8)
        ptrs = (c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        _lib.check(_lib.load().vq_resampler_run_u8_list(self._h, ptrs, len(arrs), h, w, int(filter), int(out_h), int(out_w),
                                                        top, left, ch, cw, out.ctypes.data_as(c_void_p)))
        return out

    def resize_device(self, src_ptr: int, n: int, h: int, w: int, out_h: int, out_w: int, filter: int = BILINEAR,
                      crop: Optional[Tuple[int, int, int, int]] = None, dst_ptr: Optional[int] = None) -> int:
        """Device-resident frames in, device result out; asynchronous on the handle's stream.  → device address."""
        top, left, ch, cw = _window(crop, out_h, out_w)
        _lib.check(_lib.load().vq_resampler_run_u8_device(self._h, c_void_p(src_ptr), int(n), int(h), int(w), int(filter),
                                                          int(out_h), int(out_w), top, left, ch, cw, c_void_p(dst_ptr or 0)))
        if dst_ptr:
            return dst_ptr
        ptr = c_void_p()
        _lib.check(_lib.load().vq_resampler_device_output(self._h, ctypes.byref(ptr), None))
        return ptr.value

    def cv_resize(self, frames, dsize: Tuple[int, int], **kw):
        """``cv2.resize(frame, dsize)`` (dsize = (width, height), INTER_LINEAR) of every frame — the resize of
        ``OptimizedFrameExtractor.extract_frames`` (reference frame_extractor.py:283-284).  Restated from OpenCV's
        published algorithm; parity unpinned (OpenCV is not installed in the build container)."""
        return self.resize(frames, int(dsize[1]), int(dsize[0]), CV_LINEAR, **kw)

    def stretch(self, frames, size: int = 224, **kw):
        """E1's ``transforms.Resize((S, S))`` (reference feature_extractor.py:55)."""
        return self.resize(frames, size, size, BILINEAR, **kw)

    def clip_processor(self, frames, size: int = 224, crop: int = 224, **kw):
        """The CLIP image processor's resize + centre crop (before its rescale/normalise, which the encoder's
        patchify kernel applies)."""
        a = _frames(frames)
        rh, rw, top, left = clip_processor_geometry(a.shape[1], a.shape[2], size, crop)
        return self.resize(a, rh, rw, BICUBIC, crop=(top, left, crop, crop), **kw)

    # -- quality filter -------------------------------------------------------
    def quality(self, frames) -> Tuple[np.ndarray, np.ndarray]:
        """→ (mean_brightness[n], laplacian_var[n]) float64 of BGR uint8 frames (reference frame_extractor.py:305-313)."""
        a = _frames(frames)
        n, h, w = a.shape[:3]
        mean, var = np.empty(n, np.float64), np.empty(n, np.float64)
        _lib.check(_lib.load().vq_frame_quality_u8(self._h, a.ctypes.data_as(c_void_p), n, h, w, 0,
                                                   mean.ctypes.data_as(ctypes.POINTER(c_double)),
                                                   var.ctypes.data_as(ctypes.POINTER(c_double))))
        return mean, var

    def is_low_quality(self, frames) -> np.ndarray:
        """``OptimizedFrameExtractor._is_low_quality`` per frame: very dark / very bright (mean < 20 or > 235) or
        blurry (Laplacian variance < 100)."""
        mean, var = self.quality(frames)
        return (mean < 20) | (mean > 235) | (var < 100)

    # -- resize + quality filter + compaction in one pass ----------------------
    def postprocess(self, frames, frame_size=(224, 224), quality_filter: bool = True, keep_on_device: bool = False,
                    always_resize: bool = False):
        """What ``OptimizedFrameExtractor.extract_frames`` does to each sampled frame (reference
        frame_extractor.py:279-293), for a batch of BGR uint8 frames [n, h, w, 3] in one device pass: the resize of
        :func:`postprocess_size`, the low-quality verdict of :meth:`is_low_quality` on the resized frame, survivors
        compacted in input order.  → (kept frames uint8 [n_kept, out_h, out_w, 3], keep bool[n], sums int64[n, 3] =
        {sum of bytes, sum L, sum L^2} of each resized frame).  With ``keep_on_device`` the first element is the
        device address of the kept frames instead (valid until the next call on this object)."""
        a = _frames(frames)
        n, h, w = a.shape[:3]
        return self._post(lambda lib, *rest: lib.vq_frame_postprocess_u8(self._h, a.ctypes.data_as(c_void_p), n, h, w, 0, *rest),
                          n, h, w, frame_size, quality_filter, keep_on_device, always_resize)

    def postprocess_list(self, frames, frame_size=(224, 224), quality_filter: bool = True, keep_on_device: bool = False,
                         always_resize: bool = False):
        """:meth:`postprocess` for a list of separately allocated uint8 [h, w, 3] frames of one size (what sampler
        records hold; no stacking copy)."""
        arrs, h, w = _frame_list(frames)
        if not arrs:
            return np.empty((0, 0, 0, 3), np.uint8), np.zeros(0, bool), np.zeros((0, 3), np.int64)
        ptrs = (c_void_p * len(arrs))(*[f.ctypes.data for f in arrs])
        return self._post(lambda lib, *rest: lib.vq_frame_postprocess_u8_list(self._h, ptrs, len(arrs), h, w, *rest),
                          len(arrs), h, w, frame_size, quality_filter, keep_on_device, always_resize)

    def postprocess_device(self, ptr: int, n: int, h: int, w: int, frame_size=(224, 224), quality_filter: bool = True,
                           keep_on_device: bool = True, always_resize: bool = False):
        """:meth:`postprocess` over device-resident frames [n, h, w, 3] at ``ptr`` (any alignment)."""
        n, h, w = int(n), int(h), int(w)
        return self._post(lambda lib, *rest: lib.vq_frame_postprocess_u8(self._h, c_void_p(ptr), n, h, w, 1, *rest),
                          n, h, w, frame_size, quality_filter, keep_on_device, always_resize)

    def _post(self, call, n, h, w, frame_size, quality_filter, keep_on_device, always_resize):
        if h <= 0 or w <= 0:
            raise ValueError(f"frames must not be empty, got {h} x {w}")
        out_h, out_w = postprocess_size(h, w, frame_size, always_resize)
        resized = frame_size is not None and bool(tuple(frame_size))      # None: out 0 x 0, "the frames as given"
        out = None if keep_on_device else np.empty((n, out_h, out_w, 3), np.uint8)
        keep, sums, kept = np.zeros(n, np.uint8), np.zeros((n, 3), np.int64), c_int64(0)
        _lib.check(call(_lib.load(), out_h if resized else 0, out_w if resized else 0, 1 if quality_filter else 0,
                        out.ctypes.data_as(c_void_p) if out is not None else None, ctypes.byref(kept),
                        keep.ctypes.data_as(c_void_p), sums.ctypes.data_as(c_void_p)))
        if out is not None:
            return out[:kept.value], keep.astype(bool), sums
        ptr = c_void_p()
        _lib.check(_lib.load().vq_resampler_device_output(self._h, ctypes.byref(ptr), None))
        return ptr.value, keep.astype(bool), sums

    # -- scene-change score ---------------------------------------------------
    def scene_change_scores(self, frames, prev=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """→ (score[n], mse[n], hist_diff[n]) float64 of BGR uint8 frames: entry i compares frame i - 1 with frame i
        (reference frame_extractor.py:168-186); entry 0 compares ``prev`` (one frame of the same size) with frame 0,
        or is 0.0 without one, like the reference's first frame."""
        a = _frames(frames)
        n, h, w = a.shape[:3]
        p = None
        if prev is not None:
            p = _frames(prev)
            if p.shape != (1, h, w, 3):
                raise ValueError(f"prev must be one frame of shape ({h}, {w}, 3), got {p.shape[1:] if p.shape[0] == 1 else p.shape}")
        return self._scene(a.ctypes.data_as(c_void_p), n, h, w, 0, p.ctypes.data_as(c_void_p) if p is not None else None)

    def scene_change_scores_device(self, ptr: int, n: int, h: int, w: int, prev_ptr: Optional[int] = None):
        """:meth:`scene_change_scores` over device-resident frames [n, h, w, 3] at ``ptr`` (any alignment) and an
        optional device-resident predecessor frame at ``prev_ptr``.  Results are host arrays."""
        return self._scene(c_void_p(ptr), int(n), int(h), int(w), 1, c_void_p(prev_ptr) if prev_ptr else None)

    def _scene(self, frames_p, n, h, w, on_device, prev_p):
        score, mse, hist = (np.empty(n, np.float64) for _ in range(3))
        dp = ctypes.POINTER(c_double)
        _lib.check(_lib.load().vq_frame_scene_scores_u8(self._h, frames_p, n, h, w, on_device, prev_p, score.ctypes.data_as(dp),
                                                        mse.ctypes.data_as(dp), hist.ctypes.data_as(dp)))
        return score, mse, hist
