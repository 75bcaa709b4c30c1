#!/usr/bin/env python3
"""Times the scene-change pass (vq_frame_scene_scores_u8, device form) on device-resident frames, next to
vq_frame_quality_u8(on_device=1) on the same frames in the same process — the existing kernel that streams the
same bytes.  Inputs: 256 x 1080p and 4,096 x 224 x 224, random and constant-frame content.  Per input: the median
of --reps calls after warm-up, timed with HIP events on the handle's stream (both calls return when their host
results are complete, so an interval holds the kernels, the result copy and the launch gaps); frames/s; source bytes
over time and that as a share of the 8 TB/s HBM peak (VERDICT.md quotes 6.0-6.3 TB/s for a streaming read).
usage: scene_scores_probe.py [--reps 20] [--only 1080p|224] [--content random|constant] [--out FILE]
For kernel times and traffic counters run it under rocprofv3 (--kernel-trace --stats, or --pmc, each in a run of its
own) with --reps 3."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_quierer_amd import _lib
from video_quierer_amd.preprocess import FramePreprocessor

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--only", choices=("1080p", "224"))
ap.add_argument("--content", choices=("random", "constant"))
ap.add_argument("--out")
args = ap.parse_args()

PEAK = 8.0e12
pre = FramePreprocessor()
st = torch.cuda.Stream()
pre.set_stream(st.cuda_stream)
lib = _lib.load()
dp = ctypes.POINTER(ctypes.c_double)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(call, reps):
    for _ in range(3):
        call()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


say(f"{'input':28s} {'kernel':8s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'frames/s':>12s} {'TB/s':>7s} {'of 8 TB/s':>10s}")
for name, n, h, w in (("1080p", 256, 1080, 1920), ("224", 4096, 224, 224)):
    if args.only and args.only != name:
        continue
    for content in ("random", "constant"):
        if args.content and args.content != content:
            continue
        if content == "random":
            d = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
        else:                                            # every frame one grey value, a different one per frame
            d = (torch.arange(n, device="cuda") % 251).to(torch.uint8).view(n, 1, 1, 1).expand(n, h, w, 3).contiguous()
        torch.cuda.synchronize()
        a, b, c = (np.empty(n) for _ in range(3))

        def scene():
            _lib.check(lib.vq_frame_scene_scores_u8(pre._h, ctypes.c_void_p(d.data_ptr()), n, h, w, 1, None, a.ctypes.data_as(dp),
                                                    b.ctypes.data_as(dp), c.ctypes.data_as(dp)))

        def quality():
            _lib.check(lib.vq_frame_quality_u8(pre._h, ctypes.c_void_p(d.data_ptr()), n, h, w, 1, a.ctypes.data_as(dp), b.ctypes.data_as(dp)))

        nbytes = n * h * w * 3
        for kname, call in (("scene", scene), ("quality", quality)):
            med, lo, hi = timed(call, args.reps)
            rate = nbytes / (med * 1e-3)
            say(f"{n:5d} x {h}x{w} {content:9s} {kname:8s} {med:10.3f} {lo:8.3f} {hi:8.3f} {n / (med * 1e-3):12.0f} {rate / 1e12:7.2f} {rate / PEAK:10.1%}")
        del d
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
