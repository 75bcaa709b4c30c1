#!/usr/bin/env python3
"""Times FramePreprocessor.postprocess (resize + quality verdict + compaction in one device pass) next to the composition
it replaces, in the same process, alternating the two:
  host frames:    cv_resize (resize_list, CV_LINEAR) -> is_low_quality -> boolean indexing, three trips over the bus;
  device frames:  vq_frame_quality_u8(on_device=1) on the frames -> host verdict -> torch boolean indexing on the device
                  (equal sizes: the resize is a copy, which the composition is spared).
Cases: 64 host frames of 1080 x 1920 as a list -> 224 x 224, and 4,096 device-resident frames of 224 x 224 at equal
size, each with every frame kept and with every other frame dropped.  Both routes must give identical survivors before
anything is timed.  Per case: medians of --reps rounds after warm-up, each round = new call, composition, composition
again; host clock around calls that end in a device synchronise.  The two composition series give the run-to-run
spread; the new call passes when its median is not above the slower composition median (the faster one plus the spread).
usage: frame_postprocess_probe.py [--reps 20] [--only host|device] [--out FILE]
For kernel times and traffic counters run it under rocprofv3 (--kernel-trace --stats, or --pmc, each in a run of its
own) with --reps 3."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_quierer_amd import _lib
from video_quierer_amd.preprocess import CV_LINEAR, FramePreprocessor

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--only", choices=("host", "device"))
ap.add_argument("--out")
args = ap.parse_args()

pre = FramePreprocessor()
peek = FramePreprocessor()                   # reads a result left on the device without disturbing `pre`
lib = _lib.load()
dp = ctypes.POINTER(ctypes.c_double)
lines, failed = [], []


def say(text):
    print(text, flush=True)
    lines.append(text)


def clock(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def measure(name, new, comp):
    for _ in range(3):
        new(); comp()
    a, b, c = [], [], []
    for _ in range(args.reps):
        a.append(clock(new)); b.append(clock(comp)); c.append(clock(comp))
    ma, mb, mc = statistics.median(a), statistics.median(b), statistics.median(c)
    spread = abs(mb - mc)
    ok = ma <= max(mb, mc)
    if not ok:
        failed.append(name)
    say(f"{name:44s} {ma:9.3f} {min(a):9.3f} {mb:9.3f} {mc:9.3f} {spread:8.3f} {min(mb, mc) / ma:7.2f}x  {'ok' if ok else 'SLOWER'}")


say(f"{'case':44s} {'new ms':>9s} {'new min':>9s} {'comp ms':>9s} {'comp ms':>9s} {'spread':>8s} {'ratio':>8s}")
rng = np.random.default_rng(20261019)

if args.only in (None, "host"):
    n, h, w = 64, 1080, 1920
    for label, drop in (("all kept", False), ("half dropped", True)):
        frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
        if drop:
            for f in frames[1::2]:
                f //= 32
                f += 100
        res = {}

        def new():
            res["new"] = pre.postprocess_list(frames, (224, 224))

        def comp():
            small = pre.resize_list(frames, 224, 224, CV_LINEAR)
            low = pre.is_low_quality(small)
            res["comp"] = (small[~low], ~low)

        new(); comp()
        assert np.array_equal(res["new"][1], res["comp"][1]) and np.array_equal(res["new"][0], res["comp"][0])
        assert int(res["new"][1].sum()) == (n // 2 if drop else n), res["new"][1].sum()
        measure(f"{n} host 1080x1920 list -> 224x224, {label}", new, comp)
        del frames

if args.only in (None, "device"):
    n, h, w = 4096, 224, 224
    for label, drop in (("all kept", False), ("half dropped", True)):
        d = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
        if drop:
            d[1::2] = d[1::2] // 32 + 100
        torch.cuda.synchronize()
        mean, var = np.empty(n), np.empty(n)
        res = {}

        def new():
            res["new"] = pre.postprocess_device(d.data_ptr(), n, h, w, (224, 224))

        def comp():
            _lib.check(lib.vq_frame_quality_u8(pre._h, ctypes.c_void_p(d.data_ptr()), n, h, w, 1, mean.ctypes.data_as(dp), var.ctypes.data_as(dp)))
            keep = ~((mean < 20) | (mean > 235) | (var < 100))
            res["comp"] = (d[torch.from_numpy(keep).cuda()], keep)
            torch.cuda.synchronize()

        comp(); new()                        # the new result is read back before another call on its handle
        kept = int(res["new"][1].sum())
        assert kept == (n // 2 if drop else n) and np.array_equal(res["new"][1], res["comp"][1])
        assert np.array_equal(peek.postprocess_device(res["new"][0], kept, h, w, None, quality_filter=False, keep_on_device=False)[0],
                              res["comp"][0].cpu().numpy())
        measure(f"{n} device 224x224 equal size, {label}", new, comp)
        del d, res

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
if failed:
    sys.exit("slower than the composition beyond its spread: " + "; ".join(failed))
