#!/usr/bin/env python3
"""Warped clip alignment latency over 262,144 x 512 video-like unit rows: 512 "videos" of 512 rows, each a random walk
(v[i+1] = normalize(v[i] + 0.2 g / sqrt(dim))), positions = the frame number.  The clips are cut from video 300 at twice the
pace (every second frame from frame 100 on) plus noise of norm 0.1:
  align_clip(m = 64, k = 10)                    and with alignment=True (the winners' DP again, tables, the walk back)
  align_clip(m = 256, k = 10)                   likewise
  search_sequence(m = 64, max_gap = 8)          the nearest existing call at m = 64: the same distance pass, one DP launch
each as the wall time of the host-synchronous call (median after warm-up) and as device time by kernel class from the index's
event brackets: exact_dist_f64chain is the distance pass — the floor this design accepts, printed beside every call —,
sequence_dp the alignment kernels (DP, finish, tables and walk), select_topk the last DP row's keys, the selection and the
counters.  The answer of the first call is checked: video 300 first, its stretch found to within two frames.
  one group of 262,144 rows, m = 64             the global form's bound: one workgroup walks the whole index 64 times
usage: align_probe.py OUTDIR [--quick]   (writes OUTDIR/probe.txt)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex  # noqa: E402

N, D, VIDEO = 262_144, 512, 512
SRC, FIRST = 300, 100


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def classes(idx, fn, reps):
    idx.profile_begin()
    for _ in range(reps):
        fn()
    return {k: round(v["ms"] / reps, 4) for k, v in idx.profile_end().items() if v["launches"]}


def main():
    out = sys.argv[1]
    quick = "--quick" in sys.argv
    reps = 3 if quick else 15
    os.makedirs(out, exist_ok=True)
    lines = []

    def say(*a):
        line = " ".join(str(x) for x in a)
        print(line, flush=True)
        lines.append(line)
        with open(os.path.join(out, "probe.txt"), "w") as f:      # kept current: a later step may take long
            f.write("\n".join(lines) + "\n")

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(4000)
    videos = N // VIDEO
    rows = torch.empty((videos, VIDEO, D), device=dev)
    x = torch.randn((videos, D), device=dev, generator=g)
    x /= x.norm(dim=1, keepdim=True)
    for i in range(VIDEO):
        rows[:, i] = x
        x = x + torch.randn((videos, D), device=dev, generator=g) * (0.2 / D ** 0.5)
        x /= x.norm(dim=1, keepdim=True)
    rows = rows.reshape(N, D)
    idx = OptimizedHNSWIndex(dimension=D)
    torch.cuda.synchronize()
    idx.add_device(rows.data_ptr(), N, range(N), normalize=True)
    idx.synchronize()

    def clip(m, stride):
        src = SRC * VIDEO + FIRST + stride * torch.arange(m, device=dev)
        q = rows[src] + torch.randn((m, D), device=dev, generator=g) * (0.1 / D ** 0.5)
        return list((q / q.norm(dim=1, keepdim=True)).cpu().numpy())

    clips = {64: clip(64, 2), 256: clip(256, 1)}
    clips[256] = [f for f in clips[256] for _ in (0, 1)][:256]    # m = 256: every frame twice, half the pace
    del rows, x
    video = lambda nid: nid // VIDEO                              # noqa: E731
    frame = lambda nid: nid % VIDEO                               # noqa: E731
    kw = dict(group_of=video, position_of=frame)
    say(f"# {N} x {D} rows, {videos} videos of {VIDEO} rows, positions = frame numbers, k = 10, {reps} reps")
    t0 = time.perf_counter()
    first = idx.align_clip(clips[64], 10, alignment=True, **kw)
    say(f"first call (labels and positions mapped and uploaded, the (position, tie) order sorted and uploaded): {time.perf_counter() - t0:.2f} s")
    say(f"answer m 64 (every second frame of video {SRC} from frame {FIRST}): video {first[0]['group']} frames {first[0]['start']}..{first[0]['end']}, "
        f"distance {first[0]['distance']:.5f}, next {first[1]['group']} at {first[1]['distance']:.5f}")
    assert first[0]["group"] == SRC and abs(first[0]["start"] - FIRST) <= 2 and abs(first[0]["end"] - (FIRST + 126)) <= 2, first[0]
    slow = idx.align_clip(clips[256], 10, **kw)
    say(f"answer m 256 (frames {FIRST}..{FIRST + 127} twice each): video {slow[0]['group']} frames {slow[0]['start']}..{slow[0]['end']}, "
        f"distance {slow[0]['distance']:.5f}")
    assert slow[0]["group"] == SRC and abs(slow[0]["start"] - FIRST) <= 2 and abs(slow[0]["end"] - (FIRST + 127)) <= 2, slow[0]
    say("call | wall ms | device ms: exact_dist (the floor)  sequence_dp  select | alignment kernels / distance pass | stats")
    calls = [("align_clip m 64", lambda: idx.align_clip(clips[64], 10, **kw)),
             ("align_clip m 64 alignment", lambda: idx.align_clip(clips[64], 10, alignment=True, **kw)),
             ("align_clip m 256", lambda: idx.align_clip(clips[256], 10, **kw)),
             ("align_clip m 256 alignment", lambda: idx.align_clip(clips[256], 10, alignment=True, **kw)),
             ("search_sequence m 64 max_gap 8", lambda: idx.search_sequence(clips[64], 10, max_gap=8, **kw))]
    for name, fn in calls:
        for _ in range(2):
            fn()
        ms = median_ms(fn, reps)
        cls = classes(idx, fn, max(2, reps // 5))
        dp, dist = cls.get("sequence_dp", 0.0), cls.get("exact_dist_f64chain", 0.0)
        say(f"{name:32s} | {ms:8.3f} | {dist:8.4f} {dp:8.4f} {cls.get('select_topk', 0.0):8.4f} | {dp / dist:6.3f} | {idx.last_search_stats()}")
    # the bound: one group holding every row
    one = lambda nid: 0                                           # noqa: E731
    ident = lambda nid: nid                                       # noqa: E731
    fn = lambda: idx.align_clip(clips[64], 10, group_of=one, position_of=ident)  # noqa: E731
    t0 = time.perf_counter()
    res = fn()
    first_ms = (time.perf_counter() - t0) * 1e3
    cls = classes(idx, fn, 1)
    say(f"one group of {N} rows, m 64: {first_ms:9.1f} ms the first call, device ms by class {json.dumps(cls)}   "
        f"(rows {res[0]['start_id']}..{res[0]['end_id']}, stats {idx.last_search_stats()})")
    idx.close()


if __name__ == "__main__":
    main()
