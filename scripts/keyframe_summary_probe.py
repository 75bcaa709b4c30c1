#!/usr/bin/env python3
"""Keyframe summary latency on video-like unit rows (a video is a random walk, v[i+1] = normalize(v[i] + 0.2 g / sqrt(dim))).
  library    summarize_groups() over 1,000 videos x 1,000 frames x 512 at k = 8: every video in one call (LDS form), then the
             only route without the call: _export() once plus the selection in numpy on the host, video by video
  video3600  one 3,600-frame video (the sampler's cap) at k = 8 and k = 64 (LDS form, one workgroup)
  video100k  one 100,000-frame video at k = 8 (wide form: 391 blocks of 256 rows, 2 k + 5 launches)
Next to each timing: the bytes the definition must read, k x L x dim x 4 summed over the videos (every step reads every row of
the video once; the mean's pass is not counted), and the rate they give as a fraction of the 8 TB/s HBM peak.  Wall times are
medians of host-synchronous calls after warm-up; device ms from the index's event brackets (class exact_dist_f64chain; a call's
kernels sit in ONE bracket, which is what the "launches" beside it counts).
Each step runs in a child process of its own under a time limit; a step that fails or runs out of time ends the probe.
usage: keyframe_summary_probe.py OUTDIR [--quick]   (writes OUTDIR/probe.txt)"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 512
HBM_PEAK = 8.0e12
STEPS = (("library", 420), ("video3600", 120), ("video100k", 180))     # name, seconds


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def device_ms(idx, fn, reps):
    idx.profile_begin()
    for _ in range(reps):
        fn()
    cls = idx.profile_end()["exact_dist_f64chain"]
    return cls["ms"] / reps, cls["launches"] // reps


def rate(bytes_read, ms):
    tbs = bytes_read / (ms * 1e-3) / 1e12
    return f"{bytes_read / 1e9:.3f} GB the definition reads -> {tbs:.2f} TB/s = {100 * tbs * 1e12 / HBM_PEAK:.1f} % of the HBM peak"


def host_summary(x, k):
    """The selection in numpy on one video's rows (matmul distances: the fixed-order chain's bits are not reproduced; ties to the
    smaller row).  -> keyframe indices"""
    c = x.astype(np.float64).sum(axis=0).astype(np.float32)
    s = int(np.argmin(np.float32(1.0) - x @ c))
    near = np.float32(1.0) - x @ x[s]
    near[s] = -np.inf
    chosen = [s]
    while len(chosen) < min(k, len(x)):
        s = int(np.argmax(near))
        chosen.append(s)
        near = np.minimum(near, np.float32(1.0) - x @ x[s])
        near[chosen] = -np.inf
    return chosen


def walk(torch, dev, gen, videos, frames):
    """[videos * frames][D] unit rows on the device, video after video."""
    rows = torch.empty((videos, frames, D), device=dev)
    x = torch.randn((videos, D), device=dev, generator=gen)
    x /= x.norm(dim=1, keepdim=True)
    for i in range(frames):
        rows[:, i] = x
        x = x + torch.randn((videos, D), device=dev, generator=gen) * (0.2 / D ** 0.5)
        x /= x.norm(dim=1, keepdim=True)
    return rows.reshape(videos * frames, D)


def drift(torch, dev, gen, frames):
    """One long video without a launch per frame: the normalised running sum of the same steps."""
    x = torch.randn((1, D), device=dev, generator=gen)
    x = x / x.norm() + torch.cumsum(torch.randn((frames, D), device=dev, generator=gen) * (0.2 / D ** 0.5), dim=0)
    return x / x.norm(dim=1, keepdim=True)


def build(torch, rows, per_video):
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    idx = OptimizedHNSWIndex(dimension=D)
    n = rows.shape[0]
    for c0 in range(0, n, 250_000):
        c1 = min(n, c0 + 250_000)
        torch.cuda.synchronize()
        idx.add_device(rows[c0:c1].data_ptr(), c1 - c0, range(c0, c1), normalize=True)
        idx.synchronize()
    return idx, (lambda nid: nid // per_video)


def step(name, out, quick):
    import torch
    reps = 3 if quick else 15
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(4000)
    lines = []

    def say(*a):
        line = " ".join(str(x) for x in a)
        print(line, flush=True)
        lines.append(line)
        with open(os.path.join(out, f"probe_{name}.txt"), "w") as f:      # kept current: a later part may take long
            f.write("\n".join(lines) + "\n")

    if name == "library":
        videos, frames, k = 1_000, 1_000, 8
        idx, video = build(torch, walk(torch, dev, gen, videos, frames), frames)
        t0 = time.perf_counter()
        res = idx.summarize_groups(k=k, group_of=video)
        say(f"# {videos} videos x {frames} frames x {D}, k = {k}, {reps} reps")
        say(f"first call (labels mapped and uploaded): {time.perf_counter() - t0:.2f} s")
        call = lambda: idx.summarize_groups(k=k, group_of=video)          # noqa: E731
        ms = median_ms(call, reps)
        dms, launches = device_ms(idx, call, max(2, reps // 3))
        say(f"summarize_groups(every video): {ms:.3f} ms per call (host in, dict out), device {dms:.3f} ms in {launches} launches, stats {idx.last_search_stats()}")
        say(f"  {rate(k * videos * frames * D * 4, dms)} (device time)")
        t0 = time.perf_counter()
        stored = idx._export()
        t_export = time.perf_counter() - t0
        t0 = time.perf_counter()
        host = [host_summary(stored[v * frames:(v + 1) * frames], k) for v in range(videos)]
        t_host = time.perf_counter() - t0
        same = sum([r["id"] - v * frames for r in res[v]] == host[v] for v in range(videos))
        say(f"host route: _export() {t_export:.2f} s once, numpy selection over every video {t_host * 1e3:.0f} ms "
            f"({t_host * 1e3 / ms:.1f} x the call; {same} of {videos} videos pick the same keyframes as the exact call)")
    elif name == "video3600":
        frames = 3_600
        idx, video = build(torch, drift(torch, dev, gen, frames), frames)
        say(f"# one video of {frames} frames x {D}, {reps} reps")
        for k in (8, 64):
            call = lambda: idx.summarize_group(0, k, group_of=video)      # noqa: E731
            call()
            ms = median_ms(call, reps)
            dms, launches = device_ms(idx, call, max(2, reps // 3))
            say(f"k = {k}: {ms:.3f} ms per call, device {dms:.3f} ms in {launches} launches, stats {idx.last_search_stats()}")
            say(f"  {rate(k * frames * D * 4, dms)} (device time; one workgroup on one CU)")
        stored = idx._export()
        t0 = time.perf_counter()
        host = host_summary(stored, 64)
        t_host = (time.perf_counter() - t0) * 1e3
        got = [r["id"] for r in idx.summarize_group(0, 64, group_of=video)]
        agree = next((i for i, (a, b) in enumerate(zip(got, host)) if a != b), 64)
        say(f"host route, k = 64: numpy selection {t_host:.1f} ms after _export(); its first {agree} keyframes are the call's")
    else:
        frames, k = 100_000, 8
        idx, video = build(torch, drift(torch, dev, gen, frames), frames)
        say(f"# one video of {frames} frames x {D}, k = {k} (wide form), {reps} reps")
        call = lambda: idx.summarize_group(0, k, group_of=video)          # noqa: E731
        call()
        ms = median_ms(call, reps)
        dms, launches = device_ms(idx, call, max(2, reps // 3))
        say(f"k = {k}: {ms:.3f} ms per call, device {dms:.3f} ms in {launches} launches, stats {idx.last_search_stats()}")
        say(f"  {rate(k * frames * D * 4, dms)} (device time)")
        stored = idx._export()
        t0 = time.perf_counter()
        host = host_summary(stored, k)
        t_host = (time.perf_counter() - t0) * 1e3
        got = [r["id"] for r in idx.summarize_group(0, k, group_of=video)]
        say(f"host route: numpy selection {t_host:.1f} ms after _export(); same keyframes as the call: {got == host}")
    idx.close()


def main():
    out = sys.argv[1]
    quick = "--quick" in sys.argv
    os.makedirs(out, exist_ok=True)
    if "--step" in sys.argv:
        return step(sys.argv[sys.argv.index("--step") + 1], out, quick)
    text = []
    for name, limit in STEPS:                                             # each GPU step: its own process, its own time limit
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), out, "--step", name] + (["--quick"] if quick else [])
        rc = subprocess.call(cmd)
        part = os.path.join(out, f"probe_{name}.txt")
        if os.path.exists(part):
            with open(part) as f:
                text.append(f.read())
            os.remove(part)
        if rc != 0:
            text.append(f"step {name} ended with status {rc}: the probe stops here\n")
        with open(os.path.join(out, "probe.txt"), "w") as f:
            f.write("\n".join(text))
        if rc != 0:
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
