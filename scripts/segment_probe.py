#!/usr/bin/env python3
"""Chapter segmentation latency on video-like unit rows (a video is a random walk, v[i+1] = normalize(v[i] + 0.2 g / sqrt(dim))).
  library    segment_groups() over 2,000 videos x 500 frames x 512 at k = 8: every video in one call (8 batches of 261 videos)
  video4096  one 4,096-frame video at k = 8 (one batch, the DP in LDS on one CU)
Per shape: the wall time of the call, its device time (the index's event bracket, class exact_dist_f64chain), then the four
stages apart — prefix, pair cost, DP, show — from a second run of the same call under `rocprofv3 --kernel-trace --stats` (each
kernel's total time over the run divided by the calls made), and beside them a torch fp64 restatement of the pair costs on the
same device: differences of a cumsum, rounded to fp32, then norms (timed over a few videos and scaled for the library shape; it
does not reproduce the chain's bits).  The pair stage is also given as column steps per second: pairs x dim / time.
Wall times are medians of host-synchronous calls after warm-up.  These times are recorded, not gated.
Each step runs in a child process of its own under a time limit; a step that fails or runs out of time ends the probe.
usage: segment_probe.py OUTDIR [--quick]   (writes OUTDIR/probe.txt)"""
import csv
import glob
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, K = 512, 8
SHAPES = {"library": (2_000, 500), "video4096": (1, 4_096)}
STEPS = (("library", 420), ("video4096", 180))                            # name, seconds (each of the two runs)
STAGES = (("prefix", "seg_prefix_kernel"), ("pair", "seg_pair_kernel"), ("dp", "seg_dp_kernel"), ("show", "seg_show_kernel"))


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def walk(torch, dev, gen, videos, frames):
    """[videos * frames][D] unit rows on the device, video after video: the normalised running sum of the steps."""
    x = torch.randn((videos, 1, D), device=dev, generator=gen)
    x = x / x.norm(dim=2, keepdim=True) + torch.cumsum(torch.randn((videos, frames, D), device=dev, generator=gen) * (0.2 / D ** 0.5), dim=1)
    return (x / x.norm(dim=2, keepdim=True)).reshape(videos * frames, D)


def build(torch, rows, frames):
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    idx = OptimizedHNSWIndex(dimension=D)
    n = rows.shape[0]
    for c0 in range(0, n, 250_000):
        c1 = min(n, c0 + 250_000)
        torch.cuda.synchronize()
        idx.add_device(rows[c0:c1].data_ptr(), c1 - c0, range(c0, c1), normalize=True)
        idx.synchronize()
    return idx, (lambda nid: nid // frames), (lambda nid: nid % frames)


def torch_pair_costs(torch, rows, frames, videos):
    """cost(a, b) for every a < b of `videos` videos: P = cumsum in fp64, u = fp32(P_b - P_a), cost = (b - a) - |u| in fp64.
    One video at a time, 128 values of b per block (a [128][frames][D] fp64 block is 268 MB at 500 frames)."""
    cost = None
    span = torch.arange(frames + 1, device=rows.device, dtype=torch.float64)
    for v in range(videos):
        x = rows[v * frames:(v + 1) * frames].double()
        P = torch.cat([torch.zeros((1, D), device=rows.device, dtype=torch.float64), torch.cumsum(x, dim=0)])
        for b0 in range(1, frames + 1, 128):                              # (the full square: a >= b is computed and not used)
            b1 = min(frames + 1, b0 + 128)
            u = (P[b0:b1, None, :] - P[None, :frames, :]).float().double()
            cost = (span[b0:b1, None] - span[None, :frames]) - u.square().sum(dim=2).sqrt()
    torch.cuda.synchronize()
    return cost


def step(name, out, quick, traced):
    import torch
    videos, frames = SHAPES[name]
    reps = 2 if traced else (3 if quick else 9)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5000)
    lines = []

    def say(*a):
        line = " ".join(str(x) for x in a)
        print(line, flush=True)
        lines.append(line)
        with open(os.path.join(out, f"probe_{name}.txt"), "w") as f:      # kept current: a later part may take long
            f.write("\n".join(lines) + "\n")

    rows = walk(torch, dev, gen, videos, frames)
    idx, video, frame = build(torch, rows, frames)
    call = lambda: idx.segment_groups(k=K, group_of=video, position_of=frame)          # noqa: E731
    t0 = time.perf_counter()
    res = call()
    first = time.perf_counter() - t0
    if traced:                                                            # the profiler's run: the calls only
        for _ in range(reps):
            call()
        with open(os.path.join(out, f"calls_{name}.txt"), "w") as f:
            f.write(str(reps + 1))
        idx.close()
        return
    pairs = videos * (frames * (frames + 1) // 2)
    say(f"# {videos} video(s) x {frames} frames x {D}, k = {K}, penalty 0, {reps} reps; {pairs} pairs, {pairs * D:.3e} column steps")
    say(f"first call (labels, positions and the (position, tie) order mapped and uploaded): {first:.2f} s")
    ms = median_ms(call, reps)
    idx.profile_begin()
    for _ in range(max(2, reps // 3)):
        call()
    cls = idx.profile_end()["exact_dist_f64chain"]
    n = max(2, reps // 3)
    say(f"segment_groups: {ms:.3f} ms per call (dict out), device {cls['ms'] / n:.3f} ms in {cls['launches'] // n} launches, stats {idx.last_search_stats()}")
    say(f"  chapters per video: {np.bincount([len(v) for v in res.values()], minlength=K + 1).tolist()} (index = chapters)")
    some = min(videos, 4 if quick else 16)
    torch_pair_costs(torch, rows, frames, 1)
    t0 = time.perf_counter()
    torch_pair_costs(torch, rows, frames, some)
    t_torch = (time.perf_counter() - t0) * 1e3 * videos / some
    say(f"torch fp64 pair costs (cumsum, differences, norms over the full frames x frames square, twice the pairs; {some} video(s) timed, "
        f"scaled to {videos}): {t_torch:.1f} ms")
    idx.close()


def stage_times(prof_dir, calls):
    """{stage: ms per call} from rocprofv3's kernel statistics."""
    got = {}
    for path in glob.glob(os.path.join(prof_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                for stage, kernel in STAGES:
                    if kernel in row["Name"]:
                        got[stage] = got.get(stage, 0.0) + float(row["TotalDurationNs"]) / 1e6 / calls
    return got


def main():
    out = sys.argv[1]
    quick = "--quick" in sys.argv
    os.makedirs(out, exist_ok=True)
    if "--step" in sys.argv:
        return step(sys.argv[sys.argv.index("--step") + 1], out, quick, "--traced" in sys.argv)
    text = []
    for name, limit in STEPS:                                             # each GPU run: its own process, its own time limit
        me = [sys.executable, os.path.abspath(__file__), out, "--step", name] + (["--quick"] if quick else [])
        prof = os.path.join(out, f"prof_{name}")
        runs = (["timeout", "-k", "10", str(limit)] + me,
                ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "p", "--"] + me + ["--traced"])
        rc = 0
        for cmd in runs:
            rc = subprocess.call(cmd)
            if rc != 0:
                break
        part = os.path.join(out, f"probe_{name}.txt")
        if os.path.exists(part):
            with open(part) as f:
                text.append(f.read())
            os.remove(part)
        calls_file = os.path.join(out, f"calls_{name}.txt")
        if rc == 0 and os.path.exists(calls_file):
            with open(calls_file) as f:
                calls = int(f.read())
            os.remove(calls_file)
            st = stage_times(prof, calls)
            videos, frames = SHAPES[name]
            steps = videos * (frames * (frames + 1) // 2) * D
            text.append("stages, device ms per call (rocprofv3 kernel statistics): " + " | ".join(f"{s} {st.get(s, float('nan')):.3f}" for s, _ in STAGES)
                        + (f"\n  pair stage: {steps / (st['pair'] * 1e-3):.3e} column steps/s" if st.get("pair") else "") + "\n")
        shutil.rmtree(prof, ignore_errors=True)
        if rc != 0:
            text.append(f"step {name} ended with status {rc}: the probe stops here\n")
        with open(os.path.join(out, "probe.txt"), "w") as f:
            f.write("\n".join(text))
        if rc != 0:
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
