#!/usr/bin/env python3
"""Library neighbours latency on V videos x F frames x 512 video-like unit rows (a video is a random walk,
v[i+1] = normalize(v[i] + 0.2 g / sqrt(dim))), k = 10.  Default 1,000 x 1,000 = 1M rows; --videos / --frames for what the box holds.
Each leg runs in a fresh process that builds the index, warms the call up once and times host-synchronous repetitions
(median, min .. max):
  a      vq_index_neighbors_device, every row, exclude = 1 (other videos only), mode 2
  b      ... exclude = 0 (every row but the row itself), mode 2
  c      vq_index_search_device with the stored rows as queries at k + 1, mode 2: the only other route to (b)'s answer
         (the self row still has to be struck out of every line)
  d      vq_index_search_filtered_device per video (its rows as queries, exclude = {the video}), mode 0, over a sample of 32
         videos, scaled to the library: the only other route to (a)'s answer
  sweep  row lists of m = 64 .. 4,096 asked rows in modes 1 and 2: the crossover mode 0's lower bound on m is set from
Legs a and b also print the call's stats and the tile pass (profile class scan_f16_mfma_top2) as a share of the fp16 MFMA
peak in issued flop: 2 x asked rows padded to 256 x matrix rows padded to 256 x dim over 2,517 TFLOP/s.
usage: neighbors_probe.py OUTDIR [--videos V] [--frames F] [--legs a,b,c,d,sweep] [--limit SECONDS_PER_LEG]   (appends to OUTDIR/probe.txt)"""
import os
import subprocess
import sys
import time
from ctypes import c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, K = 512, 10
MFMA_PEAK = 2.517e15
LIMIT = 600                    # seconds per leg


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, sync, reps):
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return f"median {np.median(ts):.1f} ms, {min(ts):.1f} .. {max(ts):.1f} over {reps}", float(np.median(ts))


def walk(torch, dev, gen, videos, frames):
    rows = torch.empty((videos, frames, D), device=dev)
    x = torch.randn((videos, D), device=dev, generator=gen)
    x /= x.norm(dim=1, keepdim=True)
    for i in range(frames):
        rows[:, i] = x
        x = x + torch.randn((videos, D), device=dev, generator=gen) * (0.2 / D ** 0.5)
        x /= x.norm(dim=1, keepdim=True)
    return rows.reshape(videos * frames, D)


def leg(out, name, videos, frames):
    import torch
    from video_quierer_amd import _lib
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    n = videos * frames
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5000)

    def say(*a):
        line = " ".join(str(x) for x in a)
        print(line, flush=True)
        with open(os.path.join(out, "probe.txt"), "a") as f:
            f.write(line + "\n")

    rows = walk(torch, dev, gen, videos, frames)
    idx = OptimizedHNSWIndex(dimension=D)
    for c0 in range(0, n, 250_000):
        c1 = min(n, c0 + 250_000)
        torch.cuda.synchronize()
        idx.add_device(rows[c0:c1].data_ptr(), c1 - c0, range(c0, c1), normalize=True)
        idx.synchronize()
    video = lambda nid: nid // frames                                     # noqa: E731
    lib = _lib.load()
    with idx.lock:
        labels = idx._sync_groups(video).labels
    sync = idx.synchronize
    reps = 3

    def neighbors(exclude, mode, ask=None, k=K):
        m = n if ask is None else len(ask)
        ids = torch.empty((m, k), dtype=torch.int32, device=dev)
        dist = torch.empty((m, k), dtype=torch.float32, device=dev)
        ptr = None if ask is None else _lib.i64ptr(ask)
        return lambda: _lib.check(lib.vq_index_neighbors_device(idx._h, ptr, m, k, exclude, mode, c_void_p(ids.data_ptr()), c_void_p(dist.data_ptr())))

    if name in ("a", "b"):
        exclude = 1 if name == "a" else 0
        call = neighbors(exclude, 2)
        call(); sync()                                                    # noqa: E702
        st = idx.last_search_stats()
        text, ms = timed(call, sync, reps)
        idx.profile_begin()
        call(); sync()                                                    # noqa: E702
        prof = idx.profile_end()
        tile = prof.get("scan_f16_mfma_top2", {"ms": 0.0})["ms"]
        pad = -(-n // 256) * 256
        say(f"({name}) neighbors_device, every row, exclude = {exclude}, mode 2, n = {n}: {text} | stats {st}")
        say(f"    device classes: " + ", ".join(f"{c} {v['ms']:.1f} ms" for c, v in prof.items() if v["ms"] > 0))
        if tile > 0:
            say(f"    tile pass {tile:.1f} ms: {100 * 2.0 * pad * pad * D / (tile * 1e-3) / MFMA_PEAK:.1f} % of the fp16 MFMA peak in issued flop")
    elif name == "c":
        ids = torch.empty((n, K + 1), dtype=torch.int32, device=dev)
        dist = torch.empty((n, K + 1), dtype=torch.float32, device=dev)
        call = lambda: idx.search_device(rows.data_ptr(), n, K + 1, ids.data_ptr(), dist.data_ptr(), mode=2)     # noqa: E731
        call(); sync()                                                    # noqa: E702
        st = idx.last_search_stats()
        text, ms = timed(call, sync, reps)
        say(f"(c) search_device, the stored rows as queries, k + 1 = {K + 1}, mode 2, n = {n}: {text} | stats {st} (the self row not yet struck)")
    elif name == "d":
        sample = np.random.default_rng(1).choice(videos, min(32, videos), replace=False)
        ids = torch.empty((frames, K), dtype=torch.int32, device=dev)
        dist = torch.empty((frames, K), dtype=torch.float32, device=dev)

        def call():
            for v in sample.tolist():
                sel = np.array([labels[v * frames]], dtype=np.int32)
                _lib.check(lib.vq_index_search_filtered_device(idx._h, c_void_p(rows[v * frames:(v + 1) * frames].data_ptr()), frames, K, 0,
                                                               _lib.i32ptr(sel), 1, 1, c_void_p(ids.data_ptr()), c_void_p(dist.data_ptr())))
        call(); sync()                                                    # noqa: E702
        text, ms = timed(call, sync, reps)
        say(f"(d) search_filtered_device per video, exclude = its own video, mode 0, {len(sample)} of {videos} videos: {text} | "
            f"scaled to the library: {ms * videos / len(sample) / 1e3:.1f} s")
    elif name == "sweep":
        say(f"# sweep: row lists of m asked rows, exclude = 1, n = {n}: mode 1 | mode 2")
        for m in (64, 256, 1024, 4096):
            ask = np.random.default_rng(m).choice(n, m, replace=False).astype(np.int64)
            cells = []
            for mode in (1, 2):
                call = neighbors(1, mode, ask)
                call(); sync()                                            # noqa: E702
                cells.append(timed(call, sync, reps)[0])
            say(f"m = {m}: {cells[0]} | {cells[1]}")
    idx.close()


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    videos, frames = arg("--videos", 1000), arg("--frames", 1000)
    if "--leg" in sys.argv:
        return leg(out, sys.argv[sys.argv.index("--leg") + 1], videos, frames)
    legs = sys.argv[sys.argv.index("--legs") + 1].split(",") if "--legs" in sys.argv else ["a", "b", "c", "d", "sweep"]
    with open(os.path.join(out, "probe.txt"), "a") as f:
        f.write(f"# {videos} videos x {frames} frames x {D}, k = {K}; every leg in a fresh process\n")
    for name in legs:
        cmd = ["timeout", "-k", "10", str(arg("--limit", LIMIT)), sys.executable, os.path.abspath(__file__), out, "--leg", name, "--videos", str(videos),
               "--frames", str(frames)]
        rc = subprocess.call(cmd)
        if rc != 0:
            with open(os.path.join(out, "probe.txt"), "a") as f:
                f.write(f"leg {name} ended with status {rc}: the probe stops here\n")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
