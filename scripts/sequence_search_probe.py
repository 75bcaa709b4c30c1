#!/usr/bin/env python3
"""Sequence search latency over 1M x 512 video-like unit rows: 2,000 "videos" of 500 rows, each a random walk
(v[i+1] = normalize(v[i] + 0.2 g / sqrt(dim))), positions = the frame number; steps = m frames of one video at a stride of 3
plus noise of norm 0.3.
  search_sequence(steps, 10, max_gap)   m = 2 .. 64, max_gap 8, 50 and 2^40 (host in, list of dicts out), with the device time by
                                        kernel class from the index's event brackets: sequence_dp is the DP (and the chains'
                                        trace), exact_dist_f64chain the distance pass in front of it
  (a) search_set(steps, 10), mode 1     the same distances with a simpler reduction: the DP's own cost is the difference
  (b) the host route                    _export() once, numpy distances (1 - rows @ q) and the DP in numpy over all videos at
                                        once — the only route without the call; its answer is compared with the call's on the C
                                        oracle's distances (numpy's matmul does not reproduce the fixed-order chain's bits)
  one group of 1M rows                  the global form's bound: one workgroup walks the whole index
Wall times are medians of host-synchronous calls after warm-up.
usage: sequence_search_probe.py OUTDIR [--quick]   (writes OUTDIR/probe.txt)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_quierer_amd.indexes.hnsw import MODE_EXACT, OptimizedHNSWIndex  # noqa: E402

N, D, VIDEO = 1_000_000, 512, 500
BIG = 2 ** 40


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


def host_dp(dist, max_gap, k):
    """The definition over videos of VIDEO consecutive rows at positions 0 .. VIDEO-1 (ties = row numbers), all videos at
    once.  dist [m][N] float32 -> [(video, D, chain rows)] for the k best."""
    m = len(dist)
    videos = dist[0].shape[0] // VIDEO
    C = dist[0].astype(np.float64).reshape(videos, VIDEO)
    back = []
    span = min(max_gap, VIDEO - 1)
    for j in range(1, m):
        best = np.full((videos, VIDEO), np.inf)
        arg = np.full((videos, VIDEO), -1, dtype=np.int32)
        for delta in range(span, 0, -1):                           # the farthest predecessor first: the smaller row wins a tie
            cand = C[:, :VIDEO - delta]
            better = cand < best[:, delta:]
            best[:, delta:] = np.where(better, cand, best[:, delta:])
            arg[:, delta:] = np.where(better, np.arange(VIDEO - delta, dtype=np.int32)[None, :], arg[:, delta:])
        C = best + dist[j].astype(np.float64).reshape(videos, VIDEO)
        back.append(arg)
    end = C.argmin(axis=1)                                         # (the first of equal costs: the smaller row)
    Dg = (C[np.arange(videos), end] / m).astype(np.float32)
    order = np.lexsort((np.arange(videos), Dg))[:k]
    out = []
    for v in order.tolist():
        if not np.isfinite(Dg[v]):
            break
        chain = [int(end[v])]
        for arg in reversed(back):
            chain.append(int(arg[v, chain[-1]]))
        out.append((v, Dg[v], [v * VIDEO + i for i in reversed(chain)]))
    return out


def main():
    out = sys.argv[1]
    quick = "--quick" in sys.argv
    reps = 5 if quick else 30
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
    g.manual_seed(3000)
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
    for c0 in range(0, N, 250_000):
        torch.cuda.synchronize()
        idx.add_device(rows[c0:c0 + 250_000].data_ptr(), 250_000, range(c0, c0 + 250_000), normalize=True)
        idx.synchronize()
    src = 777 * VIDEO + 40 + 3 * torch.arange(64, device=dev)
    steps_all = rows[src] + torch.randn((64, D), device=dev, generator=g) * (0.3 / D ** 0.5)
    steps_all = (steps_all / steps_all.norm(dim=1, keepdim=True)).cpu().numpy()
    del rows, x
    video = lambda nid: nid // VIDEO                              # noqa: E731
    frame = lambda nid: nid % VIDEO                               # noqa: E731
    idx.search_mode = MODE_EXACT
    say(f"# {N} x {D} rows, {videos} videos of {VIDEO} rows, positions = frame numbers, k = 10, {reps} reps")
    t0 = time.perf_counter()
    idx.search_sequence(list(steps_all[:2]), 10, max_gap=8, group_of=video, position_of=frame)
    say(f"first call (labels and positions mapped and uploaded, the (position, tie) order sorted and uploaded): {time.perf_counter() - t0:.2f} s")
    say("m  max_gap | search_sequence ms | search_set mode 1 ms | device ms: exact_dist  sequence_dp  select | DP ns per (step, row) | DP share of device time")
    for m in (2, 4, 8, 16, 32, 64):
        steps = list(steps_all[:m])
        sset = lambda: idx.search_set(steps, 10, group_of=video)  # noqa: E731
        sset()
        set_ms = median_ms(sset, reps)
        set_cls = classes(idx, sset, max(3, reps // 5))
        for max_gap in (8, 50, BIG):
            seq = lambda: idx.search_sequence(steps, 10, max_gap=max_gap, group_of=video, position_of=frame)  # noqa: E731
            for _ in range(3):
                res = seq()
            assert res[0]["group"] == 777, res[0]
            ms = median_ms(seq, reps)
            cls = classes(idx, seq, max(3, reps // 5))
            dp, dist = cls.get("sequence_dp", 0.0), cls.get("exact_dist_f64chain", 0.0)
            total = sum(cls.values())
            say(f"{m:2d} {('2^40' if max_gap == BIG else max_gap):>7} | {ms:9.3f} | {set_ms:9.3f} | {dist:8.4f} {dp:8.4f} {cls.get('select_topk', 0.0):8.4f} | "
                f"{dp * 1e6 / (max(1, m - 1) * N):7.3f} | {100 * dp / total:5.1f} %   stats {idx.last_search_stats()}")
        say(f"{m:2d} search_set device ms by class: {json.dumps(set_cls)}")
    # (b) the host route at the full size, m = 8
    from oracle import knn_oracle
    m = 8
    steps = np.ascontiguousarray(idx._unit_rows(steps_all[:m]), dtype=np.float32)      # as search_sequence normalises them
    t0 = time.perf_counter()
    stored = idx._export()
    t_export = time.perf_counter() - t0
    t0 = time.perf_counter()
    dist_np = [(np.float32(1.0) - stored @ q).astype(np.float32) for q in steps]
    t_dist = time.perf_counter() - t0
    dist_or = [knn_oracle.distances(stored, q) for q in steps]
    say(f"host route, m = {m}: _export() {t_export:.2f} s once; numpy distances {t_dist * 1e3:.0f} ms; "
        f"largest |numpy - fixed-order chain| distance {max(float(np.abs(a - b).max()) for a, b in zip(dist_np, dist_or)):.2e}")
    for max_gap in (8, 50):
        t0 = time.perf_counter()
        host_dp(dist_np, max_gap, 10)
        t_dp = time.perf_counter() - t0
        want = host_dp(dist_or, max_gap, 10)
        got = idx.search_sequence(list(steps), 10, max_gap=max_gap, group_of=video, position_of=frame)
        same = ([r["group"] for r in got] == [w[0] for w in want] and [r["chain"] for r in got] == [w[2] for w in want]
                and np.array_equal(np.array([r["distance"] for r in got], np.float32).view(np.uint32), np.array([w[1] for w in want], np.float32).view(np.uint32)))
        assert same, (got, want)
        say(f"  max_gap {max_gap}: numpy DP over all videos {t_dp * 1e3:.0f} ms (+ the distances: {(t_dist + t_dp) * 1e3:.0f} ms per query); "
            f"on the oracle's distances its groups, distances and chains are identical to the call's: {same}")
    del stored, dist_np, dist_or
    # the bound: one group holding every row
    one = lambda nid: 0                                           # noqa: E731
    ident = lambda nid: nid                                       # noqa: E731
    for m, max_gap in ((2, 8), (8, 8), (8, 50), (2, BIG), (4, BIG)):
        t0 = time.perf_counter()
        res = idx.search_sequence(list(steps_all[:m]), 10, max_gap=max_gap, group_of=one, position_of=ident)
        first = (time.perf_counter() - t0) * 1e3
        cls = classes(idx, lambda: idx.search_sequence(list(steps_all[:m]), 10, max_gap=max_gap, group_of=one, position_of=ident), 1)
        say(f"one group of {N} rows, m = {m}, max_gap {'2^40' if max_gap == BIG else max_gap}: {first:9.1f} ms the first call, device ms by class {json.dumps(cls)}   "
            f"({len(res)} result, stats {idx.last_search_stats()})")
    idx.close()


if __name__ == "__main__":
    main()
