#!/usr/bin/env python3
"""Shared-footage search latency over 1M x 512 video-like unit rows: 2,000 "videos" of 500 rows, each a random walk
(v[i+1] = normalize(v[i] + 0.2 g / sqrt(dim))), positions = the frame number.  The clip is video 777 plus noise of norm 0.1
per frame (about 0.005 away from its source frame), continued by random directions where it is longer than the video.
  shared_runs(clip, 10, max_distance)   m = 64, 500, 4,096; modes 2 (tile path) and 1 (exact path): wall medians, and the device
                                        time by kernel class from the index's event brackets (scan_f16_mfma_top2 = match_tile_kernel,
                                        sequence_dp = match_run_kernel, exact_dist_f64chain = the exact distances, the redo and
                                        match_score_kernel, rescore_verify = the norms and match_patch_kernel, select_topk = the rest)
  (a) search_set(clip, 10), mode 2      the same mainloop over the same bytes: scan_f16_mfma_top2 there is set_group_max_kernel
  (b) shared_runs, mode 1               what mode 0's crossover (MATCH_AUTO_MIN_M, csrc/knn_match.h) is read from
  (c) the host route                    _export() once, numpy scores, the runs in numpy over all videos at once: the only route the
                                        library offered before; its answer is compared with the call's on the C oracle's distances
  pairs filed at max_distance 0.05 / 0.1 / 0.2
Wall times are medians of host-synchronous calls after warm-up.
usage: match_probe.py OUTDIR [--quick]   (writes OUTDIR/probe.txt)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_quierer_amd.indexes.hnsw import MODE_EXACT, MODE_FP16, OptimizedHNSWIndex  # noqa: E402

N, D, VIDEO = 1_000_000, 512, 500
SOURCE = 777


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


def host_runs(hit, min_len, k):
    """The definition with max_miss = 0 over videos of VIDEO consecutive rows in frame order, all videos at once.  hit [m][N] bool
    -> [(video, hits, q_first, row_first, row_last)] for the k best by (-hits, span, video); span = hits without misses."""
    m = hit.shape[0]
    videos = hit.shape[1] // VIDEO
    H = hit.reshape(m, videos, VIDEO)
    run = np.zeros((videos, VIDEO), dtype=np.int32)               # the run of hits that ends at cell (i, j), along the diagonal
    best = np.zeros(videos, dtype=np.int64)                       # per video: the best (hits, -delta, -s) packed into one integer
    for i in range(m):
        prev = np.zeros_like(run)
        prev[:, 1:] = run[:, :-1]
        run = np.where(H[i], prev + 1, 0)
        j = np.arange(VIDEO)[None, :]
        delta = j - i + (m - 1)                                   # >= 0
        s = i - run + 1
        key = (run.astype(np.int64) << 40) | ((2 * (m + VIDEO) - delta).astype(np.int64) << 16) | (m - s).astype(np.int64)
        key = np.where(run >= min_len, key, 0)
        best = np.maximum(best, key.max(axis=1))
    out = []
    for v in np.lexsort((np.arange(videos), -(best >> 40)))[:k].tolist():
        if best[v] == 0:
            break
        hits = int(best[v] >> 40)
        delta = 2 * (m + VIDEO) - int((best[v] >> 16) & 0xFFFFFF) - (m - 1)
        s = m - int(best[v] & 0xFFFF)
        out.append((v, hits, s, v * VIDEO + s + delta, v * VIDEO + s + hits - 1 + delta))
    return out


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
    clip_all = torch.randn((4096, D), device=dev, generator=g)
    clip_all[:VIDEO] = rows[SOURCE * VIDEO:(SOURCE + 1) * VIDEO] + torch.randn((VIDEO, D), device=dev, generator=g) * (0.1 / D ** 0.5)
    clip_all = (clip_all / clip_all.norm(dim=1, keepdim=True)).cpu().numpy()
    del rows, x
    video = lambda nid: nid // VIDEO                              # noqa: E731
    frame = lambda nid: nid % VIDEO                               # noqa: E731
    say(f"# {N} x {D} rows, {videos} videos of {VIDEO} rows, positions = frame numbers, k = 10, min_len 3, max_miss 1, {reps} reps")
    idx.search_mode = MODE_EXACT
    t0 = time.perf_counter()
    idx.shared_runs(list(clip_all[:2]), 10, max_distance=0.05, min_len=1, group_of=video, position_of=frame)
    say(f"first call (labels and positions mapped and uploaded, the (position, tie) order sorted and uploaded): {time.perf_counter() - t0:.2f} s")
    say("m  max_distance mode | shared_runs ms | device ms by class | stats")
    tile_ms, set_ms = {}, {}
    for m in (64, 500, 4096):
        clip = list(clip_all[:m])
        for max_distance in ((0.05, 0.1, 0.2) if m == 500 else (0.05,)):
            for mode in (MODE_FP16, MODE_EXACT):
                if mode == MODE_EXACT and max_distance != 0.05:
                    continue
                idx.search_mode = mode
                run = lambda: idx.shared_runs(clip, 10, max_distance=max_distance, min_len=3, max_miss=1, group_of=video, position_of=frame)  # noqa: E731
                for _ in range(2):
                    res = run()
                assert res[0]["group"] == SOURCE and res[0]["hits"] >= min(m, VIDEO) - 2, res[:2]
                ms = median_ms(run, reps if m < 4096 else max(3, reps // 3))
                cls = classes(idx, run, 3)
                if mode == MODE_FP16 and max_distance == 0.05:
                    tile_ms[m] = cls.get("scan_f16_mfma_top2", 0.0)
                say(f"{m:4d} {max_distance:5.2f} mode {mode} | {ms:10.3f} | {json.dumps(cls)} | {idx.last_search_stats()}   best: {res[0]['hits']} hits of video {res[0]['group']}")
        idx.search_mode = MODE_FP16
        sset = lambda: idx.search_set(clip, 10, group_of=video)  # noqa: E731
        sset()
        ms = median_ms(sset, reps if m < 4096 else max(3, reps // 3))
        cls = classes(idx, sset, 3)
        set_ms[m] = cls.get("scan_f16_mfma_top2", 0.0)
        say(f"{m:4d} (a) search_set mode 2 | {ms:10.3f} | {json.dumps(cls)}")
        if set_ms[m] > 0:
            say(f"{m:4d} match_tile_kernel / set_group_max_kernel device time: {tile_ms[m]:.4f} / {set_ms[m]:.4f} = {tile_ms[m] / set_ms[m]:.3f}")
    # (c) the host route, m = 16, max_miss = 0
    from oracle import knn_oracle
    m, max_distance = 16, np.float32(0.05)
    clip = np.ascontiguousarray(idx._unit_rows(clip_all[:m]), dtype=np.float32)          # as shared_runs normalises them
    t0 = time.perf_counter()
    stored = idx._export()
    t_export = time.perf_counter() - t0
    t0 = time.perf_counter()
    hit_np = (np.float32(1.0) - clip @ stored.T).astype(np.float32) <= max_distance
    t_hit = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_runs(hit_np, 3, 10)
    t_runs = time.perf_counter() - t0
    hit_or = np.stack([knn_oracle.distances(stored, q) for q in clip]) <= max_distance
    want = host_runs(hit_or, 3, 10)
    idx.search_mode = MODE_FP16
    got = idx.shared_runs(list(clip), 10, max_distance=float(max_distance), min_len=3, max_miss=0, group_of=video, position_of=frame)
    same = [(r["group"], r["hits"], r["query_first"], r["first"], r["last"]) for r in got] == want
    assert same, (got, want)
    say(f"(c) host route, m = {m}: _export() {t_export:.2f} s once; numpy scores and hits {t_hit * 1e3:.0f} ms; numpy runs over all videos "
        f"{t_runs * 1e3:.0f} ms; on the oracle's distances its videos, hits and rows are identical to the call's: {same}")
    idx.close()


if __name__ == "__main__":
    main()
