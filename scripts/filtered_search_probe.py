#!/usr/bin/env python3
"""Filtered-search latency over 1M x 512 unit rows in 2,000 contiguous "videos" of 500 rows:
  search_filtered(q, 10, within=[one video])      "where in this video"
  search_filtered(q, 10, exclude=[one video])     "more like this from other videos"
  search_grouped(q, 10, exclude=[one video])      the grouped form of the same
  within 10 % / 60 % of the videos, nq = 1 and 32; exclude one video at nq = 256
against the unfiltered search(q, 10), search(q, 20) and search_grouped(q, 10).  Wall times are medians of host-synchronous
calls after warm-up; per-kernel-class device times come from the index's event brackets (profile_begin / profile_end; the
filter setup kernels are not bracketed).
usage: filtered_search_probe.py OUTDIR [--quick]   (writes OUTDIR/filtered_probe.json)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex  # noqa: E402

N, D, VIDEO = 1_000_000, 512, 500


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 4)


def classes(idx, fn, reps):
    idx.profile_begin()
    for _ in range(reps):
        fn()
    return {k: round(v["ms"] / reps, 4) for k, v in idx.profile_end().items() if v["launches"]}


def main():
    out = sys.argv[1]
    quick = "--quick" in sys.argv
    reps = 5 if quick else 30
    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(2000)
    idx = OptimizedHNSWIndex(dimension=D)
    for c0 in range(0, N, 250_000):
        blk = torch.randn((250_000, D), device=dev, generator=g)
        torch.cuda.synchronize()
        idx.add_device(blk.data_ptr(), 250_000, range(c0, c0 + 250_000), normalize=True)
        idx.synchronize()
    qs = torch.randn((256, D), device=dev, generator=g)
    qs = (qs / qs.norm(dim=1, keepdim=True)).cpu().numpy()
    video = lambda nid: nid // VIDEO                                      # noqa: E731
    videos = N // VIDEO
    rng = np.random.default_rng(7)
    one = [videos // 2]
    pct10 = rng.choice(videos, videos // 10, replace=False).tolist()
    pct60 = rng.choice(videos, videos * 6 // 10, replace=False).tolist()
    q0 = qs[0]
    res = {"rows": N, "dim": D, "videos": videos, "rows_per_video": VIDEO, "reps": reps}
    idx.search_grouped(q0, 10, group_of=video)                            # labels: mapped and uploaded once
    calls = {
        "search_q1_k10": lambda: idx.search(q0, 10),
        "search_q1_k20": lambda: idx.search(q0, 20),
        "search_grouped_q1_k10": lambda: idx.search_grouped(q0, 10, group_of=video),
        "filtered_within_one_q1_k10": lambda: idx.search_filtered(q0, 10, within=one, group_of=video),
        "filtered_exclude_one_q1_k10": lambda: idx.search_filtered(q0, 10, exclude=one, group_of=video),
        "grouped_exclude_one_q1_k10": lambda: idx.search_grouped(q0, 10, group_of=video, exclude=one),
        "filtered_within_10pct_q1_k10": lambda: idx.search_filtered(q0, 10, within=pct10, group_of=video),
        "filtered_within_60pct_q1_k10": lambda: idx.search_filtered(q0, 10, within=pct60, group_of=video),
        "filtered_within_10pct_nq32_k10": lambda: idx.search_filtered_batch(list(qs[:32]), 10, within=pct10, group_of=video),
        "filtered_within_60pct_nq32_k10": lambda: idx.search_filtered_batch(list(qs[:32]), 10, within=pct60, group_of=video),
        "search_batch_nq32_k10": lambda: idx.search_batch(list(qs[:32]), 10),
        "filtered_exclude_one_nq256_k10": lambda: idx.search_filtered_batch(list(qs), 10, exclude=one, group_of=video),
        "search_batch_nq256_k10": lambda: idx.search_batch(list(qs), 10),
    }

    def forced(mode, fn):                                                 # one path, whatever mode 0 would choose
        def call():
            idx.search_mode = mode
            try:
                return fn()
            finally:
                idx.search_mode = 0
        return call
    for frac, sel in (("10pct", pct10), ("25pct", pct10 + pct60[: videos * 15 // 100]), ("60pct", pct60)):
        for nq in (1, 32):
            for mode, path in ((1, "gather"), (2, "fp16")):
                calls[f"crossover_within_{frac}_nq{nq}_{path}"] = forced(
                    mode, lambda sel=sel, nq=nq: idx.search_filtered_batch(list(qs[:nq]), 10, within=sel, group_of=video))
    calls["crossover_exclude_one_q1_gather"] = forced(1, lambda: idx.search_filtered(q0, 10, exclude=one, group_of=video))
    calls["grouped_exclude_one_q1_gather"] = forced(1, lambda: idx.search_grouped(q0, 10, group_of=video, exclude=one))
    for name, fn in calls.items():
        for _ in range(3):
            fn()
        heavy = "nq256" in name or "nq32" in name
        r = {"wall_ms": median_ms(fn, max(3, reps // 5) if heavy else reps)}
        r["stats"] = idx.last_search_stats()
        r["device_ms_by_class"] = classes(idx, fn, 3 if heavy else max(3, reps // 5))
        res[name] = r
        print(name, json.dumps(r), flush=True)
    with open(os.path.join(out, "filtered_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
    idx.close()


if __name__ == "__main__":
    main()
