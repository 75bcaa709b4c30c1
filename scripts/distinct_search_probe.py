#!/usr/bin/env python3
"""Distinct-moment search latency over 1M x 512 video-like unit rows: 2,000 "videos" of 500 rows, each a random walk
(v[i+1] = normalize(v[i] + 0.2 g / sqrt(dim))), queries = a stored row plus noise of norm 1.2.
  search_distinct(q, 10, gap)      gap 3 and 50 (host in, list of dicts out)
  search(q, D) + host greedy       the same answer without the call: the plain search at the plan's depth D, then the greedy
                                   walk over its result in Python (exact only while the prefix keeps k rows)
  device time by kernel class      the index's event brackets (profile_begin / profile_end): the distinct call against
                                   search(q, D) alone; the difference is the prefix kernel plus the redo launches that leave at
                                   once, and a gap-0 call at the same depth (no redo queued) splits the two
  forced redo                      VQ_AMD_DISTINCT_DEPTH=16: the exact path's price for one query
  one group of 1M rows, k = 100    the documented worst case of the per-group walk (one wave walks the whole index)
Wall times are medians of host-synchronous calls after warm-up.
usage: distinct_search_probe.py OUTDIR [--quick]   (writes OUTDIR/probe.txt)"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_quierer_amd import _lib  # noqa: E402
from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex  # noqa: E402

N, D, VIDEO = 1_000_000, 512, 500


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


def plan(n, nq, k, gap, mode):
    depth, producer, slices = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().vq_debug_distinct_plan(n, nq, k, gap, mode, ctypes.byref(depth), ctypes.byref(producer), ctypes.byref(slices)))
    return depth.value, producer.value, slices.value


def host_greedy(res, k, gap):
    kept, seen = [], {}
    for r in res:
        g, p = r["id"] // VIDEO, r["id"]
        s = seen.setdefault(g, [])
        if any(abs(p - o) < gap for o in s):
            continue
        s.append(p)
        kept.append(r)
        if len(kept) == k:
            break
    return kept


def main():
    out = sys.argv[1]
    quick = "--quick" in sys.argv
    reps = 5 if quick else 50
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
    g.manual_seed(2000)
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
    src = torch.randint(0, N, (64,), device=dev, generator=g)
    qs = rows[src] + torch.randn((64, D), device=dev, generator=g) * (1.2 / D ** 0.5)
    qs = (qs / qs.norm(dim=1, keepdim=True)).cpu().numpy()
    del rows, x
    video = lambda nid: nid // VIDEO                              # noqa: E731
    say(f"# {N} x {D} rows, {videos} videos of {VIDEO} rows, positions = row numbers, k = 10, mode 0 (fp16 scan), {reps} reps")
    t0 = time.perf_counter()
    idx.search_distinct(qs[0], 10, 3, group_of=video)
    say(f"first call (labels and positions mapped and uploaded): {time.perf_counter() - t0:.2f} s")
    for gap in (3, 50):
        depth, producer, slices = plan(N, 1, 10, gap, 0)
        distinct = lambda: idx.search_distinct(qs[0], 10, gap, group_of=video)        # noqa: E731
        recipe = lambda: host_greedy(idx.search(qs[0], depth), 10, gap)               # noqa: E731
        for _ in range(5):
            distinct(); recipe()
        say(f"gap {gap}: plan depth {depth}, producer {'fp16 scan' if producer else 'exact'}, redo slices {slices}")
        say(f"  search_distinct(q, 10, {gap})            {median_ms(distinct, reps):8.3f} ms   stats {idx.last_search_stats()}")
        say(f"  search(q, {depth}) + host greedy          {median_ms(recipe, reps):8.3f} ms   "
            f"(kept {len(recipe())} of 10: {'the same answer' if [r['id'] for r in recipe()] == [r['id'] for r in distinct()] else 'NOT the answer'})")
        filed = []
        for q in qs:
            idx.search_distinct(q, 10, gap, group_of=video)
            filed.append(idx.last_search_stats()["exact_fallback"])
        say(f"  queries of 64 left to the redo at this depth: {sum(filed)}")
        say(f"  device ms by class, search_distinct:     {json.dumps(classes(idx, distinct, max(3, reps // 5)))}")
        say(f"  device ms by class, search(q, {depth}):      {json.dumps(classes(idx, lambda: idx.search(qs[0], depth), max(3, reps // 5)))}")
    depth = plan(N, 1, 10, 3, 0)[0]
    same_depth_no_redo = lambda: idx.search_distinct(qs[0], depth, 0, group_of=video)  # noqa: E731
    same_depth_no_redo()
    say(f"gap 0, k = {depth} (the same prefix, walked without suppression, no redo queued):")
    say(f"  device ms by class:                      {json.dumps(classes(idx, same_depth_no_redo, max(3, reps // 5)))}")
    os.environ["VQ_AMD_DISTINCT_DEPTH"] = "16"
    forced = lambda: idx.search_distinct(qs[0], 10, 3, group_of=video)                 # noqa: E731
    forced()
    say("forced redo (depth 16), one query, gap 3:")
    say(f"  search_distinct(q, 10, 3)                {median_ms(forced, max(3, reps // 5)):8.3f} ms   stats {idx.last_search_stats()}")
    say(f"  device ms by class:                      {json.dumps(classes(idx, forced, 3))}")
    del os.environ["VQ_AMD_DISTINCT_DEPTH"]
    one = lambda nid: 0                                           # noqa: E731
    idx.search_distinct(qs[0], 10, 0, group_of=one)                # relabel: one group of 1M rows
    t0 = time.perf_counter()
    res = idx.search_distinct(qs[0], 100, 50, group_of=one)
    say(f"one group of {N} rows, k = 100, gap 50:      {(time.perf_counter() - t0) * 1e3:8.1f} ms   "
        f"(one call, {len(res)} results, stats {idx.last_search_stats()})")
    idx.close()


if __name__ == "__main__":
    main()
