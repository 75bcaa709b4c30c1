#!/usr/bin/env python3
"""Diverse search latency over 1M x 512 video-like unit rows with planted repeats: 2,000 "videos" of 500 rows, each a random
walk (v[i+1] = normalize(v[i] + s g / sqrt(dim)), s = 0.2, and s = 0.01 inside one static shot of 150 frames per video); the
same 20-frame intro, with noise 0.02 / sqrt(dim), opens every fourth video.  64 queries = a stored row plus noise of norm 1.2:
16 aimed at the intro, 16 at static shots, 32 anywhere.
  depth table                      per producer and forced depth D ($VQ_AMD_DIVERSE_DEPTH): how many of the 64 queries the
                                   prefix proves at (k 10, min_dist 0.05), the call's wall time for one query and for the batch,
                                   and the device time by kernel class (the index's event brackets).  exact_dist_f64chain holds
                                   the pair pass (D^2) and the redo's distances and suppressions (k passes over the index);
                                   select_topk the walk and the redo's picks
  search(q, D) + read-back + host greedy
                                   the same answer without the call: the plain search at depth D, the D rows read back from
                                   the device, their D^2 / 2 distances in numpy (float64), the greedy walk (exact only while
                                   the prefix keeps k rows)
  proven / redo                    one query the rule's prefix proves and one it files, device ms by class
Wall times are medians of host-synchronous calls after warm-up.
usage: diverse_search_probe.py OUTDIR [--quick]   (writes OUTDIR/probe.txt)"""
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
K, MIN_DIST = 10, 0.05


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


def plan(n, nq, k, min_dist, mode):
    depth, producer, pair_bytes = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int64()
    slices, launches = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().vq_debug_diverse_plan(n, nq, k, ctypes.c_float(min_dist), mode, ctypes.byref(depth), ctypes.byref(producer),
                                                 ctypes.byref(pair_bytes), ctypes.byref(slices), ctypes.byref(launches)))
    return depth.value, producer.value, pair_bytes.value, slices.value, launches.value


def host_greedy(idx, rows, q, depth, k, min_dist):
    res = idx.search(q, depth)
    ids = torch.tensor([r["id"] for r in res], device=rows.device)
    x = rows[ids].cpu().numpy().astype(np.float64)                # the read-back: depth x dim floats
    close = (1.0 - x @ x.T).astype(np.float32) < np.float32(min_dist)
    kept = []
    for i in range(len(res)):
        if any(close[i, j] for j in kept):
            continue
        kept.append(i)
        if len(kept) == k:
            break
    return [res[i] for i in kept]


def main():
    out = sys.argv[1]
    quick = "--quick" in sys.argv
    reps = 3 if quick else 20
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
    g.manual_seed(2100)
    videos = N // VIDEO
    rows = torch.empty((videos, VIDEO, D), device=dev)
    x = torch.randn((videos, D), device=dev, generator=g)
    x /= x.norm(dim=1, keepdim=True)
    shot = torch.randint(50, VIDEO - 200, (videos, 1), device=dev, generator=g)      # where each video's static shot starts
    for i in range(VIDEO):
        rows[:, i] = x
        step = torch.where((i >= shot) & (i < shot + 150), 0.01, 0.2)
        x = x + torch.randn((videos, D), device=dev, generator=g) * (step / D ** 0.5)
        x /= x.norm(dim=1, keepdim=True)
    intro = rows[0, 100:120].clone()
    for v in range(4, videos, 4):
        rows[v, :20] = intro + torch.randn((20, D), device=dev, generator=g) * (0.02 / D ** 0.5)
    rows = rows.reshape(N, D)
    rows /= rows.norm(dim=1, keepdim=True)
    idx = OptimizedHNSWIndex(dimension=D)
    for c0 in range(0, N, 250_000):
        torch.cuda.synchronize()
        idx.add_device(rows[c0:c0 + 250_000].data_ptr(), 250_000, range(c0, c0 + 250_000), normalize=True)
        idx.synchronize()
    vsel = torch.randint(0, videos, (16,), device=dev, generator=g)
    src = torch.cat([100 + torch.randint(0, 20, (16,), device=dev, generator=g),
                     vsel * VIDEO + shot[vsel, 0] + 75,
                     torch.randint(0, N, (32,), device=dev, generator=g)])
    qs = rows[src] + torch.randn((64, D), device=dev, generator=g) * (1.2 / D ** 0.5)
    qs = (qs / qs.norm(dim=1, keepdim=True)).cpu().numpy()
    batch = list(qs)
    say(f"# {N} x {D} rows, {videos} videos of {VIDEO} rows, intro in {len(range(4, videos, 4)) + 1} videos, one static shot of 150 frames per video; "
        f"k = {K}, min_dist = {MIN_DIST}, {reps} reps; queries 0-15 intro, 16-31 static shots, 32-63 anywhere")
    rule = {}
    for mode, depths in ((0, (64, 100)), (1, (64, 128, 256, 512, 1024))):
        idx.search_mode = mode
        os.environ.pop("VQ_AMD_DIVERSE_DEPTH", None)
        rule[mode] = plan(N, 1, K, MIN_DIST, mode)
        say(f"mode {mode}: the rule's plan for one query: depth {rule[mode][0]}, producer {'fp16 scan' if rule[mode][1] else 'exact'}, "
            f"pair bytes {rule[mode][2]}, redo slices {rule[mode][3]}, launches {rule[mode][4]}")
        for depth in depths:
            os.environ["VQ_AMD_DIVERSE_DEPTH"] = str(depth)
            one = lambda: idx.search_diverse(qs[40], K, MIN_DIST)                    # noqa: E731
            many = lambda: idx.search_diverse_batch(batch, K, MIN_DIST)              # noqa: E731
            one(); many()
            st = idx.last_search_stats()
            say(f"  depth {depth:5d}: proven {st['verified']:2d} of 64, walked {st['rescanned']:6d}, redone {st['exact_fallback']:2d} | "
                f"one query (anywhere) {median_ms(one, reps):8.3f} ms | batch of 64 {median_ms(many, max(3, reps // 4)):9.3f} ms")
            say(f"      device ms by class, one query:   {json.dumps(classes(idx, one, max(3, reps // 4)))}")
            say(f"      device ms by class, batch of 64: {json.dumps(classes(idx, many, 3))}")
            say(f"      device ms by class, search(q, {depth}) x 64: {json.dumps(classes(idx, lambda: idx.search_batch(batch, depth), 3))}")
        os.environ.pop("VQ_AMD_DIVERSE_DEPTH", None)
    for mode in (0, 1):
        idx.search_mode = mode
        depth = rule[mode][0]
        say(f"mode {mode}, the rule's depth {depth}:")
        filed = []
        for q in qs:
            idx.search_diverse(q, K, MIN_DIST)
            filed.append(idx.last_search_stats()["exact_fallback"])
        say(f"  queries of 64 left to the redo: {sum(filed)} (intro {sum(filed[:16])}, static {sum(filed[16:32])}, anywhere {sum(filed[32:])})")
        for name, j in (("proven on the prefix", filed.index(0) if 0 in filed else None), ("redone", filed.index(1) if 1 in filed else None)):
            if j is None:
                continue
            call = lambda: idx.search_diverse(qs[j], K, MIN_DIST)                    # noqa: E731
            recipe = lambda: host_greedy(idx, rows, qs[j], depth, K, MIN_DIST)       # noqa: E731
            call(); recipe()
            same = [r["id"] for r in recipe()] == [r["id"] for r in call()]
            say(f"  query {j} ({name}):")
            say(f"    search_diverse(q, {K}, {MIN_DIST})                     {median_ms(call, reps):8.3f} ms   stats {idx.last_search_stats()}")
            say(f"    search(q, {depth}) + read-back + host greedy      {median_ms(recipe, reps):8.3f} ms   "
                f"(kept {len(recipe())} of {K}: {'the same answer' if same else 'NOT the answer'})")
            say(f"    device ms by class, search_diverse:  {json.dumps(classes(idx, call, max(3, reps // 4)))}")
            say(f"    device ms by class, search(q, {depth}):  {json.dumps(classes(idx, lambda: idx.search(qs[j], depth), max(3, reps // 4)))}")
    idx.close()


if __name__ == "__main__":
    main()
