#!/usr/bin/env python3
"""Clip-search latency over 1M x 512 unit rows in 2,000 "videos" of 500 rows (contiguous, then the same labels shuffled):
  search_set(clip of m frames, k = 10), m in {16, 64, 256, 1024}, fp16 path (mode 2) and, for m <= 64, the exact path (mode 1)
  yardstick for pass 1: search_grouped_batch at nq = 256 (its group-max scan reads the matrix once per 16 queries; the kernel is
  the one the clip search itself uses for m <= 16) and the plain batch scan of search_batch at nq = 256 (one 256-query tile pass)
  yardstick for the whole call: the only route without search_set — search_grouped_batch(clip, k = 1000) in mode 1 plus the
  sum on the host, on 1,000 videos x 1,000 rows (the k <= 1024 check allows no more videos)
Wall times are medians of host-synchronous calls after warm-up; device times come from the index's event brackets
(profile_begin / profile_end): "scan_f16_mfma_top2" is pass 1, the other classes are the rest of the call.
usage: set_search_probe.py OUTDIR [--quick]   (writes OUTDIR/set_probe.json)"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_quierer_amd import _lib  # noqa: E402
from video_quierer_amd.indexes.hnsw import MODE_EXACT, MODE_FP16, OptimizedHNSWIndex  # noqa: E402

N, D, VIDEO = 1_000_000, 512, 500
F16_DENSE_PEAK = 2.5e15            # MI355X fp16 / bf16 MFMA, dense (FLOP/s)


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


def split(cls):
    p1 = cls.get("scan_f16_mfma_top2", 0.0)
    return {"pass1_ms": round(p1, 4), "rest_ms": round(sum(cls.values()) - p1, 4)}


def main():
    out = sys.argv[1]
    quick = "--quick" in sys.argv
    reps = 3 if quick else 15
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
    rng = np.random.default_rng(7)
    # the clip: noisy copies of the frames of video 777 (repeated past its 500 rows), as a re-encode would give
    rn = np.array([777 * VIDEO + (i % VIDEO) for i in range(1024)], dtype=np.int64)
    rows = np.empty((1024, D), dtype=np.float32)
    _lib.check(_lib.load().vq_index_read_rows(idx._h, rn.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(rn), _lib.fptr(rows)))
    clip = rows + np.float32(0.5 / np.sqrt(D)) * rng.standard_normal(rows.shape).astype(np.float32)
    qs = rng.standard_normal((256, D)).astype(np.float32)
    contiguous = lambda nid: nid // VIDEO                                 # noqa: E731
    perm = np.random.default_rng(5).permutation(np.repeat(np.arange(N // VIDEO), VIDEO))
    shuffled = lambda nid: int(perm[nid])                                 # noqa: E731
    res = {"rows": N, "dim": D, "groups": N // VIDEO, "rows_per_group": VIDEO, "reps": reps, "layouts": {}}
    flop_256 = 2.0 * 256 * N * D
    for name, fn in (("contiguous", contiguous), ("shuffled", shuffled)):
        r = {}
        idx.search_mode = MODE_FP16
        idx.search_set(list(clip[:16]), 10, group_of=fn)                  # labels: mapped and uploaded once
        for m in (16, 64, 256, 1024):
            frames = list(clip[:m])
            call = lambda: idx.search_set(frames, 10, group_of=fn)        # noqa: E731
            call(); call()
            r[f"search_set_m{m}_k10_ms"] = round(median_ms(call, reps), 3)
            r[f"stats_m{m}"] = idx.last_search_stats()
            cls = classes(idx, call, max(3, reps // 3))
            r[f"device_m{m}"] = dict(split(cls), by_class=cls)
        p1 = r["device_m256"]["pass1_ms"]
        r["pass1_m256_tflops"] = round(flop_256 / (p1 * 1e-3) / 1e12, 1)
        r["pass1_m256_share_of_f16_dense_peak"] = round(flop_256 / (p1 * 1e-3) / F16_DENSE_PEAK, 4)
        for m in (16, 64):
            idx.search_mode = MODE_EXACT
            frames = list(clip[:m])
            call = lambda: idx.search_set(frames, 10, group_of=fn)        # noqa: E731
            call()
            r[f"search_set_exact_m{m}_k10_ms"] = round(median_ms(call, max(3, reps // 3)), 3)
        idx.search_mode = MODE_FP16
        batch = list(qs)
        gcall = lambda: idx.search_grouped_batch(batch, 10, group_of=fn)  # noqa: E731
        gcall(); gcall()
        r["search_grouped_batch_nq256_k10_ms"] = round(median_ms(gcall, reps), 3)
        gcls = classes(idx, gcall, max(3, reps // 3))
        r["device_grouped_batch_nq256"] = dict(split(gcls), by_class=gcls)
        clipcall = lambda: idx.search_grouped_batch(list(clip[:256]), 10, group_of=fn)     # noqa: E731  (the same 256 frames as m = 256)
        clipcall()
        r["device_grouped_batch_clip256"] = split(classes(idx, clipcall, max(3, reps // 3)))
        pcall = lambda: idx.search_batch(batch, 10)                       # noqa: E731
        pcall(); pcall()
        pcls = classes(idx, pcall, max(3, reps // 3))
        r["device_plain_batch_nq256"] = dict(split(pcls), by_class=pcls)
        r["pass1_m256_over_grouped_batch_scan"] = round(p1 / r["device_grouped_batch_clip256"]["pass1_ms"], 4)
        res["layouts"][name] = r
        print(name, json.dumps(r), flush=True)

    # the whole call against the only route without it: 1,000 videos x 1,000 rows, k = all of them, mode 1, host sum
    thousand = lambda nid: nid // 1000                                    # noqa: E731
    w = {}
    for m in (16, 64):
        frames = list(clip[:m])
        idx.search_mode = MODE_EXACT

        def emulate():
            per = idx.search_grouped_batch(frames, 1000, group_of=thousand)
            acc = np.zeros(1000, dtype=np.float64)
            for rr in per:
                for x in rr:
                    acc[x["group"]] += float(x["distance"])
            d = (acc / len(frames)).astype(np.float32)
            return np.lexsort((np.arange(1000), d))[:10], d
        order, d = emulate()
        w[f"emulated_m{m}_ms"] = round(median_ms(emulate, 3), 3)
        for mode, tag in ((MODE_EXACT, "exact"), (MODE_FP16, "fp16")):
            idx.search_mode = mode
            call = lambda: idx.search_set(frames, 10, group_of=thousand)  # noqa: E731
            got = call()
            assert [x["group"] for x in got] == order.tolist() and [x["distance"] for x in got] == d[order].tolist(), (m, tag)
            w[f"search_set_{tag}_m{m}_ms"] = round(median_ms(call, max(3, reps // 3)), 3)
            w[f"emulated_over_search_set_{tag}_m{m}"] = round(w[f"emulated_m{m}_ms"] / w[f"search_set_{tag}_m{m}_ms"], 1)
    res["whole_call_1000x1000"] = w
    print("whole_call", json.dumps(w), flush=True)
    with open(os.path.join(out, "set_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
    idx.close()


if __name__ == "__main__":
    main()
