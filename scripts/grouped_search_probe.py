#!/usr/bin/env python3
"""Grouped-search latency over 1M x 512 unit rows in 2,000 "videos" of 500 rows (contiguous, then the same labels shuffled):
  search_grouped(q, 10)            the grouped answer for one query (host in, list of dicts out)
  search(q, 20)                    today's caller call (video_search_system.py:297, k * 2 over-fetch)
  search_grouped_batch, nq 32/256  batches
Wall times are medians of host-synchronous calls after warm-up (the calls return only when the results are on the host);
per-kernel-class device times come from the index's event brackets (profile_begin / profile_end).
usage: grouped_search_probe.py OUTDIR [--quick]   (writes OUTDIR/grouped_probe.json)"""
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
    return float(np.median(ts))


def classes(idx, fn, reps):
    idx.profile_begin()
    for _ in range(reps):
        fn()
    return {k: round(v["ms"] / reps, 4) for k, v in idx.profile_end().items() if v["launches"]}


def main():
    out = sys.argv[1]
    quick = "--quick" in sys.argv
    reps = 5 if quick else 50
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
    contiguous = lambda nid: nid // VIDEO                                 # noqa: E731
    perm = np.random.default_rng(5).permutation(np.repeat(np.arange(N // VIDEO), VIDEO))
    shuffled = lambda nid: int(perm[nid])                                 # noqa: E731
    res = {"rows": N, "dim": D, "groups": N // VIDEO, "rows_per_group": VIDEO, "reps": reps, "layouts": {}}
    for name, fn in (("contiguous", contiguous), ("shuffled", shuffled)):
        t0 = time.perf_counter()
        idx.search_grouped(qs[0], 10, group_of=fn)                        # labels: mapped and uploaded once
        label_s = time.perf_counter() - t0
        for _ in range(5):
            idx.search_grouped(qs[0], 10, group_of=fn)
            idx.search(qs[0], 20)
        r = {"first_call_with_labelling_s": round(label_s, 3)}
        r["search_grouped_q1_k10_ms"] = median_ms(lambda: idx.search_grouped(qs[0], 10, group_of=fn), reps)
        r["stats_q1"] = idx.last_search_stats()
        r["search_q1_k20_ms"] = median_ms(lambda: idx.search(qs[0], 20), reps)
        for nq in (32, 256):
            batch = list(qs[:nq])
            idx.search_grouped_batch(batch, 10, group_of=fn)
            r[f"search_grouped_batch_nq{nq}_k10_ms"] = median_ms(lambda: idx.search_grouped_batch(batch, 10, group_of=fn), max(3, reps // 5))
            r[f"stats_nq{nq}"] = idx.last_search_stats()
        r["device_ms_by_class_grouped_q1"] = classes(idx, lambda: idx.search_grouped(qs[0], 10, group_of=fn), max(3, reps // 5))
        r["device_ms_by_class_grouped_nq32"] = classes(idx, lambda: idx.search_grouped_batch(list(qs[:32]), 10, group_of=fn), 3)
        r["device_ms_by_class_plain_q1_k20"] = classes(idx, lambda: idx.search(qs[0], 20), max(3, reps // 5))
        res["layouts"][name] = r
        print(name, json.dumps(r), flush=True)
    with open(os.path.join(out, "grouped_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
    idx.close()


if __name__ == "__main__":
    main()
