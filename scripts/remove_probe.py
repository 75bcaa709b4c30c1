#!/usr/bin/env python3
"""Row-removal cost over 1M x 512 unit rows with the caller's string ids "video{v}_{i}" (300 frames per video), id ranks and
group labels on the device:
  remove 300 rows at the tail, in the middle, at the head (HNSWIndex.remove_batch; 3 repetitions each, the index shrinking)
  remove_group of one 300-frame video a quarter of the way in
  remove 10 % of the rows at random
  the rebuild it replaces: export the matrix, build a new index of the survivors, upload ranks and labels (first grouped search)
For every removal: the library call's device time (HIP events on the index's stream around vq_index_remove_rows), its host time,
the whole Python call's host time, the rows that moved and the bytes the compaction moved (18 per moved element: gather read +
scratch write, scratch read + fp32 write + fp16 write) over the device time.
usage: remove_probe.py OUTDIR [--quick]   (writes OUTDIR/remove_probe.json)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_quierer_amd import _lib  # noqa: E402
from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex  # noqa: E402

N, D, VIDEO = 1_000_000, 512, 300
BYTES_PER_MOVED_ELEM = 18


def main():
    out = sys.argv[1]
    n = 100_000 if "--quick" in sys.argv else N
    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(300)
    vecs = rng.standard_normal((n, D), dtype=np.float32)
    ids = [f"video{r // VIDEO}_{r % VIDEO}" for r in range(n)]
    idx = OptimizedHNSWIndex(dimension=D)
    idx.add_batch(vecs, ids)
    stream = torch.cuda.current_stream(dev)
    idx.set_stream(stream.cuda_stream)
    q = vecs[123] / np.linalg.norm(vecs[123])
    idx.search_grouped(q, 10)                                     # ranks and labels on the device
    idx.search(q, 10)
    del vecs

    real = _lib.load()
    last = {}

    class Timed:                                                  # brackets the library call with events on the index's stream
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != "vq_index_remove_rows":
                return fn

            def timed(h, rows, m):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                first = min(rows[i] for i in range(m))
                size = len(idx._ids)
                torch.cuda.synchronize()
                a.record(stream)
                t0 = time.perf_counter()
                rc = fn(h, rows, m)
                t1 = time.perf_counter()
                b.record(stream)
                b.synchronize()
                last.update(lib_host_ms=(t1 - t0) * 1e3, device_ms=a.elapsed_time(b), moved_rows=size - m - first, removed=m)
                return rc
            return timed
    _lib.load = lambda: Timed()

    def record(name, fn):
        last.clear()
        t0 = time.perf_counter()
        fn()
        r = dict(last, python_host_ms=(time.perf_counter() - t0) * 1e3, size_after=idx.size())
        moved_bytes = r["moved_rows"] * D * BYTES_PER_MOVED_ELEM
        r["moved_GB"] = moved_bytes / 1e9
        r["moved_TBps_over_device_time"] = moved_bytes / (r["device_ms"] * 1e-3) / 1e12 if r["moved_rows"] > 0 else None
        res["runs"].append(dict(r, case=name))
        print(name, json.dumps(r), flush=True)

    res = {"rows": n, "dim": D, "rows_per_video": VIDEO, "runs": []}
    record("warmup_tail_1", lambda: idx.remove_batch([idx._ids[-1]]))
    for rep in range(3):
        record("tail_300", lambda: idx.remove_batch(idx._ids[-300:]))
        record("middle_300", lambda: idx.remove_batch(idx._ids[len(idx._ids) // 2: len(idx._ids) // 2 + 300]))
        record("head_300", lambda: idx.remove_batch(idx._ids[:300]))
    record("remove_group_video", lambda: idx.remove_group(f"video{(n // VIDEO) // 4}"))       # a video the cases above left alone
    gone = rng.choice(idx.size(), idx.size() // 10, replace=False)
    record("random_10pct", lambda: idx.remove_batch([idx._ids[r] for r in gone]))
    _lib.load = lambda: real
    # the rebuild a removal replaces: the matrix to the host, a new index of the survivors, ranks and labels uploaded
    t0 = time.perf_counter()
    rows = idx._export()
    t1 = time.perf_counter()
    fresh = OptimizedHNSWIndex(dimension=D)
    fresh.add_batch(rows, list(idx._ids))
    t2 = time.perf_counter()
    fresh.search_grouped(q, 10)
    t3 = time.perf_counter()
    res["rebuild"] = {"rows": len(rows), "export_s": t1 - t0, "add_s": t2 - t1, "ranks_labels_first_search_s": t3 - t2, "total_s": t3 - t0}
    print("rebuild", json.dumps(res["rebuild"]), flush=True)
    same = [r["id"] for r in fresh.search_grouped(q, 10)] == [r["id"] for r in idx.search_grouped(q, 10)]
    res["pruned_equals_rebuilt_grouped_top10"] = same
    with open(os.path.join(out, "remove_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
    fresh.close(); idx.close()


if __name__ == "__main__":
    main()
