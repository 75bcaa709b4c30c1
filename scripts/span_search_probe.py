#!/usr/bin/env python3
"""Span search latency over 1M x 512 video-like unit rows: 2,000 "videos" of 500 rows, each a random walk
(v[i+1] = normalize(v[i] + 0.2 g / sqrt(dim))), positions = the frame number; queries = frames of some videos plus noise of
norm 0.3; tau = the 1 % quantile of the first query's distances.
  search_spans(q, 10, max_distance=tau)                 nq = 1, both limits unlimited (every range starts at 0: prefix minima)
  search_spans(q, 10, max_distance=tau, max_span=60)    the same with ranges of at most 61 rows (read one by one)
  search_spans(q, 10, max_distance=tau, max_gap=1)      (frame numbers: no gap bites; the max-scan alone)
  search_spans_batch(16 queries, ...)                   one chunk of 16 queries
  search_sequence([q], 10, max_gap=8)                   the nearest existing call: the same distance pass, one DP launch
each as the wall time of the host-synchronous call (median after warm-up) and as device time by kernel class from the index's
event brackets: exact_dist_f64chain is the distance pass, sequence_dp the span kernels (DP and finish), select_topk the
per-query selection and the counters.  The answer of the first call is compared with a numpy walk over the call's own exported
rows (distances by numpy: masses compared to a tolerance, spans exactly where the masses are apart).
  one group of 1M rows                                  the global form's bound: one workgroup walks the whole index
usage: span_search_probe.py OUTDIR [--quick]   (writes OUTDIR/probe.txt)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_quierer_amd.indexes.hnsw import MODE_EXACT, OptimizedHNSWIndex  # noqa: E402

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


def host_spans(d, tau, k):
    """Unlimited spans of videos of VIDEO consecutive rows: per video the best (mass, shortest, earliest) run by Kadane's walk
    over the integer gains.  d [N] float32 -> [(video, mass, start row, end row)] for the k best."""
    w = np.rint((np.float64(tau) - d.astype(np.float64)) * 2.0 ** 24).astype(np.int64).reshape(-1, VIDEO)
    out = []
    for v in range(len(w)):
        P = np.concatenate([[0], np.cumsum(w[v])])
        best = None
        cur = 0
        for b in range(VIDEO):
            if P[b] <= P[cur]:
                cur = b
            c = (-(P[b + 1] - P[cur]), b - cur + 1, cur)
            if best is None or c < best:
                best = c
        if -best[0] > 0:
            out.append((v, int(-best[0]), v * VIDEO + best[2], v * VIDEO + best[2] + best[1] - 1))
    out.sort(key=lambda t: (np.float32(-float(t[1]) * 2.0 ** -24), t[0]))
    return out[:k]


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
    src = (777 + 70 * torch.arange(16, device=dev)) * VIDEO + 240          # videos 777 .. 1,827 of 2,000
    queries = rows[src] + torch.randn((16, D), device=dev, generator=g) * (0.3 / D ** 0.5)
    queries = (queries / queries.norm(dim=1, keepdim=True)).cpu().numpy()
    del rows, x
    video = lambda nid: nid // VIDEO                              # noqa: E731
    frame = lambda nid: nid % VIDEO                               # noqa: E731
    idx.search_mode = MODE_EXACT
    q = queries[0]
    stored = idx._export()
    d_np = (np.float32(1.0) - stored @ np.ascontiguousarray(idx._unit_rows([q]), dtype=np.float32)[0]).astype(np.float32)
    tau = float(np.float32(np.quantile(d_np, 0.01)))
    say(f"# {N} x {D} rows, {videos} videos of {VIDEO} rows, positions = frame numbers, k = 10, tau = {tau:.6f} (1 % quantile of query 0), {reps} reps")
    kw = dict(max_distance=tau, group_of=video, position_of=frame)
    t0 = time.perf_counter()
    first = idx.search_spans(q, 10, **kw)
    say(f"first call (labels and positions mapped and uploaded, the (position, tie) order sorted and uploaded): {time.perf_counter() - t0:.2f} s")
    want = host_spans(d_np, np.float32(tau), 10)
    got = [(r["group"], r["mass"], r["start_id"], r["end_id"]) for r in first]
    masses_close = len(got) == len(want) and all(abs(a[1] - b[1] * 2.0 ** -24) < 1e-3 for a, b in zip(got, want))
    say(f"answer: {len(first)} videos, best {first[0]['group']} frames {first[0]['start']}..{first[0]['end']} ({first[0]['frames']} rows, "
        f"score {first[0]['score']:.4f}); numpy walk on numpy distances: same videos {[a[0] for a in got] == [b[0] for b in want]}, "
        f"masses within 1e-3 {masses_close}, same spans {[a[2:] for a in got] == [b[2:] for b in want]}")
    assert first[0]["group"] == 777 and first[0]["start"] <= 240 <= first[0]["end"], first[0]
    del stored, d_np
    say("call | wall ms | device ms: exact_dist  sequence_dp  select | span kernels / distance pass | stats")
    calls = [("search_spans nq 1 unlimited", lambda: idx.search_spans(q, 10, **kw)),
             ("search_spans nq 1 max_span 60", lambda: idx.search_spans(q, 10, max_span=60, **kw)),
             ("search_spans nq 1 max_gap 1", lambda: idx.search_spans(q, 10, max_gap=1, **kw)),
             ("search_spans nq 1 max_gap 1 max_span 300", lambda: idx.search_spans(q, 10, max_gap=1, max_span=300, **kw)),
             ("search_spans_batch nq 16 unlimited", lambda: idx.search_spans_batch(list(queries), 10, **kw)),
             ("search_spans_batch nq 16 max_span 60", lambda: idx.search_spans_batch(list(queries), 10, max_span=60, **kw)),
             ("search_sequence m 1 max_gap 8", lambda: idx.search_sequence([q], 10, max_gap=8, group_of=video, position_of=frame))]
    for name, fn in calls:
        for _ in range(3):
            fn()
        ms = median_ms(fn, reps)
        cls = classes(idx, fn, max(3, reps // 5))
        dp, dist = cls.get("sequence_dp", 0.0), cls.get("exact_dist_f64chain", 0.0)
        say(f"{name:42s} | {ms:8.3f} | {dist:8.4f} {dp:8.4f} {cls.get('select_topk', 0.0):8.4f} | {dp / dist:6.3f} | {idx.last_search_stats()}")
    # the bound: one group holding every row
    one = lambda nid: 0                                           # noqa: E731
    ident = lambda nid: nid                                       # noqa: E731
    for label, extra in (("unlimited", {}), ("max_span 60", {"max_span": 60}), ("max_span 100000", {"max_span": 100_000})):
        fn = lambda: idx.search_spans(q, 10, max_distance=tau, group_of=one, position_of=ident, **extra)  # noqa: E731
        t0 = time.perf_counter()
        res = fn()
        first_ms = (time.perf_counter() - t0) * 1e3
        cls = classes(idx, fn, 1)
        say(f"one group of {N} rows, {label}: {first_ms:9.1f} ms the first call, device ms by class {json.dumps(cls)}   "
            f"({len(res)} result, {res[0]['frames'] if res else 0} rows, stats {idx.last_search_stats()})")
    idx.close()


if __name__ == "__main__":
    main()
