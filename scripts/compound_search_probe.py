#!/usr/bin/env python3
"""Compound search latency over 1M x 512 video-like unit rows: 2,000 "videos" of 500 rows, each a random walk (v[i+1] =
normalize(v[i] + 0.2 g / sqrt(dim))).  16 terms = one stored row plus noise of norm 1.2 each (different noise per term), so
that rows near ALL terms exist; k = 20; everything device-resident, one process.
  compound vs plain                per m in 1, 3, 8, 16 (all-AND) and one mixed form with two veto terms, modes 2 and 1:
                                   vq_index_search_compound_device against vq_index_search_device with nq = m, the same k and
                                   mode, on the same handle in the same run; wall time = the call plus vq_index_synchronize,
                                   median after warm-up; device ms by kernel class (the index's event brackets); the call's
                                   outcome (last_search_stats: proven / rows re-scored / exact)
  crossover                        modes 1 and 2 (m = 3, all-AND) on prefixes of the rows: where the fp16 path starts to pay
usage: compound_search_probe.py OUTDIR [--quick]   (writes OUTDIR/probe.txt)"""
import ctypes
import json
import os
import sys
import time
from ctypes import c_float, c_void_p

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_quierer_amd import _lib  # noqa: E402
from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex  # noqa: E402

N, D, VIDEO, K = 1_000_000, 512, 500, 20
MIXED_VETO = [0, -1, 1, 1, 2, 2, 2, -1]


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


def build(rows, n):
    idx = OptimizedHNSWIndex(dimension=D)
    for c0 in range(0, n, 250_000):
        c = min(250_000, n - c0)
        torch.cuda.synchronize()
        idx.add_device(rows[c0:c0 + c].data_ptr(), c, range(c0, c0 + c), normalize=True)
        idx.synchronize()
    return idx


def main():
    out = sys.argv[1]
    reps = 5 if "--quick" in sys.argv else 30
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
    g.manual_seed(2200)
    videos = N // VIDEO
    rows = torch.empty((videos, VIDEO, D), device=dev)
    x = torch.randn((videos, D), device=dev, generator=g)
    x /= x.norm(dim=1, keepdim=True)
    for i in range(VIDEO):
        rows[:, i] = x
        x = x + torch.randn((videos, D), device=dev, generator=g) * (0.2 / D ** 0.5)
        x /= x.norm(dim=1, keepdim=True)
    rows = rows.reshape(N, D)
    terms = rows[777_123][None, :] + torch.randn((16, D), device=dev, generator=g) * (1.2 / D ** 0.5)
    terms = (terms / terms.norm(dim=1, keepdim=True)).contiguous()
    ids = torch.empty(16 * K, dtype=torch.int32, device=dev)
    dist = torch.empty(16 * K, dtype=torch.float32, device=dev)
    td = torch.empty(K * 16, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    lib = _lib.load()

    def compound(idx, m, clause_of, margin, mode):
        cl = np.array(clause_of, dtype=np.int32)

        def call():
            _lib.check(lib.vq_index_search_compound_device(idx._h, c_void_p(terms.data_ptr()), m, _lib.i32ptr(cl), c_float(margin), K, mode,
                                                           c_void_p(ids.data_ptr()), c_void_p(dist.data_ptr()), c_void_p(td.data_ptr())))
            idx.synchronize()
        return call

    def plain(idx, m, mode):
        def call():
            _lib.check(lib.vq_index_search_device(idx._h, c_void_p(terms.data_ptr()), m, K, mode, c_void_p(ids.data_ptr()),
                                                  c_void_p(dist.data_ptr())))
            idx.synchronize()
        return call

    idx = build(rows, N)
    say(f"# {N} x {D} rows, {videos} videos of {VIDEO} rows; 16 terms around one stored row; k = {K}; {reps} reps; wall ms = call + synchronize, median")
    for mode in (2, 1):
        say(f"mode {mode}:")
        cases = [(f"all-AND m = {m:2d}", m, list(range(m)), 0.0) for m in (1, 3, 8, 16)] + [("mixed 1|2|3 + 2 vetoes, m = 8", 8, MIXED_VETO, 0.0)]
        for name, m, clause_of, margin in cases:
            c, p = compound(idx, m, clause_of, margin, mode), plain(idx, m, mode)
            for _ in range(3):
                c(); p()
            c()
            st = idx.last_search_stats()
            tc, tp = median_ms(c, reps), median_ms(p, reps)
            say(f"  {name:32s} compound {tc:8.3f} ms | plain nq = {m:2d} {tp:8.3f} ms | ratio {tc / tp:5.2f} | stats {st}")
            say(f"      device ms by class, compound: {json.dumps(classes(idx, c, max(3, reps // 4)))}")
            say(f"      device ms by class, plain:    {json.dumps(classes(idx, p, max(3, reps // 4)))}")
    idx.close()
    say("crossover, m = 3 all-AND, compound wall ms by rows held; 'aimed': terms around stored row 1,000; 'unrelated': the terms above, "
        "whose row is not in the prefix")
    far = terms.clone()
    near = rows[1_000][None, :] + torch.randn((16, D), device=dev, generator=g) * (1.2 / D ** 0.5)
    near = (near / near.norm(dim=1, keepdim=True)).contiguous()
    for n in (4_096, 16_384, 32_768, 65_536, 131_072, 262_144, 524_288):
        sub = build(rows, n)
        parts = []
        for name, tset in (("aimed", near), ("unrelated", far)):
            terms.copy_(tset)
            torch.cuda.synchronize()
            t = {}
            for mode in (1, 2):
                c = compound(sub, 3, [0, 1, 2], 0.0, mode)
                for _ in range(3):
                    c()
                t[mode] = median_ms(c, reps)
            st = sub.last_search_stats()
            parts.append(f"{name}: mode 1 {t[1]:6.3f} | mode 2 {t[2]:6.3f} ms (proven {st['verified']}, re-scored {st['rescanned']})")
        say(f"  n = {n:7d}: " + " || ".join(parts))
        sub.close()


if __name__ == "__main__":
    main()
