#!/usr/bin/env python3
"""Library clustering (vq_index_cluster) on 1,000 videos x 1,000 frames x 512 video-like unit rows (a video is a random walk,
v[i+1] = normalize(v[i] + 0.2 g / sqrt(dim))) at P = 32, 256, 1,000 and 4,096 clusters seeded from stored rows.
  per P      cluster(P, max_iter=ITERS): wall ms of the synchronous call, iterations, rows still changing in the last one;
             device ms of ONE iteration, split: the assignment (label_rows on the centroids the call returned, mode 0, every
             class of the index's event brackets added up), then through vq_index_debug_cluster_update on the labels the call
             returned: the by-label list (class select_topk: histogram, prefix, scan, scatter), the piece sums (class
             exact_dist_f64chain) and the finish (class normalize_rows)
  baseline   what a caller can do without the call, on the same box: rows as an fp16 torch tensor, (rows16 @ C16.T).argmax(1)
             in row chunks that keep the product within 512 MiB, then sums.index_add_(0, labels, rows) in fp32 and a row
             normalisation: neither reproducible (atomic adds in arrival order) nor tie-defined
  streaming  the piece pass reads the fp32 master once (n x dim x 4 bytes): its rate over the 8 TB/s HBM peak, and over what
             torch's rows.sum(0) reaches on the same tensor (a streaming read of the same bytes)
Wall times are medians of host-synchronous calls after a warm-up call.  The GPU part runs in a child process under a time limit.
usage: cluster_probe.py OUTDIR [--quick]   (writes OUTDIR/probe.txt)"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 512
HBM_PEAK = 8.0e12
PS = (32, 256, 1000, 4096)
ITERS = 5
LIMIT = 900                    # seconds for the GPU part


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def class_ms(idx, fn, reps):
    idx.profile_begin()
    for _ in range(reps):
        fn()
    return {name: c["ms"] / reps for name, c in idx.profile_end().items()}


def walk(torch, dev, gen, videos, frames):
    rows = torch.empty((videos, frames, D), device=dev)
    x = torch.randn((videos, D), device=dev, generator=gen)
    x /= x.norm(dim=1, keepdim=True)
    for i in range(frames):
        rows[:, i] = x
        x = x + torch.randn((videos, D), device=dev, generator=gen) * (0.2 / D ** 0.5)
        x /= x.norm(dim=1, keepdim=True)
    return rows.reshape(videos * frames, D)


def torch_ms(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def step(out, quick):
    import torch
    from video_quierer_amd import _lib
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    videos, frames = (200, 500) if quick else (1_000, 1_000)
    n = videos * frames
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5000)
    lines = []

    def say(*a):
        line = " ".join(str(x) for x in a)
        print(line, flush=True)
        lines.append(line)
        with open(os.path.join(out, "probe.txt"), "w") as f:              # kept current: a later part may take long
            f.write("\n".join(lines) + "\n")

    rows = walk(torch, dev, gen, videos, frames)
    idx = OptimizedHNSWIndex(dimension=D)
    for c0 in range(0, n, 250_000):
        c1 = min(n, c0 + 250_000)
        torch.cuda.synchronize()
        idx.add_device(rows[c0:c1].data_ptr(), c1 - c0, range(c0, c1), normalize=True)
        idx.synchronize()
    rows16 = rows.half()
    lib = _lib.load()
    reps = 3 if quick else 10
    master = n * D * 4.0
    read_ms = torch_ms(torch, lambda: rows.sum(0), reps)
    say(f"# {videos} videos x {frames} frames x {D}; clusters seeded from stored rows (seed 1); max_iter {ITERS}, mode 0")
    say(f"# a streaming read of the fp32 master ({master / 1e9:.2f} GB): torch rows.sum(0) {read_ms:.3f} ms = {master / (read_ms * 1e-3) / 1e12:.2f} TB/s; "
        f"at the {HBM_PEAK / 1e12:.0f} TB/s HBM peak {master / HBM_PEAK * 1e3:.3f} ms")
    for P in PS:
        call = lambda: idx.cluster(P, max_iter=ITERS, seed=1)             # noqa: E731
        res = call()
        wall = median_ms(call, 3)
        cen, labels = res["centroids"], np.ascontiguousarray(res["labels"])
        sizes = np.array([c["size"] for c in res["clusters"]])
        pieces = int((-(-sizes // 1024)).sum())
        say(f"P = {P}: cluster() call {wall:.2f} ms for {res['iterations']} iterations ({wall / res['iterations']:.2f} ms each), changed {res['changed']}; "
            f"sizes {sizes.min()} .. {sizes.max()}, {pieces} pieces")
        a = class_ms(idx, lambda: idx.label_rows(cen, mode=0), reps)
        st = idx.last_search_stats()
        cout, counts = np.empty_like(cen), np.empty(P, dtype=np.int32)
        upd = lambda: _lib.check(lib.vq_index_debug_cluster_update(idx._h, _lib.i32ptr(labels), P, _lib.fptr(cen), _lib.fptr(cout), _lib.i32ptr(counts)))  # noqa: E731
        upd()
        u = class_ms(idx, upd, reps)
        assign, lst, piece, finish = sum(a.values()), u["select_topk"], u["exact_dist_f64chain"], u["normalize_rows"]
        say(f"  device ms per iteration: assignment {assign:.3f} (stats {st}) | list {lst:.3f} | piece sums {piece:.3f} | finish {finish:.3f} | "
            f"update {lst + piece + finish:.3f} = {100 * (lst + piece + finish) / (assign + lst + piece + finish):.0f} % of the iteration")
        say(f"  piece sums: {master / (piece * 1e-3) / 1e12:.2f} TB/s of the master = {100 * master / (piece * 1e-3) / HBM_PEAK:.0f} % of the HBM peak, "
            f"{100 * read_ms / piece:.0f} % of torch's streaming read")
        c16 = torch.from_numpy(cen).to(dev).half()
        chunk = max(1, (512 << 20) // (2 * P))

        def torch_assign():
            lab = torch.empty(n, dtype=torch.int64, device=dev)
            for c0 in range(0, n, chunk):
                lab[c0:c0 + chunk] = (rows16[c0:c0 + chunk] @ c16.T).argmax(1)
            return lab

        def torch_iteration():
            sums = torch.zeros((P, D), device=dev)
            sums.index_add_(0, torch_assign(), rows)
            return sums / sums.norm(dim=1, keepdim=True).clamp_min(1e-30)
        t_all = torch_ms(torch, torch_iteration, reps)
        lab_t = torch_assign()
        t_add = torch_ms(torch, lambda: torch.zeros((P, D), device=dev).index_add_(0, lab_t, rows), reps)
        say(f"  torch fp16 argmax + fp32 index_add_ + normalise: {t_all:.3f} ms per iteration (index_add_ alone {t_add:.3f}); ours "
            f"{(assign + lst + piece + finish) / t_all:.2f} x that")
    idx.close()


def main():
    out = sys.argv[1]
    quick = "--quick" in sys.argv
    os.makedirs(out, exist_ok=True)
    if "--step" in sys.argv:
        return step(out, quick)
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), out, "--step"] + (["--quick"] if quick else [])
    rc = subprocess.call(cmd)
    if rc != 0:
        with open(os.path.join(out, "probe.txt"), "a") as f:
            f.write(f"the GPU part ended with status {rc}: the probe stops here\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
