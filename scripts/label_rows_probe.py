#!/usr/bin/env python3
"""Zero-shot labelling latency on 1,000 videos x 1,000 frames x 512 video-like unit rows (a video is a random walk,
v[i+1] = normalize(v[i] + 0.2 g / sqrt(dim))) against P = 32, 256, 1,000 and 4,096 random unit prompts.
  per (P, mode 1 | 2):  label_rows() and label_groups(top=3): device ms (the index's event brackets, all classes added up; the
             fp16 tile pass, class scan_f16_mfma_top2, on its own) and the wall time of one synchronous Python call
             (host prompts in, numpy / dict out; label_groups builds 1,000 lists), with the call's stats
  baseline   what a caller can do without the call: the rows as an fp16 torch tensor, (rows @ prompts.T).argmax(1) in row chunks
             that keep the fp16 product within 512 MiB (no exactness contract, no tie rule, no distances, no tags)
  rooflines  the tile pass as a fraction of the fp16 MFMA peak, counting the flop it ISSUES (2 n P_pad dim over 2,517 TFLOP/s;
             P_pad = P rounded up to whole 256-prompt tiles) and, beside it, the useful share P / P_pad; and of the HBM peak
             (n dim 2 bytes per 2,048-prompt range over 8 TB/s)
  sweep      label_rows() in modes 1 and 2 over the first 16,384 / 65,536 / 262,144 rows at P = 32 and 256: the crossover the
             mode-0 rule (csrc/knn_label.h plan_label) is set from
Wall times are medians of host-synchronous calls after a warm-up call.  The GPU part runs in a child process under a time limit.
usage: label_rows_probe.py OUTDIR [--quick]   (writes OUTDIR/probe.txt)"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 512
HBM_PEAK = 8.0e12
MFMA_PEAK = 2.517e15
PS = (32, 256, 1000, 4096)
LIMIT = 900                    # seconds for the GPU part


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def device_ms(idx, fn, reps):
    idx.profile_begin()
    for _ in range(reps):
        fn()
    prof = idx.profile_end()
    return sum(c["ms"] for c in prof.values()) / reps, prof.get("scan_f16_mfma_top2", {"ms": 0.0})["ms"] / reps


def walk(torch, dev, gen, videos, frames):
    rows = torch.empty((videos, frames, D), device=dev)
    x = torch.randn((videos, D), device=dev, generator=gen)
    x /= x.norm(dim=1, keepdim=True)
    for i in range(frames):
        rows[:, i] = x
        x = x + torch.randn((videos, D), device=dev, generator=gen) * (0.2 / D ** 0.5)
        x /= x.norm(dim=1, keepdim=True)
    return rows.reshape(videos * frames, D)


def step(out, quick):
    import torch
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
    video = lambda nid: nid // frames                                     # noqa: E731
    rows16 = rows.half()
    say(f"# sweep: label_rows() over the first n rows, device ms (call ms), mode 1 | mode 2")
    for ns in (16_384, 65_536, 262_144):
        if ns > n:
            continue
        sub = OptimizedHNSWIndex(dimension=D)
        torch.cuda.synchronize()
        sub.add_device(rows[:ns].data_ptr(), ns, range(ns), normalize=True)
        sub.synchronize()
        for P in (32, 256):
            prompts = np.random.default_rng(P).standard_normal((P, D)).astype(np.float32)
            prompts /= np.linalg.norm(prompts, axis=1, keepdims=True)
            cells = []
            for mode in (1, 2):
                call = lambda: sub.label_rows(prompts, mode=mode)         # noqa: E731
                call()
                ms = median_ms(call, 11)
                dms, _ = device_ms(sub, call, 11)
                cells.append(f"{dms:.3f} ({ms:.3f})")
            say(f"n = {ns}, P = {P}: {cells[0]} | {cells[1]}")
        sub.close()
    del rows
    say(f"# {videos} videos x {frames} frames x {D}; prompts: random unit vectors")
    for P in PS:
        prompts = np.random.default_rng(P).standard_normal((P, D)).astype(np.float32)
        prompts /= np.linalg.norm(prompts, axis=1, keepdims=True)
        p16 = torch.from_numpy(prompts).to(dev).half()
        chunk = max(1, (512 << 20) // (2 * P))

        def torch_route():
            outl = torch.empty(n, dtype=torch.int64, device=dev)
            for c0 in range(0, n, chunk):
                outl[c0:c0 + chunk] = (rows16[c0:c0 + chunk] @ p16.T).argmax(1)
            return outl
        torch_route()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps_t = 3 if quick else 10
        e0.record()
        for _ in range(reps_t):
            base = torch_route()
        e1.record()
        torch.cuda.synchronize()
        base_ms = e0.elapsed_time(e1) / reps_t
        say(f"P = {P}: torch fp16 (rows @ prompts.T).argmax(1), {chunk}-row chunks: {base_ms:.3f} ms device")
        base = base.cpu().numpy()
        p_pad, ranges = -(-P // 256) * 256, -(-P // 2048)
        for mode in (1, 2):
            reps = 3 if mode == 1 or quick else 10
            idx.search_mode = mode
            rows_call = lambda: idx.label_rows(prompts, mode=mode)        # noqa: E731
            groups_call = lambda: idx.label_groups(prompts, top=3, group_of=video)      # noqa: E731
            lab, _ = rows_call()
            st = idx.last_search_stats()
            groups_call()
            ms_r, ms_g = median_ms(rows_call, reps), median_ms(groups_call, reps)
            d_r, tile = device_ms(idx, rows_call, reps)
            d_g, _ = device_ms(idx, groups_call, reps)
            say(f"  mode {mode}: label_rows device {d_r:.3f} ms, call {ms_r:.2f} ms | label_groups(top=3) device {d_g:.3f} ms, call {ms_g:.2f} ms | "
                f"{d_r / base_ms:.2f} x the torch route | stats {st} | labels equal to torch's argmax: {float((lab == base).mean()):.4f}")
            if mode == 2 and tile > 0:
                say(f"    tile pass {tile:.3f} ms: {100 * 2.0 * n * p_pad * D / (tile * 1e-3) / MFMA_PEAK:.1f} % of the fp16 MFMA peak in issued flop "
                    f"({100 * P / p_pad:.0f} % of them useful: P_pad = {p_pad}), "
                    f"{100 * n * D * 2.0 * ranges / (tile * 1e-3) / HBM_PEAK:.1f} % of the HBM peak")
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
