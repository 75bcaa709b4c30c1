#!/usr/bin/env python3
"""The pure Python cost of `index.search(q, 20)`: 20,000 calls on a 4,000-id index over a stand-in for the library (no GPU, no
device time), integer and string ids, for this tree's indexes/hnsw.py against another revision's copy of that file loaded
beside it — the two alternate in blocks of 500 calls in one process, so both see the same machine.
usage: search_python_cost.py <another revision's hnsw.py>   (e.g. from `git show <rev>:video-quierer_amd/indexes/hnsw.py`)"""
import ctypes, importlib.util, os, sys, threading, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_quierer_amd import _lib
from video_quierer_amd.indexes import hnsw as new_mod
spec = importlib.util.spec_from_file_location("hnsw_other", sys.argv[1])
old_mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(old_mod)

K = 20
ROWS = np.arange(100, 100 + K, dtype=np.int32)
DIST = np.linspace(0.1, 0.3, K).astype(np.float32)


class Fake:
    def vq_index_search(self, h, q, nq, k, mode, ids, dist):
        ctypes.memmove(ids, ROWS.ctypes.data, 4 * k)
        ctypes.memmove(dist, DIST.ctypes.data, 4 * k)
        return 0

    def vq_index_set_id_ranks(self, h, ptr, n):
        return 0


fake = Fake()
_lib.load = lambda: fake


def mk(mod, ids, identity):
    idx = mod.HNSWIndex.__new__(mod.HNSWIndex)
    idx._h, idx.dimension, idx.lock, idx.search_mode, idx.search_times = None, 512, threading.RLock(), 0, []
    if hasattr(idx, "_reset_host_state"):
        idx._reset_host_state()
    idx._ids = list(ids)
    idx._row_of = {nid: r for r, nid in enumerate(idx._ids)}
    idx._identity, idx._tie_order = identity, ("device" if identity else "stale")
    idx.element_count = len(idx._ids)
    idx.entry_point = idx._ids[0]
    return idx


q = np.random.default_rng(0).standard_normal(512).astype(np.float32)
for kind in ("int", "str"):
    ids = list(range(4000)) if kind == "int" else [f"video{r // 1000}_{r % 1000}" for r in range(4000)]
    a, b = mk(old_mod, ids, kind == "int"), mk(new_mod, ids, kind == "int")
    assert a.search(q, K) == b.search(q, K)
    ta, tb = [], []
    for block in range(40):
        for idx, ts in ((a, ta), (b, tb)) if block % 2 == 0 else ((b, tb), (a, ta)):
            for _ in range(500):
                t0 = time.perf_counter(); idx.search(q, K); ts.append(time.perf_counter() - t0)
            idx.search_times.clear()
    ta = np.array(ta).reshape(40, 500); tb = np.array(tb).reshape(40, 500)
    ma, mb = np.median(ta, axis=1) * 1e6, np.median(tb, axis=1) * 1e6
    print(f"{kind} ids, 20,000 calls each, interleaved in blocks of 500: other p50 {np.median(ta) * 1e6:.2f} us (quietest block {ma.min():.2f}), "
          f"this tree p50 {np.median(tb) * 1e6:.2f} us (quietest block {mb.min():.2f}); per-block-pair difference this tree - other: median {np.median(mb - ma):+.2f} us", flush=True)
