#!/usr/bin/env python3
"""Host time per call of every search family's two entry points, through ctypes on a small index (300 rows of dim 64, mode 1:
the kernels are short, what is left is the host layer of csrc/vq_index.hip): p50 / p95 in microseconds of
  host           the host form (queries up, run, results back, one wait)
  device+sync    the _device form on device arrays, then vq_index_synchronize
  empty host / empty device+sync   the same two on an index that holds no row (the empty answer alone)
The families, their arguments and arrays are those of tests/test_index_host_forms.py.  Select another build with $VQ_AMD_LIB.
usage: host_forms_probe.py [reps]"""
import os
import sys
import time
from ctypes import byref, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_index_host_forms as T  # noqa: E402
from video_quierer_amd import _lib  # noqa: E402


def percentiles(fn, reps):
    for _ in range(10):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return 1e6 * ts[len(ts) // 2], 1e6 * ts[int(len(ts) * 0.95)]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    _lib.init(0)
    lib = _lib.load()
    d = T._data()
    h, empty = c_void_p(), c_void_p()
    _lib.check(lib.vq_index_create(T.DIM, byref(h)))
    _lib.check(lib.vq_index_add(h, T._hptr(d["rows"]), T.N, 0))
    _lib.check(lib.vq_index_set_groups(h, T._hptr(d["group"]), T.N, len(T.LENGTHS)))
    _lib.check(lib.vq_index_set_positions(h, T._hptr(d["pos"]), T.N))
    _lib.check(lib.vq_index_set_id_ranks(h, T._hptr(d["rank"]), T.N))
    _lib.check(lib.vq_index_create(T.DIM, byref(empty)))
    fams, _keep = T._families(d)
    hip = T.Hip()
    print(f"# library {_lib.LIB_PATH}; {T.N} x {T.DIM} rows, k = {T.K}, mode 1, every output asked for; p50 (p95) us over {reps} calls", flush=True)
    print("family | host | device+sync | empty host | empty device+sync", flush=True)
    for fam in fams:
        cols = []
        for handle in (h, empty):
            f = fam
            if handle is empty and fam.host == "vq_index_neighbors":
                f = T.Family(fam.name, fam.host, None, fam.outs, lambda q, o: (None, 0, T.K, 0, 1, *o))
            arrs = T._canaries(f, True)
            hargs = f.args(T._hptr(f.q) if f.q is not None else None, [T._hptr(arrs[o.name]) for o in f.outs])
            dargs = f.args(hip.array(f.q) if f.q is not None else None, [hip.array(arrs[o.name]) for o in f.outs])
            hfn, dfn = getattr(lib, f.host), getattr(lib, f.device)

            def host_call():
                assert hfn(handle, *hargs) == 0, lib.vq_last_error()

            def device_call():
                assert dfn(handle, *dargs) == 0, lib.vq_last_error()
                lib.vq_index_synchronize(handle)
            cols += [percentiles(host_call, reps), percentiles(device_call, reps)]
        print(f"{fam.name:18s} | " + " | ".join(f"{a:8.1f} ({b:8.1f})" for a, b in cols), flush=True)
        hip.free()
    # the clustering call (P = 4, 3 iterations from four listed rows), whose forms take different arguments
    import numpy as np
    from ctypes import c_int
    init_rows = _keep[1]
    outs = [T._canary(t, s) for t, s in ((T.F32, (4, T.DIM)), (T.I32, (T.N,)), (T.F32, (T.N,)), (T.I32, (4,)), (T.I32, (4,)))]
    it, changed = c_int(0), np.zeros(3, dtype=T.I32)
    cols = []
    for handle in (h, empty):
        hp, dp, drows = [T._hptr(a) for a in outs], [hip.array(a) for a in outs], hip.array(init_rows)

        def host_call():
            assert lib.vq_index_cluster(handle, None, T._hptr(init_rows), 4, 3, 1, *hp, byref(it), T._hptr(changed)) == 0, lib.vq_last_error()

        def device_call():
            assert lib.vq_index_cluster_device(handle, None, drows, 4, 3, 1, *dp) == 0, lib.vq_last_error()
            lib.vq_index_synchronize(handle)
        cols += [percentiles(host_call, reps), percentiles(device_call, reps)]
    print(f"{'cluster':18s} | " + " | ".join(f"{a:8.1f} ({b:8.1f})" for a, b in cols), flush=True)
    hip.free()
    lib.vq_index_destroy(h)
    lib.vq_index_destroy(empty)


if __name__ == "__main__":
    main()
