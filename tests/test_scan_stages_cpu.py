"""CPU (`-m "not gpu"`): the stage checker of the fp16 scans (tests/scan_stage_ref.py) on its own.

  - vq_debug_scan_row_of maps (stream, local) one-to-one onto the padded rows, for every key layout;
  - soundness: the numpy emulation of a scan passes the checker on every input class the GPU tests use, i.e. the
    reference alone stays inside E = eps_unit(dim) max|row| |q| (printed: the worst error / E per class);
  - non-vacuity: each planted scan defect is caught, one at a time, by the assertion that is there for it.
"""
import numpy as np
import pytest

import scan_stage_ref as ref


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from video_quierer_amd import _lib
    return _lib.load()


def table_for(lib, layout, n):
    return ref.row_table(lib, layout, ref.pad_rows(layout, n) // ref.STREAM_ROWS)


@pytest.mark.parametrize("layout", [1, 2, 3])
@pytest.mark.parametrize("ranges", [1, 2, 5])
def test_row_of_is_a_bijection_onto_the_padded_rows(lib, layout, ranges):
    rows_per_range = {1: 1024, 2: 2048, 3: 128}[layout]
    n_pad = ranges * rows_per_range
    t = ref.row_table(lib, layout, n_pad // ref.STREAM_ROWS)
    assert t.shape == (n_pad // 128, 128)
    assert np.array_equal(np.sort(t.reshape(-1)), np.arange(n_pad))
    # a stream never leaves its range (the ragged mask and the rescans rely on it)
    assert np.array_equal(t.min(1) // rows_per_range, t.max(1) // rows_per_range)
    assert lib.vq_debug_scan_row_of(0, 0, 0) == -1 and lib.vq_debug_scan_row_of(4, 0, 0) == -1
    assert lib.vq_debug_scan_row_of(layout, 0, 128) == -1 and lib.vq_debug_scan_row_of(layout, -1, 0) == -1


def test_eps_unit_is_the_sum_of_its_four_terms():
    # the two figures the derivation's comment quotes
    assert abs(ref.eps_unit(512) - 1.07e-3) < 0.01e-3 and abs(ref.eps_unit(4096) - 1.5e-3) < 0.02e-3
    assert ref.eps_unit(64) < ref.eps_unit(128) < ref.eps_unit(1024)


# (dim, layout, n): every layout at a ragged size; dim 64 is where the bound has least room (its accumulation term is smallest)
SOUND_SHAPES = [(64, 1, 1024 + 129), (192, 1, 129), (128, 2, 2048 + 65), (512, 2, 65), (1024, 2, 300), (256, 3, 6 * 128 + 1),
                (512, 3, 129), (768, 3, 127)]


@pytest.mark.parametrize("name", ref.INPUT_CLASSES)
def test_the_emulated_scan_is_sound_on_every_input_class(lib, name):
    worst = 0.0
    for dim, layout, n in SOUND_SHAPES:
        rng = np.random.default_rng([11, dim, layout])
        rows, qs = ref.input_class(name, rng, n, 6, dim)
        t = table_for(lib, layout, n)
        keys = ref.emulate_keys(rows, qs, t)
        r = ref.check_keys(keys, rows, qs, t)
        print(f"emulation {name} dim={dim} layout={layout} n={n}: keys {r:.4g}")
        worst = max(worst, r)
        if layout == 3:
            labels = np.sort(rng.integers(0, 9, n)).astype(np.int64)
            labels = np.unique(labels, return_inverse=True)[1]
            G = int(labels.max()) + 1
            g = ref.check_group_best(ref.emulate_group_best(rows, qs, labels, G), rows, qs, labels, G)
            allowed = np.arange(G) % 2 == 0
            ga = ref.check_group_best(ref.emulate_group_best(rows, qs, labels, G, allowed), rows, qs, labels, G, allowed)
            km = ref.emulate_keys(rows, qs, t, allowed[labels], ref.stream_labels(labels))
            m = ref.check_keys(km, rows, qs, t, allowed[labels])
            print(f"emulation {name} dim={dim} layout=3 n={n}: group max {g:.4g}, masked group max {ga:.4g}, masked keys {m:.4g}")
            worst = max(worst, g, ga, m)
    print(f"emulation {name}: worst error / E = {worst:.4g}")
    assert worst <= 1.0


# ---- non-vacuity: one planted defect at a time ----
DIM, N, A, B = 128, 3 * 128 + 1, 5, 9           # rows A and B share stream 0; the last stream holds one row


@pytest.fixture(scope="module")
def planted(lib):
    rng = np.random.default_rng(5)
    rows = ref.gaussian_unit(rng, N, DIM)
    rows[B] = ref.unit(rows[A] + 0.1 * rng.standard_normal(DIM).astype(np.float32) / np.sqrt(DIM))
    qs = ref.gaussian_unit(rng, 3, DIM)
    qs[0] = rows[A]                                  # query 0: row A scores 1, row B ~0.995, every other row ~0.1
    t = table_for(lib, 3, N)
    labels = np.minimum(np.arange(N) // 50, 6).astype(np.int64)      # runs of 50 rows: A and B in group 0
    keys = ref.emulate_keys(rows, qs, t)
    ref.check_keys(keys, rows, qs, t)                # the undamaged scan passes
    return rows, qs, t, labels, keys


def test_defect_row_dropped_from_a_fold(planted):
    rows, qs, t, _, _ = planted
    with pytest.raises(ref.StageError, match=f"row {A} was not emitted"):
        ref.check_keys(ref.emulate_keys(rows, qs, t, drop=(0, A)), rows, qs, t)


def test_defect_local_index_off_by_one(planted):
    rows, qs, t, _, keys = planted
    bad = keys.copy()
    assert bad[0, 0, 0] & 127 == A
    bad[0, 0, 0] ^= 1
    with pytest.raises(ref.StageError, match=f"names row {A ^ 1} whose exact"):
        ref.check_keys(bad, rows, qs, t)


def test_defect_k_slice_missing_from_one_row(planted):
    rows, qs, t, _, _ = planted
    with pytest.raises(ref.StageError, match=f"names row {A} whose exact"):
        ref.check_keys(ref.emulate_keys(rows, qs, t, skip_slice=(A, 32)), rows, qs, t)


def test_defect_row_past_the_end_emitted(planted):
    rows, qs, t, _, _ = planted
    with pytest.raises(ref.StageError, match="stream 3: 2 keys name a row, the stream holds 1"):
        ref.check_keys(ref.emulate_keys(rows, qs, t, n_scan=N + 1), rows, qs, t)


def test_defect_same_row_as_both_keys(planted):
    rows, qs, t, _, keys = planted
    bad = keys.copy()
    bad[1, 2, 1] = bad[1, 2, 0]
    with pytest.raises(ref.StageError, match="query 1 stream 2: both keys name row"):
        ref.check_keys(bad, rows, qs, t)


def test_defect_second_key_replaced_by_the_third_best(planted):
    rows, qs, t, _, keys = planted
    bad = keys.copy()
    bad[0, 0, 1] = ref.emulate_keys(rows, qs, t, third=True)[0, 0, 2]
    with pytest.raises(ref.StageError, match=f"row {B} was not emitted"):
        ref.check_keys(bad, rows, qs, t)


def test_defect_label_run_truncated_by_one_row(planted):
    rows, qs, _, labels, _ = planted
    G = int(labels.max()) + 1
    ref.check_group_best(ref.emulate_group_best(rows, qs, labels, G), rows, qs, labels, G)
    # the run of group 0 loses row A; (row B alone would still be within E of it for query 0 only if 1 - 0.995 <= E: it is not)
    with pytest.raises(ref.StageError, match="query 0 group 0"):
        ref.check_group_best(ref.emulate_group_best(rows, qs, labels, G, truncate_row=A), rows, qs, labels, G)


def test_defect_disallowed_row_emitted_by_the_masked_scan(planted):
    rows, qs, t, labels, _ = planted
    allowed = (labels % 2 == 1)                      # group 0 (rows A, B) is disallowed
    sl = ref.stream_labels(labels)
    ref.check_keys(ref.emulate_keys(rows, qs, t, allowed, sl), rows, qs, t, allowed)
    leaky = allowed.copy()
    leaky[A] = True
    with pytest.raises(ref.StageError, match=f"names row {A}, which is past n = {N} or not allowed"):
        ref.check_keys(ref.emulate_keys(rows, qs, t, leaky, sl), rows, qs, t, allowed)
    # and a group that must read "none" but does not, or the reverse
    G = int(labels.max()) + 1
    ga = np.arange(G) % 2 == 1
    best = ref.emulate_group_best(rows, qs, labels, G, ga)
    ref.check_group_best(best, rows, qs, labels, G, ga)
    best[0, 0] = 1.0
    with pytest.raises(ref.StageError, match="query 0 group 0: reads 1.0"):
        ref.check_group_best(best, rows, qs, labels, G, ga)
