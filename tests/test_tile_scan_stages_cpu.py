"""CPU (`-m "not gpu"`): the stage checkers of the streamed 256 x 256 tile scans (tests/tile_stage_ref.py) on their own.

  - the restated layout-2 geometry is the library's (vq_debug_scan_row_of);
  - soundness: the numpy emulation of each tile scan passes its checker on every input class at dims 256, 512 and 768, i.e.
    the reference alone stays inside E (printed: the worst error / E per class);
  - the thresholds of every shared-footage case the GPU test runs satisfy the two conditions the test relies on;
  - non-vacuity: each planted defect of the mainloop, of a fold's mask or of a list is caught, one at a time, by the assertion
    that is there for it.
"""
import numpy as np
import pytest

import scan_stage_ref as ref
import tile_stage_ref as tile

DIMS = (256, 512, 768)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from video_quierer_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("streams", [16, 48])
def test_the_restated_geometry_is_the_librarys(lib, streams):
    assert np.array_equal(tile.table2(streams), ref.row_table(lib, 2, streams))


def class_inputs(name, rng, n, nq, dim, stored_queries=False):
    """stored_queries: the "queries" are stored rows (library neighbours): qnorm has no meaning, a second unnormalised seed stands in"""
    if stored_queries and name == "qnorm":
        return ref.unnormalised_rows(np.random.default_rng([13, dim, 2]), n, dim), None
    return ref.input_class(name, rng, n, nq, dim)


def run_labels(n, run=37):
    return (np.arange(n) // run).astype(np.int64)


# ---------------------------------------------------------------- soundness
@pytest.mark.parametrize("name", ref.INPUT_CLASSES)
def test_the_emulated_neighbour_scan_is_sound_on_every_input_class(name):
    worst = 0.0
    n = 300                                          # two streamed tiles, the second ragged; a resident tile with pad rows
    table = tile.table2(16)
    for dim in DIMS:
        rows, _ = class_inputs(name, np.random.default_rng([13, dim]), n, 1, dim, stored_queries=True)
        asked = np.arange(n)
        for exclude, tags in ((0, np.arange(n)), (1, run_labels(n))):
            keys = tile.emulate_neighbor_keys(rows, asked, tags)
            r = tile.check_keys(keys, rows, rows[asked], table, tile.allowed_from_tags(tags[asked], tags))
            print(f"emulation neighbours {name} dim={dim} n={n} exclude={exclude}: keys {r:.4g}")
            worst = max(worst, r)
    print(f"emulation neighbours {name}: worst error / E = {worst:.4g}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", ref.INPUT_CLASSES)
def test_the_emulated_label_scan_is_sound_on_every_input_class(name):
    worst = 0.0
    for dim in DIMS:
        for n, P in ((130, 300), (5, 2), (3, 2049)):             # ragged tiles; a range of two prompts; a second range of one
            rows, prompts = ref.input_class(name, np.random.default_rng([15, dim, P]), n, P, dim)        # qnorm: the prompts' norms
            r = tile.check_label_parts(tile.emulate_label_parts(rows, prompts), n, rows, prompts)
            print(f"emulation label {name} dim={dim} n={n} P={P}: keys {r:.4g}")
            worst = max(worst, r)
    print(f"emulation label {name}: worst error / E = {worst:.4g}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", ref.INPUT_CLASSES)
def test_the_emulated_match_scan_is_sound_on_every_input_class(name):
    worst = 0.0
    for dim in DIMS:
        rows, qs, max_dist = tile.match_inputs(name, dim, 70, 300)
        assert tile.threshold_conditions(ref.exact_scores(rows, qs), max_dist) == (True, True)
        bits, filed, info = tile.emulate_match(rows, qs, max_dist)
        assert len(filed) >= 1
        r = tile.check_match_bits(bits, filed, info, rows, qs, max_dist)
        print(f"emulation match {name} dim={dim} m=70 n=300: {len(filed)} filed, farthest at {r:.4g} of the band")
        worst = max(worst, r)
    print(f"emulation match {name}: worst |s - T| / band = {worst:.4g}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", ref.INPUT_CLASSES)
def test_the_emulated_group_max_is_sound_at_the_tile_scans_dims(name):
    worst = 0.0
    for dim in DIMS:
        rows, qs = ref.input_class(name, np.random.default_rng([17, dim]), 300, 20, dim)
        labels = run_labels(300)
        G = int(labels.max()) + 1
        allowed = np.arange(G) % 3 != 1
        worst = max(worst, tile.check_group_best(tile.emulate_group_best(rows, qs, labels, G), rows, qs, labels, G),
                    tile.check_group_best(tile.emulate_group_best(rows, qs, labels, G, allowed), rows, qs, labels, G, allowed))
    print(f"emulation group max {name}: worst error / E = {worst:.4g}")
    assert worst <= 1.0


@pytest.mark.parametrize("cls,dim,m,n", tile.MATCH_CASES)
def test_every_gpu_match_case_has_a_threshold_that_meets_both_conditions(cls, dim, m, n):
    rows, qs, max_dist = tile.match_inputs(cls, dim, m, n)
    near, clear = tile.threshold_conditions(ref.exact_scores(rows, qs), max_dist)
    assert near, "no pair lies within MATCH_SLACK / 2 of T"
    assert clear, "a score lies within 2^-21 of T"


# ---------------------------------------------------------------- non-vacuity: neighbours
DIM, N, A, B = 256, 600, 300, 301              # three streamed tiles; rows A and B sit in tile 1, half 0, and share a stream


@pytest.fixture(scope="module")
def nb():
    rng = np.random.default_rng(7)
    rows = ref.gaussian_unit(rng, N, DIM)
    rows[B] = ref.unit(rows[A] + 0.1 * rng.standard_normal(DIM).astype(np.float32) / np.sqrt(DIM))
    assert tile.stream_of(np.array([A]))[0] == tile.stream_of(np.array([B]))[0]
    asked = np.arange(N)
    labels = run_labels(N, 50)                       # A and B in one group
    table = tile.table2(16)
    for tags in (np.arange(N), labels):              # the undamaged scans pass
        tile.check_keys(tile.emulate_neighbor_keys(rows, asked, tags), rows, rows, table, tile.allowed_from_tags(tags, tags))
    return rows, asked, labels, table


def nb_check(nb, exclude=0, **plant):
    rows, asked, labels, table = nb
    tags = labels if exclude else np.arange(N)
    return tile.check_keys(tile.emulate_neighbor_keys(rows, asked, tags, **plant), rows, rows, table, tile.allowed_from_tags(tags, tags))


def test_defect_stale_half_tile_in_the_neighbour_scan(nb):
    with pytest.raises(ref.StageError, match=r"names row \d+ whose exact score is"):
        nb_check(nb, plant=("stale", 1, 0, 64))


def test_defect_accumulators_not_cleared_in_the_neighbour_scan(nb):
    with pytest.raises(ref.StageError, match=r"names row \d+ whose exact score is"):
        nb_check(nb, plant=("noclear", 1, 0, 0))


def test_defect_quadrant_folded_under_the_previous_tile_in_the_neighbour_scan(nb):
    # the keys of tile t's quadrant name the rows 256 earlier: a row named twice, named with another row's score, or the asked row itself
    caught = r"both keys name row|names row \d+ whose exact score is|names row \d+, which is past n = 600 or not allowed"
    with pytest.raises(ref.StageError, match=caught):
        nb_check(nb, plant=("fold", 1, 0, 0))
    with pytest.raises(ref.StageError, match=caught):
        nb_check(nb, plant=("fold", 2, 1, 1))


def test_defect_first_pad_row_not_masked_in_the_neighbour_scan():
    rows = ref.gaussian_unit(np.random.default_rng(9), 2, DIM)
    asked, tags, table = np.arange(2), np.arange(2), tile.table2(16)
    tile.check_keys(tile.emulate_neighbor_keys(rows, asked, tags), rows, rows, table, tile.allowed_from_tags(tags, tags))
    with pytest.raises(ref.StageError, match="query 0 stream 0: 2 keys name a row, the stream holds 1"):
        tile.check_keys(tile.emulate_neighbor_keys(rows, asked, tags, n_scan=3), rows, rows, table, tile.allowed_from_tags(tags, tags))


def test_defect_struck_pair_emitted_by_the_neighbour_scan(nb):
    with pytest.raises(ref.StageError, match=f"query {A} stream .* names row {A}, which is past n = {N} or not allowed"):
        nb_check(nb, exclude=0, leak=(A, A))         # the row itself
    with pytest.raises(ref.StageError, match=f"query {A} stream .* names row {B}, which is past n = {N} or not allowed"):
        nb_check(nb, exclude=1, leak=(A, B))         # a row of its own group


# ---------------------------------------------------------------- non-vacuity: label
LN, LP = 130, 600


@pytest.fixture(scope="module")
def lb():
    rng = np.random.default_rng(11)
    rows = ref.gaussian_unit(rng, LN, DIM)
    prompts = ref.unit(-0.5 * rows[0][None, :] + ref.gaussian_unit(rng, LP, DIM))      # row 0: every score negative
    assert (ref.exact_scores(prompts, rows[:1]) < -0.1).all()
    tile.check_label_parts(tile.emulate_label_parts(rows, prompts), LN, rows, prompts)
    return rows, prompts


def lb_check(lb, **plant):
    rows, prompts = lb
    return tile.check_label_parts(tile.emulate_label_parts(rows, prompts, **plant), LN, rows, prompts)


def test_defect_stale_half_tile_in_the_label_scan(lb):
    with pytest.raises(ref.StageError, match=r"K[12] .* names prompt \d+ whose exact score is|exceeds the floor"):
        lb_check(lb, plant=("stale", 1, 1, 128))


def test_defect_accumulators_not_cleared_in_the_label_scan(lb):
    with pytest.raises(ref.StageError, match=r"K[12] .* names prompt \d+ whose exact score is|exceeds the floor"):
        lb_check(lb, plant=("noclear", 1, 1, 1))


def test_defect_quadrant_folded_under_the_previous_tile_in_the_label_scan(lb):
    with pytest.raises(ref.StageError, match=r"both keys name prompt|K[12] .* names prompt \d+ whose exact score is"):
        lb_check(lb, plant=("fold", 1, 0, 1))


def test_defect_first_pad_prompt_not_masked_in_the_label_scan(lb):
    with pytest.raises(ref.StageError, match=f"row 0 range 0: J1 {LP} J2 .*: outside the range's prompts 0 .. {LP - 1}"):
        lb_check(lb, p_scan=LP + 1)


def test_defect_label_floor_replaced_by_the_fourth_best(lb):
    rows, prompts = lb
    top = -np.sort(-ref.exact_scores(prompts, rows), axis=1)
    assert ((top[:, 2] - top[:, 3]) > 3 * ref.bound(rows, prompts).max()).any()
    with pytest.raises(ref.StageError, match="is neither J1 nor J2, its exact score .* exceeds the floor"):
        lb_check(lb, floor_rank=4)


# ---------------------------------------------------------------- non-vacuity: match
@pytest.fixture(scope="module")
def mt():
    rows, qs, max_dist = tile.match_inputs("gaussian", DIM, 70, 300)
    bits, filed, info = tile.emulate_match(rows, qs, max_dist)
    tile.check_match_bits(bits, filed, info, rows, qs, max_dist)
    dist = np.abs(ref.exact_scores(rows, qs) - tile.match_threshold(max_dist))
    return rows, qs, max_dist, bits, filed, info, dist


def test_defect_sure_bit_flipped_off_the_band(mt):
    rows, qs, max_dist, bits, filed, info, dist = mt
    q, r = np.unravel_index(dist.argmax(), dist.shape)
    bad = bits.copy()
    bad[q, r >> 5] ^= np.uint32(1 << (r & 31))
    with pytest.raises(ref.StageError, match=f"query {q} row {r}: the bit is"):
        tile.check_match_bits(bad, filed, info, rows, qs, max_dist)


def test_defect_filed_pair_dropped(mt):
    rows, qs, max_dist, bits, filed, info, dist = mt
    q, r = np.unravel_index(dist.argmin(), dist.shape)
    keep = filed != ((np.uint64(q) << np.uint64(32)) | np.uint64(r))
    assert keep.sum() == len(filed) - 1
    with pytest.raises(ref.StageError, match=f"query {q} row {r} is not filed"):
        tile.check_match_bits(bits, filed[keep], dict(info, cursor=len(filed) - 1), rows, qs, max_dist)


def test_defect_out_of_band_pair_filed_or_filed_twice(mt):
    rows, qs, max_dist, bits, filed, info, dist = mt
    q, r = np.unravel_index(dist.argmax(), dist.shape)
    more = np.append(filed, (np.uint64(q) << np.uint64(32)) | np.uint64(r))
    with pytest.raises(ref.StageError, match=f"query {q} row {r} is filed, its exact score .* outside the band"):
        tile.check_match_bits(bits, more, dict(info, cursor=len(more)), rows, qs, max_dist)
    twice = np.append(filed, filed[:1])
    with pytest.raises(ref.StageError, match="is filed 2 times"):
        tile.check_match_bits(bits, twice, dict(info, cursor=len(twice)), rows, qs, max_dist)
    with pytest.raises(ref.StageError, match="exceeds the capacity"):
        tile.check_match_bits(bits, filed, dict(info, cap=len(filed) - 1), rows, qs, max_dist)
    with pytest.raises(ref.StageError, match="the call is flagged 2"):
        tile.check_match_bits(bits, filed, dict(info, flag=2), rows, qs, max_dist)


def test_defect_bit_set_behind_the_last_row(mt):
    rows, qs, max_dist, bits, filed, info, dist = mt
    bad = bits.copy()
    bad[3, 300 >> 5] |= np.uint32(1 << (300 & 31))
    with pytest.raises(ref.StageError, match="query 3: the bit of row 300 is set, the index holds 300 rows"):
        tile.check_match_bits(bad, filed, info, rows, qs, max_dist)


def test_defect_stale_half_tile_in_the_match_scan():
    rng = np.random.default_rng(19)
    rows, qs = ref.gaussian_unit(rng, 600, DIM), ref.gaussian_unit(rng, 70, DIM)
    noise = rng.standard_normal(DIM).astype(np.float32) / np.sqrt(DIM)
    rows[300] = ref.unit(qs[0] + 0.1 * noise)        # a clear hit (0.995) in streamed tile 1, half 0
    rows[10] = ref.unit(qs[0] + 0.48 * noise)        # the pair the threshold sits beside (0.9)
    max_dist = tile.choose_max_dist(ref.exact_scores(rows, qs), skip=1)
    assert 0.85 < tile.match_threshold(max_dist) < 0.95
    tile.check_match_bits(*tile.emulate_match(rows, qs, max_dist), rows, qs, max_dist)
    with pytest.raises(ref.StageError, match="query 0 row 300: the bit is 0"):
        tile.check_match_bits(*tile.emulate_match(rows, qs, max_dist, plant=("stale", 1, 0, 0)), rows, qs, max_dist)
