"""CPU: the oracles against the golden vectors captured from the real
transformers CLIP model and the real reference hnsw.py (tests/golden/make_golden.py)."""
import hashlib
import random

import numpy as np

from conftest import INDEX_SEED, synth_frames
from oracle import clip_vit_oracle, hnsw_oracle, knn_oracle


def test_synthetic_inputs_match_capture(golden_encoder, b32_weights):
    frames = synth_frames(64)
    assert hashlib.sha256(frames.tobytes()).hexdigest() == str(golden_encoder["frames_sha256"])
    h = hashlib.sha256()
    for k in sorted(b32_weights):
        h.update(b32_weights[k].tobytes())
    assert h.hexdigest() == str(golden_encoder["weights_sha256"])


def test_encoder_oracle_matches_transformers(golden_encoder, b32_weights):
    emb = clip_vit_oracle.encode_frames(synth_frames(64), b32_weights, batch_size=32)
    assert emb.dtype == np.float32 and emb.shape == (64, 512)
    assert np.abs(emb - golden_encoder["embeddings"]).max() <= 1e-5
    assert np.allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-6)


def test_encoder_oracle_edge_cases(b32_weights):
    assert clip_vit_oracle.encode_frames(np.zeros((0, 224, 224, 3), np.uint8), b32_weights).shape == (0,)
    f = synth_frames(3, seed=5)
    # batch slicing does not change results; PIL path (no channel swap) == pre-swapped ndarray path
    a = clip_vit_oracle.encode_frames(f, b32_weights, batch_size=2)
    b = clip_vit_oracle.encode_frames(f, b32_weights, batch_size=3)
    assert np.abs(a - b).max() < 1e-6
    c = clip_vit_oracle.encode_frames(f[..., ::-1], b32_weights, swap_rb=False)
    assert np.abs(a - c).max() < 1e-6


def test_extract_from_video_frames_shape(b32_weights):
    frames = synth_frames(5, seed=11)
    fd = [{"frame": f, "timestamp": i * 0.5, "frame_number": i} for i, f in enumerate(frames)]
    out = clip_vit_oracle.extract_from_video_frames(fd, b32_weights, batch_size=2)
    assert [o["frame_number"] for o in out] == list(range(5))
    assert all(o["features"].shape == (512,) and "feature_extraction_time" in o for o in out)
    assert "features" not in fd[0]          # copies, not in-place


def _build_hnsw(n=1000):
    vecs = np.random.default_rng(INDEX_SEED).standard_normal((n, 512)).astype(np.float32)
    random.seed(0)
    h = hnsw_oracle.HnswOracle(512)
    h.add_batch(list(vecs), list(range(n)))
    return h


def test_hnsw_restatement_builds_the_reference_graph(golden_knn):
    h = _build_hnsw()
    assert np.array_equal(np.array(h.level, dtype=np.int32), golden_knn["levels"])
    assert h.ids[h.entry] == int(golden_knn["entry_point"])
    assert np.array_equal(np.stack(h.vec), golden_knn["stored"])
    edges = sorted((lv, a, b) for a in range(len(h.ids)) for lv, s in enumerate(h.adj[a]) for b in s)
    assert np.array_equal(np.array(edges, dtype=np.int32), golden_knn["edges"])


def test_hnsw_restatement_search_lists(golden_knn, golden_encoder):
    h = _build_hnsw()
    for ef in (50, 1000):
        h.ef_search = ef
        for k in (5, 10):
            res = [h.search(q, k) for q in golden_encoder["embeddings"]]
            ids = np.array([[r["id"] for r in rr] for rr in res], dtype=np.int32)
            d = np.array([[r["distance"] for r in rr] for rr in res], dtype=np.float32)
            sc = np.array([[r["score"] for r in rr] for rr in res], dtype=np.float32)
            assert np.array_equal(ids, golden_knn[f"ids_ef{ef}_k{k}"])
            assert np.array_equal(d, golden_knn[f"dist_ef{ef}_k{k}"])
            assert np.array_equal(sc, golden_knn[f"score_ef{ef}_k{k}"])
    assert type(res[0][0]["distance"]) is np.float32


def test_exact_oracle_equals_exhaustive_reference(golden_knn, golden_encoder):
    q = np.stack([e / np.linalg.norm(e) for e in golden_encoder["embeddings"]]).astype(np.float32)
    for k in (5, 10):
        ids, d = knn_oracle.topk(golden_knn["stored"], q, k)
        assert np.array_equal(ids, golden_knn[f"ids_ef1000_k{k}"])            # identical id lists
        assert np.abs(d - golden_knn[f"dist_ef1000_k{k}"]).max() <= 2e-7      # fixed-order dot vs BLAS order
    # the reference at its default ef_search=50 is approximate: report its recall vs exact
    ids10, _ = knn_oracle.topk(golden_knn["stored"], q, 10)
    rec = np.mean([len(set(a) & set(b)) / 10 for a, b in zip(golden_knn["ids_ef50_k10"], ids10)])
    assert 0.5 < rec < 1.0


def test_exact_oracle_equals_the_exhaustive_reference_at_10k_and_100k_rows():
    """tests/golden/knn_ref_<n>.npz (the REAL OptimizedHNSWIndex over 10k / 100k seeded rows under the caller's string ids):
    the inputs regenerate from the seed to the rows the reference stored, the reference at ef_search = N returned the
    exact answer for every query, and the C oracle + the (distance, id) tie rule reproduces its lists."""
    import os
    from conftest import GOLDEN, KNN_BIG_DUPES, knn_big_ids, knn_big_inputs
    for n in (10_000, 100_000):
        path = os.path.join(GOLDEN, f"knn_ref_{n}.npz")
        if not os.path.exists(path):
            continue
        ref = np.load(path)
        rows, qs = knn_big_inputs(n)
        ids = knn_big_ids(n)
        stored = np.stack([v / np.linalg.norm(v) for v in rows]).astype(np.float32)            # hnsw.py:157
        assert hashlib.sha256(stored.tobytes()).hexdigest() == str(ref["stored_sha256"])
        assert int(ref["exhaustive_lists_identical_k10"]) == 64 and int(ref["exhaustive_lists_identical_k20"]) == 64
        unit_q = np.stack([q / np.linalg.norm(q) for q in qs]).astype(np.float32)              # hnsw.py:499
        orow, od = knn_oracle.topk(stored, unit_q, 20)
        row_of = {s: r for r, s in enumerate(ids)}
        want = np.array([[row_of[s] for _, s in sorted((od[j, i], ids[orow[j, i]]) for i in range(20))] for j in range(64)])
        for k in (10, 20):
            assert np.array_equal(want[:, :k], ref[f"rows_ef{n}_k{k}"])
            assert np.abs(od[:, :k] - ref[f"dist_ef{n}_k{k}"]).max() <= 3e-7
            assert 0.0 < float(ref[f"default_ef_recall_k{k}"]) < 1.0       # the default walk (ef_search = 50) is approximate
        # the planted duplicate frames: id order, not row order
        assert list(ref[f"rows_ef{n}_k10"][0, :2]) == [10, 2] and list(ref[f"rows_ef{n}_k10"][1, :3]) == [100, 20, 3]
        assert KNN_BIG_DUPES[0] == (2, 10)


def test_exact_oracle_edge_cases():
    rng = np.random.default_rng(3)
    x = knn_oracle.normalize_rows(rng.standard_normal((7, 16)).astype(np.float32))
    assert np.allclose(np.linalg.norm(x, axis=1), 1, atol=1e-6)
    ids, d = knn_oracle.topk(x, x[:2], 10)                  # k > n: padded with -1 / +inf
    assert (ids[:, 7:] == -1).all() and np.isinf(d[:, 7:]).all()
    assert ids[0, 0] == 0 and ids[1, 0] == 1
    dup = np.concatenate([x, x[:3]])                        # exact duplicates: ties broken by smaller row
    ids, d = knn_oracle.topk(dup, x[:1], 2)
    assert list(ids[0]) == [0, 7] and d[0, 0] == d[0, 1]
    bf = hnsw_oracle.brute_force(dup, list(range(10)), x[0], 2)
    assert [r["id"] for r in bf] == [0, 7]


def test_encoder_oracle_matches_transformers_vit_l14_336():
    """configs[4] geometry (577 tokens, patch 14, hidden 1024, 24 layers, 16 heads, projection 768)."""
    import os
    from conftest import GOLDEN, FRAME_SEED
    from video_quierer_amd.weights import VIT_L_14_336, seeded_weights
    g = np.load(os.path.join(GOLDEN, "encoder_l14_336_seed1234.npz"))
    frames = np.random.default_rng(FRAME_SEED).integers(0, 255, (32, 336, 336, 3), dtype=np.uint8)
    assert hashlib.sha256(frames.tobytes()).hexdigest() == str(g["frames_sha256"])
    cfg = VIT_L_14_336
    # the fixture holds 32 frames (one bench-sized batch for the GPU test); the CPU suite re-runs the restatement on the first 2
    emb = clip_vit_oracle.encode_frames(frames[:2], seeded_weights(cfg, 1234), patch=cfg.patch_size, heads=cfg.heads,
                                        layers=cfg.layers, batch_size=2)
    assert g["embeddings"].shape == (32, 768) and emb.shape == (2, 768) and np.abs(emb - g["embeddings"][:2]).max() <= 1e-5


def test_text_oracle_matches_transformers():
    import os
    from conftest import GOLDEN
    from video_quierer_amd.weights import TEXT_B_32, seeded_text_weights
    g = np.load(os.path.join(GOLDEN, "text_b32_seed1234.npz"))
    W = seeded_text_weights(TEXT_B_32, 1234)
    emb = clip_vit_oracle.encode_token_ids(g["input_ids"], W)
    assert np.abs(emb - g["embeddings"]).max() <= 1e-5
    pad = np.full((g["input_ids"].shape[0], 77), 49407, dtype=np.int64)
    pad[:, :g["input_ids"].shape[1]] = g["input_ids"]
    assert np.array_equal(clip_vit_oracle.encode_token_ids(pad, W), emb)     # eos padding never reaches the pooled row


def test_text_oracle_matches_transformers_l14_width():
    """The ViT-L/14 text tower (768 wide, 12 heads, projection 768): the restatement against transformers' output."""
    import os
    from conftest import GOLDEN
    from video_quierer_amd.weights import TEXT_L_14, seeded_text_weights
    g = np.load(os.path.join(GOLDEN, "text_l14_seed1234.npz"))
    W = seeded_text_weights(TEXT_L_14, 1234)
    emb = clip_vit_oracle.encode_token_ids(g["input_ids"], W, heads=TEXT_L_14.heads, layers=TEXT_L_14.layers)
    assert emb.shape == (16, 768) and np.abs(emb - g["embeddings"]).max() <= 1e-5


# ------------------------------------------------------------------ resize in front of the encoder (§8f #3)
def _resample_oracle_output(h, w, kind, mode):
    from conftest import resample_input
    from oracle import resample_oracle
    img = resample_input(h, w, kind)
    return resample_oracle.stretch_to_square(img) if mode == "stretch" else resample_oracle.clip_processor_u8(img)


def test_resample_oracle_matches_pillow_golden(golden_resample):
    from conftest import RESAMPLE_CASES
    for i, (name, h, w, kind, mode) in enumerate(RESAMPLE_CASES):
        out = _resample_oracle_output(h, w, kind, mode)
        assert out.shape == (224, 224, 3) and out.dtype == np.uint8
        assert hashlib.sha256(out.tobytes()).hexdigest() == str(golden_resample[f"sha256_{name}"]), name
        if i < 2:
            assert np.array_equal(out, golden_resample[f"out_{name}"])


def test_resample_oracle_matches_pillow_live():
    """Where Pillow is importable (the build container), the restatement equals it on ragged sizes and both filters."""
    Image = __import__("pytest").importorskip("PIL.Image")
    from oracle import resample_oracle as ro
    rng = np.random.default_rng(77)
    for (h, w, ow, oh) in [(37, 53, 224, 224), (300, 400, 201, 640), (2, 3, 7, 5), (1, 1, 4, 4), (500, 224, 224, 100), (64, 64, 64, 17)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for filt, pil_filt in ((ro.BILINEAR, Image.BILINEAR), (ro.BICUBIC, Image.BICUBIC)):
            assert np.array_equal(ro.resize_u8(img, ow, oh, filt), np.asarray(Image.fromarray(img).resize((ow, oh), pil_filt))), (h, w, ow, oh, filt)


def test_quality_oracle_properties():
    """Parity unpinned (OpenCV absent): pin the restatement's own invariants instead."""
    from oracle import quality_oracle as q
    flat = np.full((32, 48, 3), 120, np.uint8)
    assert q.quality(flat) == (120.0, 0.0) and q.is_low_quality(flat)              # no texture -> "blurry"
    assert q.is_low_quality(np.full((8, 8, 3), 10, np.uint8)) and q.is_low_quality(np.full((8, 8, 3), 250, np.uint8))
    noise = np.random.default_rng(3).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    assert not q.is_low_quality(noise)
    g = q.bgr_to_gray(np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8))
    assert g.tolist() == [[255, 0, 29, 150, 76]]                                      # the familiar 0.114/0.587/0.299 greys
    chk = np.indices((6, 6)).sum(0) % 2 * 255
    L = q.laplacian_f64(chk.astype(np.uint8))
    assert np.array_equal(np.abs(L), np.full((6, 6), 1020.0))                         # checkerboard: |L| = 4*255 everywhere (reflect-101 keeps parity)


def test_cv_resize_oracle_properties():
    """Parity unpinned (OpenCV absent): invariants of the INTER_LINEAR restatement."""
    from oracle import cv_resize_oracle as cv, resample_oracle as ro
    rng = np.random.default_rng(21)
    assert np.unique(cv.resize_linear_u8(np.full((37, 53, 3), 137, np.uint8), 224, 224)).tolist() == [137]   # weights sum to one
    img = rng.integers(0, 256, (100, 80, 3), dtype=np.uint8)
    assert np.array_equal(cv.resize_linear_u8(img, 80, 100), img)                                            # equal size = copy
    big = rng.integers(0, 256, (448, 448, 3), dtype=np.uint8).astype(np.int64)
    half = cv.resize_linear_u8(big.astype(np.uint8), 224, 224)
    assert np.array_equal(half, (big[0::2, 0::2] + big[0::2, 1::2] + big[1::2, 0::2] + big[1::2, 1::2] + 2) >> 2)
    up = cv.resize_linear_u8(img, 224, 224)                 # up-scaling needs no antialiasing: Pillow's bilinear is the same map
    assert np.abs(up.astype(int) - ro.resize_u8(img, 224, 224, ro.BILINEAR)).max() <= 1
    s, w0, w1 = cv.linear_coeffs(1920, 224, True)
    assert np.all(w0 + w1 == 2048) and s.min() >= 0 and s.max() <= 1919 and np.all(np.diff(s) > 0)


# ---- persistence / live-index fixtures written by the REAL reference classes (make_golden.py interop) ----
def _golden(name):
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)


def _interop_vectors():
    rng = np.random.default_rng(11)
    vecs = (rng.standard_normal((50, 64)) * 2.5).astype(np.float32)
    ids = [f"video{i // 25}_{i % 25}" for i in range(50)]
    qs = rng.standard_normal((8, 64)).astype(np.float32)
    return vecs, ids, qs


def test_reference_written_index_file_equals_exact_oracle():
    """The pickle the real HNSWIndex.save wrote: its keys (hnsw.py:311-324), its sidecar, its rows (= v/|v|, :157)
    and the result lists the real class returned from it = the exact oracle's answer in (distance, id) order."""
    import pickle
    with open(_golden("ref_index_50.pkl"), "rb") as f:
        raw = f.read()
    assert hashlib.sha256(raw).hexdigest() == open(_golden("ref_index_50.pkl.sha256")).read().strip()
    s = pickle.loads(raw)
    assert sorted(s) == sorted(["dimension", "M", "max_M", "ef_construction", "ef_search", "level_generation_factor",
                                "data", "levels", "graph", "entry_point", "element_count"])
    vecs, ids, qs = _interop_vectors()
    stored = np.stack([s["data"][i] for i in ids])
    assert np.array_equal(stored, np.stack([v / np.linalg.norm(v) for v in vecs]).astype(np.float32))
    gold = np.load(_golden("ref_index_50_results.npz"))
    uq = np.stack([q / np.linalg.norm(q) for q in qs]).astype(np.float32)
    rows, dist = knn_oracle.topk(stored, uq, 5)
    assert [[ids[r] for r in rr] for rr in rows] == [list(r) for r in gold["ids"]]
    assert np.abs(dist - gold["dist"]).max() <= 3e-7


def test_reference_class_loads_a_build_written_index_file():
    """The file the GPU build's HNSWIndex.save wrote (tests/golden/build_index_50.pkl, produced on the GPU box by
    tests/test_gpu_parity.py::test_index_save_writes_the_reference_layout) loads with the REAL class — same rows, same ids,
    same parameters.  It carries no navigable graph: searching it with the reference needs a re-add.
    What the real class saw is the fixture build_index_50_refload.npz (make_golden.py refload), keyed by the SHA-256 of the
    file it loaded; the load (hnsw.py:341-380), the flat-graph walk and the re-add are restated here on the committed file."""
    import pickle
    with open(_golden("build_index_50.pkl"), "rb") as f:
        raw = f.read()
    seen = np.load(_golden("build_index_50_refload.npz"))
    assert hashlib.sha256(raw).hexdigest() == str(seen["sha256"]) == open(_golden("build_index_50.pkl.sha256")).read().strip()
    vecs, ids, qs = _interop_vectors()
    unit = np.stack([v / np.linalg.norm(v) for v in vecs]).astype(np.float32)
    # the real class after load(): parameters, rows, a walk that sees the entry point only, the lists after a re-add
    assert int(seen["dimension"]) == 64 and int(seen["size"]) == 50 and str(seen["entry_point"]) in ids
    assert np.array_equal(seen["data"], unit)
    assert len(seen["flat_search_ids"]) == 1
    gold = np.load(_golden("ref_index_50_results.npz"))
    assert [list(r) for r in seen["rebuilt_ids"]] == [list(r) for r in gold["ids"]]
    # the same from the committed file: every field load() reads, restored as it restores them
    s = pickle.loads(raw)
    for key in ("dimension", "M", "max_M", "ef_construction", "ef_search", "level_generation_factor", "element_count", "entry_point"):
        assert s[key] == seen["size" if key == "element_count" else key].item(), key
    assert np.array_equal(np.stack([s["data"][i] for i in ids]), seen["data"])
    h = hnsw_oracle.HnswOracle(s["dimension"], M=s["M"], ef_construction=s["ef_construction"], ef_search=s["ef_search"],
                               max_M=s["max_M"], level_generation_factor=s["level_generation_factor"])
    for i, (node, v) in enumerate(s["data"].items()):
        h.ids.append(node)
        h.row_of[node] = i
        h.vec.append(v)
        h.level.append(s["levels"][node])
        h.adj.append([set() for _ in range(s["levels"][node] + 1)])
    for lv, nodes in s["graph"].items():
        for node, nbrs in nodes.items():
            h.adj[h.row_of[node]][int(lv)] = {h.row_of[n] for n in nbrs}
    h.entry = h.row_of[s["entry_point"]]
    assert [r["id"] for r in h.search(qs[0], 5)] == list(seen["flat_search_ids"])
    random.seed(3)
    rebuilt = hnsw_oracle.HnswOracle(64)
    rebuilt.add_batch([s["data"][i] for i in ids], ids)
    res = [rebuilt.search(q, 5) for q in qs]
    assert [[r["id"] for r in rr] for rr in res] == [list(r) for r in seen["rebuilt_ids"]]
    assert np.array_equal(np.array([[r["distance"] for r in rr] for rr in res], dtype=np.float32), seen["rebuilt_dist"])


def test_simple_index_fixture_is_reversed_argsort_of_dots():
    """What the real SimpleVideoIndex returned (simple_index.npz) restated: top-k of E @ (q / (|q| + 1e-10)) by
    np.argsort(sim)[::-1] (video_search_overhaul.py:49-57); exact duplicates come out larger frame id first."""
    gold = np.load(_golden("simple_index.npz"))
    rng = np.random.default_rng(77)
    emb = rng.standard_normal((300, 512)).astype(np.float32)
    emb[:200] /= np.linalg.norm(emb[:200], axis=1, keepdims=True)
    emb[250] = emb[230]
    emb[20] = emb[10]
    for row, qi in enumerate(gold["query_rows"]):
        q = emb[qi] * np.float32(gold["query_scale"])
        sims = emb @ (q / (np.linalg.norm(q) + 1e-10))
        assert list(np.argsort(sims)[::-1][:12]) == list(gold["frame_id_k12"][row])
        assert np.allclose(sims[gold["frame_id_k12"][row]], gold["score_k12"][row], rtol=0, atol=1e-5)
    assert list(gold["frame_id_k5"][4][:2]) == [250, 230]
