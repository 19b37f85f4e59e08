"""Host side of the index build (rvcx.infer.index: plan_index, the feature-directory reader) and the ABI names it
adds. No GPU. The plan restates rvc/train/process/extract_index.py:43-45 and :58."""
import numpy as np

from rvcx.infer.index import load_feature_dir, plan_index


def test_plan_index_matches_extract_index():
    assert plan_index(3000) == (False, 76)
    assert plan_index(250_000) == (True, 256)
    assert plan_index(250_000, "Faiss") == (False, 6410)
    assert plan_index(200_000) == (False, 5128)  # "> 2e5" is strict: the largest unreduced case


def test_plan_index_overrides():
    assert plan_index(600, reduce_above=500, reduce_to=64) == (True, min(int(16 * np.sqrt(64)), 64 // 39))
    assert plan_index(600, "KMeans", reduce_above=600) == (False, 15)


def test_feature_dir_reader_concatenates_in_sorted_name_order(tmp_path):
    rng = np.random.default_rng(0)
    parts = {"10_b.npy": rng.standard_normal((3, 8)).astype(np.float32),
             "0_a.npy": rng.standard_normal((5, 8)).astype(np.float32),
             "2_c.npy": rng.standard_normal((2, 8)).astype(np.float32)}
    for name, a in parts.items():  # written in an order that is not the sorted one
        np.save(tmp_path / name, a, allow_pickle=False)
    (tmp_path / "notes.txt").write_text("not a feature file")
    got = load_feature_dir(str(tmp_path))
    want = np.concatenate([parts[n] for n in sorted(parts)], axis=0)  # "0_a", "10_b", "2_c": string order
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)


def test_lib_lists_the_new_symbols():
    from rvcx import _lib

    for name in ("rvcx_index_default_build_opts", "rvcx_index_build", "rvcx_index_save", "rvcx_index_centroids"):
        assert name in _lib.EXPORTS
    for name in ("rvcx_kmeans_assign", "rvcx_kmeans_update"):
        assert name in _lib.TEST_EXPORTS
    assert set(_lib.EXPORTS + _lib.TEST_EXPORTS) <= set(_lib.exported_symbols())
    o = _lib.IndexBuildOpts()
    assert _lib.load().rvcx_index_default_build_opts(o) == 0
    assert (o.niter, o.nprobe, o.seed, bool(o.init_rows)) == (10, 1, 0, False)
