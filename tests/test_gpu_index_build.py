"""Index build on device (Engine.index_build / index_save, rvcx.infer.index.build_index) against the fp64 toy
builder and the file format of oracle/ivf.py, and the pipeline driven by an index built here
(rvc/train/process/extract_index.py:37-70). The assignment rule and its derived tolerance are those of
tests/test_gpu_kmeans.py."""
import numpy as np
import pytest
import torch

from conftest import golden
from kmeans_ref import _clustered, case1, check_assign, sqdist64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ix_engine():
    from rvcx.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _oracle_rows(n, nlist, seed):
    """The initial rows oracle.ivf.build_ivfflat draws."""
    return np.random.Generator(np.random.PCG64(seed)).choice(n, nlist, replace=False)


def _saved(eng):
    from oracle import ivf

    b = eng.index_save()
    return b, ivf.read_ivfflat(b)


@pytest.mark.parametrize("n,d,nlist,seed,niter", [(300, 768, 7, 13, 3), (1037, 256, 12, 12, 4)])
def test_lloyd_trajectory_matches_fp64_oracle(ix_engine, n, d, nlist, seed, niter):
    """No list is ever empty and every point is decided by >= 20 tol in every iteration, so the device build must
    land on the oracle's lists exactly and on its centroids within one fp32 ulp."""
    from oracle import ivf

    x = _clustered(n, d, seed)
    ref = ivf.build_ivfflat(x, nlist, iters=niter, seed=seed)
    info = ix_engine.index_build(x, nlist, niter=niter, init_rows=_oracle_rows(n, nlist, seed))
    assert info == {"d": d, "ntotal": n, "nlist": nlist, "nprobe": 1}
    _, got = _saved(ix_engine)
    for l in range(nlist):
        np.testing.assert_array_equal(got.list_ids[l], ref.list_ids[l])
        np.testing.assert_array_equal(got.list_vecs[l], ref.list_vecs[l])
    cent = ix_engine.host(ix_engine.index_centroids())
    np.testing.assert_array_equal(cent, got.centroids)
    ulp = np.spacing(np.abs(ref.centroids))
    err = np.abs(cent.astype(np.float64) - ref.centroids.astype(np.float64))
    print(f"max centroid error {float((err / ulp).max()):.2f} ulp")
    assert (err <= ulp).all()


def test_save_and_reload_round_trip(ix_engine):
    from oracle import ivf
    from rvcx import _lib
    from rvcx.engine import Engine
    from rvcx.infer.index import IndexIVFFlat

    x = _clustered(1037, 256, 12)
    ix_engine.index_build(x, 12, niter=4, init_rows=_oracle_rows(1037, 12, 12))
    h1 = IndexIVFFlat.from_engine(ix_engine)
    b, parsed = _saved(ix_engine)
    assert ivf.write_ivfflat(parsed) == b
    assert _lib.index_parse(b) == {"d": 256, "ntotal": 1037, "nlist": 12, "nprobe": 1}
    q = _clustered(200, 256, 3)
    D1, I1 = h1.search(q, 8)
    r1 = h1.reconstruct_n(0, h1.ntotal)
    np.testing.assert_array_equal(r1, x)
    e2 = Engine(0)
    try:
        h2 = IndexIVFFlat(e2, data=b)
        D2, I2 = h2.search(q, 8)
        np.testing.assert_array_equal(I2, I1)
        np.testing.assert_array_equal(D2, D1)
        np.testing.assert_array_equal(h2.reconstruct_n(0, h2.ntotal), r1)
        assert e2.index_save() == b
    finally:
        e2.close()


def test_loaded_files_save_back_byte_for_byte(ix_engine):
    from oracle import ivf

    # "sprs": the empty-list index of test_gpu_index.py::test_empty_lists_sparse_file
    x = _clustered(40, 64, 5, ncl=2)
    idx = ivf.build_ivfflat(x, nlist=16, nprobe=2)
    idx.list_vecs[3] = idx.list_vecs[3][:0]
    idx.list_ids[3] = idx.list_ids[3][:0]
    keep = np.concatenate(idx.list_ids)
    remap = {int(i): j for j, i in enumerate(np.sort(keep))}
    idx.list_ids = [np.array([remap[int(i)] for i in ids], dtype=np.int64) for ids in idx.list_ids]
    sparse = ivf.write_ivfflat(idx, sparse=True)
    assert b"sprs" in sparse  # 15 of 16 lists are non-empty: the writer's own choice would be "full"
    ix_engine.index_load(sparse)
    assert ix_engine.index_save() == sparse
    # "full"
    x = _clustered(300, 256, 6)
    full = ivf.write_ivfflat(ivf.build_ivfflat(x, nlist=5, nprobe=3), sparse=False)
    assert b"full" in full
    ix_engine.index_load(full)
    assert ix_engine.index_save() == full


def test_empty_list_split(ix_engine):
    """The plain Lloyd step leaves one of 20 lists empty from iteration 1 on; the oracle keeps that list's stale
    centroid, the build splits the largest list into it, so its fp64 k-means objective must be strictly lower."""
    from oracle import ivf

    x, _ = case1()
    n, nlist = len(x), 20
    ref = ivf.build_ivfflat(x, nlist, iters=3, seed=11)
    assert min(len(i) for i in ref.list_ids) == 0
    rows = _oracle_rows(n, nlist, 11)
    ix_engine.index_build(x, nlist, niter=3, init_rows=rows)
    b1, got = _saved(ix_engine)
    ids = np.concatenate(got.list_ids)
    np.testing.assert_array_equal(np.sort(ids), np.arange(n))
    list_of_row = np.empty(n, np.int64)
    for l, li in enumerate(got.list_ids):
        assert (np.diff(li) > 0).all()
        list_of_row[li] = l
    np.testing.assert_array_equal(ix_engine.host(ix_engine.index_reconstruct_n(0, n)), x)
    D, _, _, _ = check_assign(x, got.centroids, list_of_row)
    objective = D[np.arange(n), list_of_row].sum()
    ref_of_row = np.empty(n, np.int64)
    for l, li in enumerate(ref.list_ids):
        ref_of_row[li] = l
    ref_objective = sqdist64(x, ref.centroids)[np.arange(n), ref_of_row].sum()
    print(f"objective {objective:.6e} vs oracle {ref_objective:.6e}; smallest list {min(map(len, got.list_ids))}")
    assert objective < ref_objective
    ix_engine.index_build(x, nlist, niter=3, init_rows=rows)
    assert ix_engine.index_save() == b1


def test_seeded_init_is_reproducible_and_valid(ix_engine):
    """init_rows None: the rows come from the seed; two builds agree, another seed gives another index."""
    x = _clustered(1037, 256, 12)
    ix_engine.index_build(x, 12, niter=2, seed=5)
    b1 = ix_engine.index_save()
    ix_engine.index_build(x, 12, niter=2, seed=5)
    assert ix_engine.index_save() == b1
    ix_engine.index_build(x, 12, niter=2, seed=6)
    assert ix_engine.index_save() != b1
    np.testing.assert_array_equal(ix_engine.host(ix_engine.index_reconstruct_n(0, 1037)), x)


def test_build_index_end_to_end_toy(ix_engine, tmp_path):
    from rvcx.infer.index import build_index, plan_index, read_index

    x = _clustered(600, 768, 14)
    plan = plan_index(600, reduce_above=500, reduce_to=64)
    assert plan[0] is True
    index = build_index(ix_engine, x, seed=3, reduce_above=500, reduce_to=64)
    assert (index.ntotal, index.nlist, index.nprobe, index.d) == (64, plan[1], 1, 768)
    path = tmp_path / "added.index"
    index.write(str(path))
    back = read_index(str(path), ix_engine)
    assert (back.ntotal, back.nlist, back.nprobe, back.d) == (64, plan[1], 1, 768)
    # the stored vectors are the reduction's centres: each within the data's bounding box, none repeated
    v = back.reconstruct_n(0, 64)
    assert np.isfinite(v).all() and len(np.unique(v, axis=0)) == 64
    assert (v >= x.min(0) - 1e-3).all() and (v <= x.max(0) + 1e-3).all()


def test_pipeline_uses_a_built_index(engine, synth_w, hubert_w, rmvpe_w, tmp_path):
    """The recipe of test_gpu_index.py::test_pipeline_with_index_matches_oracle with the index built on device."""
    from oracle import hubert as ohubert
    from oracle import ivf
    from oracle.metrics import spectrogram_correlation
    from rvcx import synthetic
    from rvcx.config import HUBERT_BASE
    from rvcx.infer import Config, HubertModel, PipelineMLX, RMVPE0Predictor, Synthesizer
    from rvcx.infer.index import IndexIVFFlat

    from pipeline_ref import NoiseRecorder, oracle_pipeline

    train = synthetic.speech_like(16000 * 4, seed=31).astype(np.float32)
    with torch.no_grad():
        feats = ohubert.hubert_forward(hubert_w, HUBERT_BASE, torch.from_numpy(train).view(1, -1), "v2")[0].numpy()
    engine.index_build(feats, 6, niter=8, init_rows=_oracle_rows(len(feats), 6, 0))
    path = tmp_path / "added_IVF6_Flat_nprobe_1_v2.index"
    IndexIVFFlat.from_engine(engine).write(str(path))
    engine.index_unload()

    g = golden("pipeline_2p5s.npz")
    noise = NoiseRecorder(44)
    orc = oracle_pipeline(synth_w, hubert_w, rmvpe_w, noise)
    ref = orc.pipeline(0, g["audio"].copy(), protect=0.33, index=ivf.read_ivfflat(path.read_bytes()), index_rate=0.75)
    ez, es = noise.cat()
    hub, rm, net_g = HubertModel(engine), RMVPE0Predictor(engine), Synthesizer(engine)
    pipe = PipelineMLX(48000, Config(), hub, rm)
    out = pipe.pipeline(hub, net_g, 0, g["audio"], 0, "rmvpe", str(path), 0.75, True, 1.0, "v2", 0.33, False, 1.0,
                        False, 155.0, eps_z=ez, eps_src=es)
    assert out.shape == ref.shape
    corr = spectrogram_correlation(out, ref)
    print(f"spectrogram correlation {corr:.6f}")
    assert corr > 0.99


def test_errors(ix_engine):
    from rvcx._lib import RvcxError
    from rvcx.engine import Engine

    x = _clustered(64, 256, 1)
    with pytest.raises(RvcxError) as e:
        ix_engine.index_build(x, 65)
    assert e.value.code == -1
    with pytest.raises(RvcxError) as e:
        ix_engine.index_build(x, 3, init_rows=[4, 9, 4])
    assert e.value.code == -1
    with pytest.raises(RvcxError) as e:
        ix_engine.index_build(x, 3, init_rows=[4, 9, 64])
    assert e.value.code == -1
    with pytest.raises(RvcxError) as e:
        ix_engine.index_build(x, 3, niter=-1)
    assert e.value.code == -1
    e2 = Engine(0)
    try:
        with pytest.raises(RvcxError) as e:
            e2.index_save()
        assert e.value.code == -5
        # a failed build leaves the loaded index alone
        e2.index_build(x, 4, niter=1, seed=1)
        before = e2.index_save()
        with pytest.raises(RvcxError):
            e2.index_build(x, 100)
        assert e2.index_save() == before
    finally:
        e2.close()
