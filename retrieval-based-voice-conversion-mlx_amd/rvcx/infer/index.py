"""FAISS-compatible feature index handle on MI355X.

Replaces the reference's use of faiss in the pipeline (rvc/infer/pipeline.py:430-434 and :378-388;
rvc_mlx/infer/pipeline_mlx.py:267-278 and :183-201):

    index = read_index(path, engine)          # faiss.read_index(path)
    big_npy = index.reconstruct_n(0, index.ntotal)
    D, I = index.search(feats, k=8)

The file is parsed by librvcx.so (faiss 1.7.4 IndexIVFFlat layout) and kept in HBM; search and the
retrieval blend run as HIP kernels (csrc/ivf.hip). Outputs are numpy at this API edge, like faiss.
"""
from __future__ import annotations

import numpy as np

from ..engine import Engine


class IndexIVFFlat:
    """Device-resident IndexIVFFlat bound to one Engine (one rvcx context holds one index)."""

    def __init__(self, engine: Engine, path: str = None, data: bytes = None):
        if data is None:
            with open(path, "rb") as f:
                data = f.read()
        engine.index_load(data)
        self._bind(engine, path)

    def _bind(self, engine: Engine, path: str = None):
        self.engine = engine
        self.path = path
        info = engine.index_info()
        if info is None:
            raise RuntimeError("the engine holds no index")
        self.d, self.ntotal, self.nlist = info["d"], info["ntotal"], info["nlist"]
        self._nprobe = info["nprobe"]
        self.is_trained = True

    @classmethod
    def from_engine(cls, engine: Engine) -> "IndexIVFFlat":
        """Wrap the index the engine already holds (built by Engine.index_build or loaded earlier)."""
        self = cls.__new__(cls)
        self._bind(engine)
        return self

    def write(self, path: str):
        """faiss.write_index(index, path) (extract_index.py:70)."""
        self._bound()
        data = self.engine.index_save()
        with open(path, "wb") as f:
            f.write(data)
        self.path = path

    @property
    def nprobe(self) -> int:
        return self._nprobe

    @nprobe.setter
    def nprobe(self, v: int):
        self.engine.index_set_nprobe(int(v))
        self._nprobe = self.engine.index_info()["nprobe"]

    def _bound(self):
        info = self.engine.index_info()
        if info is None or info["ntotal"] != self.ntotal or info["d"] != self.d:
            raise RuntimeError("this index is no longer the one loaded in its engine")

    def search(self, x, k: int):
        """-> (D float32 [n, k], I int64 [n, k]) like faiss Index.search."""
        self._bound()
        d, i = self.engine.index_search(np.ascontiguousarray(x, dtype=np.float32), int(k))
        return self.engine.host(d), self.engine.host(i)

    def reconstruct_n(self, i0: int, ni: int) -> np.ndarray:
        self._bound()
        return self.engine.host(self.engine.index_reconstruct_n(i0, ni))

    def retrieve(self, feats, index_rate: float) -> np.ndarray:
        """Pipeline._retrieve_speaker_embeddings (pipeline.py:378-388) for feats [L, d] (or [1, L, d])."""
        self._bound()
        f = np.asarray(feats, dtype=np.float32)
        out = self.engine.host(self.engine.index_retrieve(f.reshape(-1, f.shape[-1]), index_rate))
        return out.reshape(f.shape)


def read_index(path: str, engine: Engine) -> IndexIVFFlat:
    return IndexIVFFlat(engine, path=path)


# ------------------------------------------------------------------------------------ build
# Replaces rvc/train/process/extract_index.py:29-70 (faiss-cpu + sklearn) with the device k-means of
# csrc/kmeans.hip / index_build.cpp. Unpinned against faiss and sklearn themselves; three documented deviations:
#   * the row shuffle is seeded (PCG64(seed)); the reference's np.random.shuffle is not;
#   * the > 200 000 row reduction (:43-56) runs the same device Lloyd k-means to reduce_to centres in place of
#     sklearn's MiniBatchKMeans(init="random"): full-batch instead of mini-batch updates;
#   * the IVF training picks the donor of an empty list deterministically (index_build.cpp) where faiss draws it.
def plan_index(n_rows: int, algorithm: str = "Auto", reduce_above: int = 200_000, reduce_to: int = 10_000):
    """-> (reduce, n_ivf): whether extract_index.py:43-45 reduces the rows to reduce_to k-means centres first, and
    n_ivf = min(int(16 * sqrt(m)), m // 39) over the m rows that go into the index (:58). Host only."""
    n_rows = int(n_rows)
    reduce = n_rows > reduce_above and algorithm in ("Auto", "KMeans")
    m = int(reduce_to) if reduce else n_rows
    return reduce, min(int(16 * np.sqrt(m)), m // 39)


def load_feature_dir(feature_dir: str) -> np.ndarray:
    """extract_index.py:29-37: the *.npy feature files of a directory, concatenated in sorted name order."""
    import os

    names = sorted(n for n in os.listdir(feature_dir) if n.endswith(".npy"))
    if not names:
        raise FileNotFoundError(f"no .npy feature files in {feature_dir}")
    return np.concatenate([np.load(os.path.join(feature_dir, n)) for n in names], axis=0)


def build_index(engine: Engine, feats, algorithm: str = "Auto", seed: int = 0, niter: int = 10,
                **plan_overrides) -> IndexIVFFlat:
    """extract_index.py:37-68 on device: shuffle, optional k-means reduction, IVF train + add with nprobe 1.
    feats [N, d] fp32 (the concatenated HuBERT features); plan_overrides: reduce_above / reduce_to of plan_index.
    The built index is the engine's loaded index on return."""
    x = np.ascontiguousarray(feats, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError(f"build_index: feats must be [N, d], got {x.shape}")
    reduce, n_ivf = plan_index(x.shape[0], algorithm, **plan_overrides)
    x = x[np.random.Generator(np.random.PCG64(seed)).permutation(x.shape[0])]
    if n_ivf < 1:
        raise ValueError(f"build_index: {x.shape[0]} rows are too few for an IVF index (n_ivf = {n_ivf})")
    xd = engine._dev(x, engine.torch.float32)
    if reduce:
        reduce_to = int(plan_overrides.get("reduce_to", 10_000))
        engine.index_build(xd, reduce_to, niter=niter, nprobe=1, seed=seed)
        xd = engine.index_centroids().clone()
    engine.index_build(xd, n_ivf, niter=niter, nprobe=1, seed=seed)
    return IndexIVFFlat.from_engine(engine)


def build_index_from_dir(engine: Engine, feature_dir: str, algorithm: str = "Auto", seed: int = 0,
                         **kw) -> IndexIVFFlat:
    """extract_index.py:29-68 for a directory of extracted features (the `extracted/` folder of a training run)."""
    return build_index(engine, load_feature_dir(feature_dir), algorithm=algorithm, seed=seed, **kw)
