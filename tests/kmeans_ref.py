"""The fp64 yardstick of the k-means kernels (tests/test_gpu_kmeans.py, whose docstring derives the tolerance) and the
clustered inputs its tests and the index-build tests share."""
import functools

import numpy as np

def _clustered(n, d, seed, ncl=24):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((ncl, d)).astype(np.float32) * 2
    return (centers[rng.integers(0, ncl, n)] + rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)


def sqdist64(x, c):
    """[n, nlist] fp64 squared distances (the expansion in fp64: its own error, ~1e-12, is far below any tol here)."""
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return np.maximum((x64 ** 2).sum(1)[:, None] + (c64 ** 2).sum(1)[None, :] - 2.0 * (x64 @ c64.T), 0.0)


def assign_tol(x, c):
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return 2e-6 * ((x64 ** 2).sum(1) + 2.0 * (c64 ** 2).sum(1).max())


def check_assign(x, cent, got, min_decided=0.99):
    """The rule of the module docstring; returns (fp64 distances, fp64 argmin, tol, decided mask)."""
    D = sqdist64(x, cent)
    tol = assign_tol(x, cent)
    best = D.argmin(1)
    if D.shape[1] > 1:
        two = np.partition(D, 1, axis=1)[:, :2]
        decided = (two[:, 1] - two[:, 0]) > tol
    else:
        decided = np.ones(len(D), bool)
    share = decided.mean()
    print(f"decided {share:.5f} ({(~decided).sum()} undecided of {len(D)})")
    assert share >= min_decided
    got = np.asarray(got)
    assert got.min() >= 0 and got.max() < D.shape[1]
    np.testing.assert_array_equal(got[decided], best[decided])
    rows = np.arange(len(D))
    assert (D[rows, got] - D[rows, best] <= tol).all()
    return D, best, tol, decided


@functools.lru_cache(maxsize=None)
def case1():
    """x [4133, 768] and the 50 centroids of three fp64 Lloyd iterations over it, computed once."""
    from oracle import ivf

    x = _clustered(4133, 768, 11)
    cent = ivf.build_ivfflat(x, 50, iters=3, seed=11).centroids
    return x, cent  # shared: the tests copy before they change either
