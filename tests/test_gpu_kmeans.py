"""The k-means kernels of the index build (csrc/kmeans.hip through rvcx_kmeans_assign / rvcx_kmeans_update) against
fp64 numpy.

The assignment tolerance is derived, not measured. The project holds its contractions to 1e-6 of each output's own
sum |x w| (tests/test_gpu_conv_math.py); with 2 sum |x_i c_i| <= |x|^2 + |c|^2 a score |c|^2 - 2 x.c is off by at
most 1e-6 (|x|^2 + 2 |c|^2). A pick can therefore differ from the fp64 argmin only where the fp64 gap between the
best and the chosen centroid is <= tol(q) = 2e-6 (|x_q|^2 + 2 max_l |c_l|^2). A point is *decided* when its fp64
best-to-second gap exceeds tol: decided points must get the fp64 argmin, the rest a centroid within tol of the
minimum, and every case asserts that at least 99 % of its points are decided."""
import numpy as np
import pytest

from kmeans_ref import _clustered, case1, check_assign, sqdist64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def km_engine():
    from rvcx.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def test_assign_ragged_tiles(km_engine):
    """4133 rows (no multiple of the 128-query block), 50 centroids (no multiple of 32: padded columns must score
    +inf). Every point is decided (minimum gap 15.9 tol), so the ids are the fp64 argmin throughout."""
    x, cent = case1()
    a, dist = km_engine.kmeans_assign(x, cent)
    a, dist = km_engine.host(a), km_engine.host(dist)
    D, best, tol, decided = check_assign(x, cent, a, min_decided=1.0)
    np.testing.assert_array_equal(a, best)
    err = np.abs(dist.astype(np.float64) - D[np.arange(len(D)), best])
    print(f"max dist err / tol = {(err / tol).max():.3e}")
    assert (err <= tol).all()


def test_assign_several_centroid_tiles(km_engine):
    """300 centroids: three tiles of 128 with a ragged last one; the centroids are rows of x."""
    x, _ = case1()
    cent = x[np.random.Generator(np.random.PCG64(21)).choice(4133, 300, replace=False)]
    a, _ = km_engine.kmeans_assign(x, cent, want_dist=False)
    check_assign(x, cent, km_engine.host(a))


def test_assign_d256_and_bad_d(km_engine):
    from rvcx._lib import RvcxError

    x = _clustered(1037, 256, 12)
    cent = x[np.random.Generator(np.random.PCG64(12)).choice(1037, 12, replace=False)]
    a, dist = km_engine.kmeans_assign(x, cent)
    a, dist = km_engine.host(a), km_engine.host(dist)
    D, best, tol, _ = check_assign(x, cent, a)
    assert (np.abs(dist.astype(np.float64) - D[np.arange(len(D)), a]) <= tol).all()
    with pytest.raises(RvcxError) as e:
        km_engine.kmeans_assign(x[:, :48], cent[:, :48])
    assert e.value.code == -2  # RVCX_E_SHAPE, before any launch


def test_assign_ties_pick_the_lower_id(km_engine):
    x, cent = case1()
    cent = cent.copy()
    lo, hi = 5, 37
    cent[hi] = cent[lo]
    a = km_engine.host(km_engine.kmeans_assign(x, cent, want_dist=False)[0])
    assert not (a == hi).any()
    # without the duplicate the usual rule holds, and some points do sit on the tied pair
    _, best, _, _ = check_assign(x, np.delete(cent, hi, axis=0), a - (a > hi))
    assert (best == lo).sum() > 0


def test_update_means_sizes_empty_list_and_determinism(km_engine):
    x, cent = case1()
    x64 = x.astype(np.float64)
    a = sqdist64(x, cent).argmin(1).astype(np.int32)
    sizes_ref = np.bincount(a, minlength=50)
    full = np.nonzero(sizes_ref)[0]  # (three stale-centroid Lloyd steps from 50 random rows leave some lists empty)
    assert 30 <= len(full) < 50  # both kinds of list are in the input
    c1, s1 = km_engine.kmeans_update(x, a, cent)
    c1, s1 = km_engine.host(c1), km_engine.host(s1)
    np.testing.assert_array_equal(s1, sizes_ref)
    for l in range(50):
        if sizes_ref[l]:
            want = np.float32(x64[a == l].mean(0))
            assert (np.abs(c1[l].astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all(), l
        else:
            assert c1[l].tobytes() == cent[l].tobytes(), l
    # a list emptied by hand keeps its centroid bit for bit
    src, dst = int(full[0]), int(full[1])
    a2 = a.copy()
    a2[a2 == src] = dst
    c2, s2 = km_engine.kmeans_update(x, a2, cent)
    c2, s2 = km_engine.host(c2), km_engine.host(s2)
    assert s2[src] == 0 and s2[dst] == sizes_ref[src] + sizes_ref[dst]
    assert c2[src].tobytes() == cent[src].tobytes()
    want = np.float32(x64[a2 == dst].mean(0))
    assert (np.abs(c2[dst].astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    # run to run
    c3, s3 = km_engine.kmeans_update(x, a, cent)
    assert km_engine.host(c3).tobytes() == c1.tobytes()
    np.testing.assert_array_equal(km_engine.host(s3), s1)
