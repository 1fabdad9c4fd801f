"""CPU: the host half of the float64 statistics path.  `measurements.stats_from_order` turns what boa_group_stats_f64 returns
(count, sum, centred sum of squares, min, max, six order statistics) into the reference's eight statistics; fed from `np.sort`
it must reproduce numpy: order statistics, min and max under `==`, mean and std to rtol 1e-12 (the summation order of the
inputs handed in here is numpy's own)."""
import math

import numpy as np
import pytest

RANK_QS = (0.25, 0.5, 0.75)


def _order(sorted_x):
    n = len(sorted_x)
    return [sorted_x[f((n - 1) * q)] for q in RANK_QS for f in (math.floor, math.ceil)]


def _host_stats(x):
    from boa_hip import measurements as M
    x = np.asarray(x, dtype=np.float64)
    s = np.sort(x)
    mean = x.sum() / len(x)
    return M.stats_from_order(len(x), x.sum(), ((x - mean) ** 2).sum(), s[0], s[-1], _order(s))


def _check(x):
    x = np.asarray(x, dtype=np.float64)
    st = _host_stats(x)
    assert st["n"] == len(x)
    assert st["median"] == np.median(x), (len(x), st["median"], np.median(x))
    assert st["p25"] == np.percentile(x, 25), (len(x), st["p25"], np.percentile(x, 25))
    assert st["p75"] == np.percentile(x, 75), (len(x), st["p75"], np.percentile(x, 75))
    assert st["min"] == np.min(x) and st["max"] == np.max(x)
    assert np.isclose(st["mean"], np.mean(x), rtol=1e-12, atol=0)
    if np.std(x) > 0:
        assert np.isclose(st["std"], np.std(x), rtol=1e-12, atol=0)
    else:
        assert st["std"] == 0.0


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 4 * 37 + 1, 4 * 37 + 2, 1000])
def test_random_samples_equal_numpy(n):
    rng = np.random.default_rng(n)
    for scale in (1.0, 350.0, 1e-3):
        _check(rng.normal(40.0, 120.0, size=n) * scale)
        _check(rng.uniform(-1024.0, 3071.0, size=n) * scale)


@pytest.mark.parametrize("n", [1, 2, 5, 8, 150])
def test_all_equal_and_signed_zeros(n):
    _check(np.full(n, -1024.0))
    _check(np.full(n, 0.1))
    z = np.zeros(n)
    z[::2] = -0.0
    _check(z)
    _check(np.concatenate([z, [-1.5, 2.5]]))


@pytest.mark.parametrize("n", [2, 3, 4, 6, 9, 150, 151])
def test_neighbouring_doubles(n):
    """Samples that differ in the last mantissa bit only: the interpolation must not move off numpy's result."""
    for start in (1.0, -37.3, 1e30, 5e-324, -200.0):
        x = np.empty(n)
        x[0] = start
        for i in range(1, n):
            x[i] = np.nextafter(x[i - 1], np.inf)
        np.random.default_rng(n).shuffle(x)
        _check(x)
        _check(np.repeat(x, 2))


def test_empty_group_is_none():
    from boa_hip import measurements as M
    assert M.stats_from_order(0, 0.0, 0.0, 0.0, 0.0, [0.0] * 6) is None


def test_non_finite_values_are_refused_by_name(monkeypatch):
    from boa_hip import measurements as M
    monkeypatch.delenv("BOA_STATS_FLOAT", raising=False)
    good = np.array([[[-1024.5, 30.25]]])
    vals, is_float = M.ct_for_stats(good, "/data/case7/image.nii.gz")
    assert is_float and vals.dtype == np.float64 and np.array_equal(vals, good)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match=r"/data/case7/image\.nii\.gz.*non-finite"):
            M.ct_for_stats(np.array([[[0.5, bad]]]), "/data/case7/image.nii.gz")


def test_dispatch_follows_require_int16_exact(monkeypatch):
    """int16-exact values keep the int16 path; BOA_STATS_FLOAT=1 forces the float path for them."""
    from boa_hip import measurements as M
    monkeypatch.delenv("BOA_STATS_FLOAT", raising=False)
    exact = np.array([[[-1024.0, 3071.0]]])
    vals, is_float = M.ct_for_stats(exact)
    assert not is_float and vals.dtype == np.int16
    for other in (np.array([[[40000, 1]]], dtype=np.int32), np.array([[[0.5, 1.0]]], dtype=np.float32)):
        vals, is_float = M.ct_for_stats(other)
        assert is_float and vals.dtype == np.float64 and np.array_equal(vals, other)
    monkeypatch.setenv("BOA_STATS_FLOAT", "1")
    vals, is_float = M.ct_for_stats(exact.astype(np.int16))
    assert is_float and vals.dtype == np.float64 and np.array_equal(vals, exact)
