"""PeriodicMetric on the host: the distance against an independent statement of it, the argument checks, its place among the
built-in metrics, and the periodic C entries' argument validation (which returns before any HIP call).  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import torch_assimilate_amd as mia

MIA_ERR_NULL, MIA_ERR_ARG = -1, -7


def cyclic_dist(g, o, period, groups):
    """Restatement of the spec: per coordinate a = |d| mod L, min(a, L - a) on a cyclic axis, |d| on an open one; the Euclidean
    norm over the coordinates of each radius group."""
    g = np.asarray(g, dtype=np.float64)
    o = np.asarray(o, dtype=np.float64)
    out = np.zeros((max(groups) + 1, o.shape[0]))
    for c, grp in enumerate(groups):
        a = np.abs(o[:, c] - g[c])
        if period[c] > 0:
            a = np.mod(a, period[c])
            a = np.minimum(a, period[c] - a)
        out[grp] += a * a
    return np.sqrt(out)


def check(metric, g, o, period, groups):
    got = np.asarray(metric(g, o))
    want = cyclic_dist(np.asarray(g).reshape(-1)[-np.shape(o)[1]:], o, period, groups)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-9)


def test_ring_1d_and_coordinates_outside_the_period():
    rng = np.random.default_rng(1)
    L = 40.0
    o = rng.uniform(-3 * L, 4 * L, size=(500, 1))
    for g in (0.0, 0.3, 19.99, 39.7, -5.5, 123.25):
        check(mia.PeriodicMetric(L), [g], o, [L], [0])
    d = np.asarray(mia.PeriodicMetric(L)([0.5], np.array([[39.5], [20.5], [80.5]])))
    np.testing.assert_allclose(d[0], [1.0, 20.0, 0.0], atol=1e-12)


def test_channel_2d_one_cyclic_axis():
    rng = np.random.default_rng(2)
    per = [100.0, 0.0]
    o = np.stack([rng.uniform(-50, 250, 400), rng.uniform(0, 30, 400)], axis=1)
    m = mia.PeriodicMetric(per)
    for g in ([1.0, 3.0], [99.0, 15.0], [250.0, 0.0]):
        check(m, g, o, per, [0, 0])
    # None marks an open coordinate as 0 does
    check(mia.PeriodicMetric([100.0, None]), [97.0, 5.0], o, per, [0, 0])


def test_3d_two_radius_groups_and_time_column():
    rng = np.random.default_rng(3)
    per = [60.0, 0.0, 0.0]
    groups = [0, 0, 1]
    m = mia.PeriodicMetric(per, coord_group=groups)
    o = np.stack([rng.uniform(0, 60, 300), rng.uniform(0, 20, 300), rng.uniform(0, 5, 300)], axis=1)
    g = [58.0, 4.0, 2.0]
    check(m, g, o, per, groups)
    # the reference's state rows carry a leading time column: dist_func(grid_ind, obs_grid) ignores it
    check(m, [7.0] + g, o, per, groups)
    assert np.asarray(m([7.0] + g, o)).shape == (2, 300)


def test_scalar_period_applies_to_every_coordinate():
    o = np.array([[9.5, 0.5], [5.0, 5.0]])
    d = np.asarray(mia.PeriodicMetric(10.0)([0.5, 9.5], o))
    np.testing.assert_allclose(d[0], [np.sqrt(2.0), np.sqrt(4.5 ** 2 + 4.5 ** 2)], rtol=1e-12)


@pytest.mark.parametrize("period", [-1.0, float("nan"), float("inf"), [10.0, -2.0], [], [[1.0, 2.0]]])
def test_bad_periods_raise(period):
    with pytest.raises(ValueError):
        mia.PeriodicMetric(period)


def test_period_length_must_match_coordinates():
    with pytest.raises(ValueError):
        mia.PeriodicMetric([10.0, 20.0], coord_group=[0, 0, 0])
    m = mia.PeriodicMetric([10.0, 20.0])
    with pytest.raises(ValueError):
        m([0.0, 0.0, 0.0], np.zeros((4, 3)))
    with pytest.raises(ValueError):
        m.periods(3)


def test_builtin_metric_is_recognised():
    m = mia.PeriodicMetric(40.0)
    assert isinstance(m, mia.EuclideanMetric)
    assert mia.GaspariCohn(4.0, dist_func=m).builtin_metric is m
    assert mia.GaspariCohnInf(4.0, dist_func=m).builtin_metric is m
    assert m.periods(2) == [40.0, 40.0]
    assert mia.EuclideanMetric().periods(2) is None


def test_engine_period_argument_checks():
    from torch_assimilate_amd.engine import _periods
    assert _periods(None, 2) is None
    assert _periods([0.0, None], 2) is None                      # every coordinate open: the plain entries
    assert list(_periods(5.0, 2)) == [5.0, 5.0]
    for bad in ([1.0], [-1.0, 0.0], [float("nan"), 1.0]):
        with pytest.raises(ValueError):
            _periods(bad, 2)


@pytest.fixture(scope="module")
def lib():
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def test_periodic_entries_reject_bad_periods_before_device_work(lib):
    cg = (C.c_int32 * 1)(0)
    rc = (C.c_double * 1)(4.0)
    st = (C.c_int32 * 2)()
    for bad in (-1.0, float("nan"), float("inf")):
        per = (C.c_double * 1)(bad)
        # (null device pointers throughout: a call that got past the check would fail on them -- or touch a device)
        assert lib.mia_letkf_localize_taper_periodic_f64(0, None, 0, 10, None, 10, 1, cg, per, rc, 1, 1e-5, 8,
                                                         None, None, None, None, None, 0, None) == MIA_ERR_ARG
        assert lib.mia_letkf_index_build_periodic_f64(None, 10, 1, cg, per, rc, 1, None, 0, None) == MIA_ERR_ARG
        assert lib.mia_letkf_localize_tiles_periodic_f64(0, None, 0, 10, None, 10, 1, cg, per, rc, 1, 1e-5, 8, 0,
                                                         C.c_void_p(256), 1 << 20, st, None, 0, None) == MIA_ERR_ARG
        assert lib.mia_letkf_sharded_step_periodic_f32(
            C.c_void_p(256), 10, 1, 4, None, None, 10, C.c_void_p(256), None, 1, cg, per, rc, 1, 1e-5, 1.0, 0.0, 0, 8, None, 1,
            0, C.c_void_p(256), C.c_void_p(256), C.c_void_p(256), C.c_void_p(256), 1 << 20, None, None, None, 0) == MIA_ERR_ARG
    # a null period is a null pointer, not an open metric: the plain entries are for that
    assert lib.mia_letkf_index_build_periodic_f64(None, 10, 1, cg, None, rc, 1, None, 0, None) == MIA_ERR_NULL
    assert lib.mia_status_string(MIA_ERR_ARG).startswith(b"invalid argument")


def test_step_args_mirror_has_the_period_field():
    from torch_assimilate_amd import _cabi
    a = _cabi.StepArgs()
    assert list(a.period) == [0.0, 0.0, 0.0]
    assert _cabi.StepArgs.period.offset == C.sizeof(_cabi.StepArgs) - 3 * C.sizeof(C.c_double)
