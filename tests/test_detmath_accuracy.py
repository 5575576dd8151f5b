"""The oracle's deterministic logarithm and exponential (oracle/detmath.h) against float64 log and exp: the error in units in
the last place, monotonicity, the exact points, and the Gumbel draw over every argument it can get.  Measured over the whole
domains (too long for the suite): logf 0.827 ulp at 0x3fb4f239 over all positive normal floats, expf 1.010 ulp at 0xc0bc17a1
over all floats in [-87, 88], both non-decreasing; the bounds below leave room only for an ulp defined differently at a
binade's edge.  The device is held to these bits by tests/test_gpu_detmath_edges.py."""
import numpy as np

from oracle import oracle_lib as orc
from tests import detmath_sets as ds
from tests.detmath_sets import EXPF_ULP, LOGF_ULP

F32 = np.float32


def test_logf_against_float64():
    worst = 0.0
    for name, x in ds.logf_runs().items():
        got = orc.logf_n(x)
        ref = np.log(x.astype(np.float64))
        nz = ref != 0.0
        assert (got[~nz] == 0.0).all(), name                   # log(1) is 0 exactly
        err = ds.ulp_error(got[nz], ref[nz])
        i = int(np.argmax(err))
        print("logf %-14s %9d points, worst %.4f ulp at 0x%08x" % (name, len(x), err[i], x[nz].view(np.uint32)[i]))
        assert err[i] <= LOGF_ULP, (name, err[i], hex(x[nz].view(np.uint32)[i]))
        assert (np.diff(got) >= 0).all(), name
        worst = max(worst, err[i])
    assert worst > 0.8      # (the worst point of the whole domain is in the sets)


def test_logf_is_relatively_accurate_around_one():
    """log x -> 0 at 1: an absolute tolerance says nothing there.  0.85 ulp of the result is 0.85 * 2^-23 of it at the most."""
    x = ds.logf_near_one()
    assert len(x) > 20000 and x[0] == F32(1.0 - 2.0 ** -10) and x[-1] == F32(1.0 + 2.0 ** -10)
    got, ref = orc.logf_n(x).astype(np.float64), np.log(x.astype(np.float64))
    nz = ref != 0.0
    assert (got[~nz] == 0.0).all() and (~nz).sum() == 1
    rel = np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])
    print("logf near 1: worst relative error %.3e" % rel.max())
    assert rel.max() <= LOGF_ULP * 2.0 ** -23
    assert (np.diff(got) >= 0).all()


def test_expf_against_float64():
    worst = 0.0
    for name, x in ds.expf_runs().items():
        got = orc.expf_n(x)
        inside = (x >= F32(-87.0)) & (x <= F32(88.0))
        ref = np.exp(x[inside].astype(np.float64))
        err = ds.ulp_error(got[inside], ref)
        i = int(np.argmax(err))
        print("expf %-16s %9d points, worst %.4f ulp at 0x%08x" % (name, len(x), err[i], x[inside].view(np.uint32)[i]))
        assert err[i] <= EXPF_ULP, (name, err[i], hex(x[inside].view(np.uint32)[i]))
        # outside: 0 below -87 and exp(88) above 88, by design
        assert (got[x < F32(-87.0)] == 0.0).all() and (got[x > F32(88.0)] == orc.expf_n(np.array([88.0], F32))[0]).all()
        assert (np.diff(got) >= 0).all(), name
        worst = max(worst, err[i])
    assert worst > 1.0
    assert (orc.expf_n(np.array([0.0, -0.0], F32)) == 1.0).all()
    assert np.isfinite(orc.expf_n(np.array([88.0], F32))[0])


def test_the_gumbel_grid_is_finite_and_monotone():
    u = ds.gumbel_grid()
    inner = orc.logf_n(u)
    assert (inner < 0).all() and (np.diff(inner) >= 0).all()
    g = -orc.logf_n(-inner)
    assert np.isfinite(g).all() and (np.diff(g) >= 0).all()
    print("gumbel grid: g in [%.4f, %.4f]" % (g[0], g[-1]))
    assert -2.8117 < g[0] < -2.8115 and 16.6354 < g[-1] < 16.6356
    # the inner logarithm within the bound as well (u covers (0, 1) on an even grid)
    err = ds.ulp_error(inner, np.log(u.astype(np.float64)))
    assert err.max() <= LOGF_ULP


def test_the_array_probes_equal_the_scalar_ones():
    x = np.concatenate([ds.specials(), ds.bits([ds.LOGF_WORST, ds.EXPF_WORST])])
    for arr, one in ((orc.expf_n, orc.lib().orc_probe_expf), (orc.logf_n, orc.lib().orc_probe_logf)):
        want = np.array([F32(one(float(v))) for v in x], dtype=F32)     # (a NaN's payload may change on the way: values)
        got = arr(x)
        assert (np.isnan(got) == np.isnan(want)).all() and (got[~np.isnan(got)] == want[~np.isnan(want)]).all()
