"""det_expf and det_logf on the MI355X (link.probe_detmath) against the oracle's array probes, bit for bit, on the sets the CPU
accuracy test holds to float64 (tests/test_detmath_accuracy.py; tests/detmath_sets.py) and on the arguments no sweep holds:
NaNs of both kinds and signs, infinities, zeros, denormals, FLT_MIN, FLT_MAX, the exponential's cut-offs with their
neighbours and negative arguments to the logarithm.  The restatements of every search mode take the oracle's probes for the
device's functions on the strength of this."""
import numpy as np
import pytest

from ataxxzero_amd import link
from oracle import oracle_lib as orc
from tests import detmath_sets as ds

pytestmark = pytest.mark.gpu


def _same_bits(kind, x, ref):
    assert x.dtype == np.float32 and len(x) <= 1 << 24
    got = link.probe_detmath(kind, x)
    want = ref(x).view(np.uint32)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(hex(int(x.view(np.uint32)[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]
    return got.view(np.float32)


def test_specials_bit_for_bit():
    x = ds.specials()
    e = _same_bits(0, x, orc.expf_n)
    l = _same_bits(1, x, orc.logf_n)
    # neither function ever returns a NaN or an infinity, whatever it is given; a NaN is below every cut-off
    assert np.isfinite(e).all() and np.isfinite(l).all()
    nan = np.isnan(x)
    assert nan.sum() == 8 and (e[nan] == 0.0).all() and (l[nan] == np.float32(-87.33654475)).all()
    assert (l[x < np.float32(1.17549435e-38)] == np.float32(-87.33654475)).all()
    assert (e[x == 0.0] == 1.0).all() and (x == 0.0).sum() == 2


@pytest.mark.parametrize("name", sorted(ds.logf_runs()))
def test_logf_sets_bit_for_bit(name):
    _same_bits(1, ds.logf_runs()[name], orc.logf_n)


def test_logf_near_one_bit_for_bit():
    _same_bits(1, ds.logf_near_one(), orc.logf_n)


@pytest.mark.parametrize("name", sorted(ds.expf_runs()))
def test_expf_sets_bit_for_bit(name):
    _same_bits(0, ds.expf_runs()[name], orc.expf_n)


def test_the_gumbel_grid_bit_for_bit():
    """both logarithms of gumbel_noise over every u it can draw"""
    u = ds.gumbel_grid()
    inner = _same_bits(1, u, orc.logf_n)
    _same_bits(1, -inner, orc.logf_n)
