"""Pins ctuo_burg_cepstrum() against the reference's own Burg estimator.

src/vdet/Burg.h is FFTW-free: oracle/Makefile builds it into oracle/_ref/libref_burg.so, and tests/golden/make_ref_fixtures.py
recorded its predictor, cepstrum and error on these segments in tests/golden/ref_outputs.npz.
"""
import numpy as np
import pytest

from oracle.oracle import burg_cepstrum
from tests.golden.make_ref_fixtures import BURG_CASES, burg_segments
from tests.util import ref_outputs


@pytest.mark.parametrize("npoints,ncoefs", BURG_CASES)
def test_burg_bit_identical_to_reference_header(npoints, ncoefs):
    z = ref_outputs()
    key = f"burg_{npoints}_{ncoefs}"
    a_ref, c_ref, al_ref = z[key + "_a"], z[key + "_c"], z[key + "_alpha"]
    segs = burg_segments(npoints)
    assert len(segs) == len(al_ref) == 8
    for seg, ar, cr, alr in zip(segs, a_ref, c_ref, al_ref):
        a, c, alpha = burg_cepstrum(seg, ncoefs)
        assert np.array_equal(a, ar) and np.array_equal(c, cr) and alpha == alr
