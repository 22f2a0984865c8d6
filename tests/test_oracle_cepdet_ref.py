"""Pins the oracle's CepstralDetector restatement (ctuo_cepdet_*) against the reference's own header.

src/vdet/CepstralDet.h with Burg.h / Fft.h / Fft.cc / Complex.h is FFTW-free: oracle/Makefile compiles it into
oracle/_ref/libref_cepdet.so, and tests/golden/make_ref_fixtures.py recorded its decisions in tests/golden/ref_outputs.npz.
Decisions must agree frame for frame over whole recordings, across detector restarts and option sets.
"""
import numpy as np
import pytest

from oracle.oracle import CepstralDetector
from tests.golden.make_ref_fixtures import CEPDET_CASES, cepdet_key, frames
from tests.util import ref_outputs, sig


@pytest.mark.parametrize("npoints,hop,ninit,ncoefs,p,q", CEPDET_CASES)
def test_detector_decisions_identical_to_reference_header(npoints, hop, ninit, ncoefs, p, q):
    z = ref_outputs()
    total = ones = 0
    for name in ("CS0", "CS3"):
        fr = frames(sig(name), npoints, hop)
        ref = z[f"{cepdet_key(npoints, hop, ninit, ncoefs, p, q)}_{name}"]
        assert ref.size == fr.shape[0]
        det = CepstralDetector(npoints, ninit, ncoefs, p, q)
        got = np.array([det.process(f) for f in fr], dtype=np.uint8)
        assert np.array_equal(got, ref)
        total += ref.size
        ones += int(ref.sum())
    assert 0 < ones < total  # both classes occur, so the comparison is not vacuous
