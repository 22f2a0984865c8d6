"""oracle/fftw_standin.cc, the FFTW stand-in the reference binary is built against, checked on its own: the three r2r transforms against
numpy.fft.rfft, numpy.fft.irfft x n and the closed-form REDFT10 sum in float64, within 1e-12 of the input's 2-norm."""
import ctypes
import os

import numpy as np
import pytest

from oracle import oracle as orc

R2HC, HC2R, REDFT10 = 0, 1, 5
LENGTHS = [32, 256, 512, 1024, 4096, 101]   # the FFT sizes of the front end and trapdct's context length


@pytest.fixture(scope="module")
def L():
    orc.build()
    path = os.path.join(os.path.dirname(orc.__file__), "_build", "libfftw_standin.so")
    if not os.path.exists(path):
        orc.build(force=True)
    lib = ctypes.CDLL(path)
    lib.fftw_malloc.restype = ctypes.c_void_p
    lib.fftw_malloc.argtypes = [ctypes.c_size_t]
    lib.fftw_free.argtypes = [ctypes.c_void_p]
    lib.fftw_plan_r2r_1d.restype = ctypes.c_void_p
    lib.fftw_plan_r2r_1d.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint]
    lib.fftw_execute.argtypes = [ctypes.c_void_p]
    lib.fftw_destroy_plan.argtypes = [ctypes.c_void_p]
    return lib


def _run(L, kind, x, in_place=False):
    """Plans first and fills the input afterwards, as the reference does; fftw_malloc'ed buffers."""
    n = x.size
    pin = L.fftw_malloc(8 * n)
    pout = pin if in_place else L.fftw_malloc(8 * n)
    a = np.ctypeslib.as_array(ctypes.cast(pin, ctypes.POINTER(ctypes.c_double)), shape=(n,))
    b = np.ctypeslib.as_array(ctypes.cast(pout, ctypes.POINTER(ctypes.c_double)), shape=(n,))
    plan = L.fftw_plan_r2r_1d(n, pin, pout, kind, 0)
    assert plan
    a[:] = x
    L.fftw_execute(plan)
    first = b.copy()
    if not in_place:
        assert np.array_equal(a, x)        # the input survives (the reference reads HC2R's input again)
        L.fftw_execute(plan)               # a plan is executed once per frame
        assert np.array_equal(b, first)
    L.fftw_destroy_plan(plan)
    L.fftw_free(pin)
    if not in_place:
        L.fftw_free(pout)
    return first


def _halfcomplex(X, n):
    hc = np.zeros(n)
    hc[:n // 2 + 1] = X.real
    k = np.arange(1, (n + 1) // 2)
    hc[n - k] = X.imag[k]
    return hc


@pytest.mark.parametrize("n", LENGTHS)
def test_r2hc(L, n):
    x = np.random.default_rng(n).standard_normal(n)
    want = _halfcomplex(np.fft.rfft(x), n)
    assert np.abs(_run(L, R2HC, x) - want).max() <= 1e-12 * np.linalg.norm(x)
    assert np.array_equal(_run(L, R2HC, x, in_place=True), _run(L, R2HC, x))


@pytest.mark.parametrize("n", LENGTHS)
def test_hc2r(L, n):
    rng = np.random.default_rng(100 + n)
    X = rng.standard_normal(n // 2 + 1) + 1j * rng.standard_normal(n // 2 + 1)
    X[0] = X[0].real
    if n % 2 == 0:
        X[-1] = X[-1].real
    hc = _halfcomplex(X, n)
    want = np.fft.irfft(X, n) * n
    assert np.abs(_run(L, HC2R, hc) - want).max() <= 1e-12 * np.linalg.norm(hc)
    # and the pair is n times the identity
    x = rng.standard_normal(n)
    assert np.abs(_run(L, HC2R, _run(L, R2HC, x)) - n * x).max() <= 1e-12 * n * np.linalg.norm(x)


@pytest.mark.parametrize("n", LENGTHS)
def test_redft10(L, n):
    x = np.random.default_rng(200 + n).standard_normal(n)
    j, k = np.arange(n), np.arange(n)[:, None]
    # pi (j + 1/2) k / n with the integer (2 j + 1) k reduced modulo the period 4 n first: the float64 argument stays below 2 pi
    want = 2.0 * (np.cos(np.pi * (((2 * j + 1) * k) % (4 * n)) / (2 * n)) * x).sum(axis=1)
    assert np.abs(_run(L, REDFT10, x) - want).max() <= 1e-12 * np.linalg.norm(x)


def test_only_the_three_kinds_and_positive_lengths(L):
    buf = (ctypes.c_double * 8)()
    for kind in (2, 3, 4, 6, 7, -1):
        assert not L.fftw_plan_r2r_1d(8, buf, buf, kind, 0)
    assert not L.fftw_plan_r2r_1d(0, buf, buf, R2HC, 0)
    one = _run(L, R2HC, np.array([3.5]))
    assert one.tolist() == [3.5]
