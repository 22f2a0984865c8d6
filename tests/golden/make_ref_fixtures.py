#!/usr/bin/env python3
"""Records what the reference's own FFTW-free pieces compute on the inputs of the *_ref tests: tests/golden/ref_outputs.npz.

  make -C oracle ref && python tests/golden/make_ref_fixtures.py

oracle/Makefile's `ref` target compiles src/io/amulaw.h, src/vdet/Burg.h, src/vdet/CepstralDet.h and src/vad/vad.h's
medianFilter of a reference tree (REF=<path>) into oracle/_ref/libref_*.so through the oracle/ref_*_driver.cc shims.  This script
drives those libraries on the same inputs the tests build (tests/util.py's signals and generators, the oracle's rows) and stores
their outputs, so the tests pin the restatements against the reference without the reference tree:
  amulaw_{mu,a}                               the expander's 256-entry tables (int16)
  burg_<npoints>_<ncoefs>_{a,c,alpha}         Burg predictor / cepstrum / error on 8 Hamming-windowed segments of CS3
  cepdet_<case>_<signal>                      CepstralDetector decisions over a whole recording (uint8)
  median_<cri>_<order>_<utt>_{dec,out}        medianFilter decisions and the vectors it delays (float32, as the writer sees them)
  median_identity_{dec,out}                   order 1 on random vectors
  medlist_<order>_<trial>_{frames,rows,n}     the filter driven over a list of files: frame numbers of the rows each file writes
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle.oracle import Oracle  # noqa: E402
from tests.util import sig, synth_utt  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(HERE, "ref_outputs.npz")

BURG_CASES = [(200, 14), (400, 14), (200, 10), (64, 5)]
CEPDET_CASES = [(200, 80, 10, 12, 0.95, 0.99), (400, 160, 10, 12, 0.95, 0.99), (200, 80, 40, 10, 0.8, 0.97), (256, 128, 3, 14, 0.9, 0.95)]
MEDIAN_CRITERIA = ["-vad_cri_mode energy -vad_thr_mode adapt", "-vad_cri_mode energy -vad_thr_mode dyn",
                   "-vad burg -vad_cri_mode cepdist -vad_cepdist_mode lpc -vad_thr_mode adapt"]
MEDIAN_ORDERS = [3, 5, 7]
MEDIAN_BASE = "-fs 8000 -format_in raw -format_out htk -preset mfcc -vad_out_mode vad".split()
LIST_ORDERS = [3, 5]
LIST_TRIALS = 6
DEFAULT_ORDER_LISTS = [[6, 6, 6, 7], [1, 6]]


def cepdet_key(npoints, hop, ninit, ncoefs, p, q):
    return f"cepdet_{npoints}_{hop}_{ninit}_{ncoefs}_{p}_{q}"


def burg_segments(npoints):
    x = sig("CS3").astype(np.float64)
    starts = np.random.default_rng(1).integers(0, x.size - npoints, size=8)
    return [np.ascontiguousarray(x[s:s + npoints] * np.hamming(npoints)) for s in starts]


def frames(x, npoints, hop):
    n = (x.size - npoints) // hop + 1
    return np.ascontiguousarray(np.stack([x[t * hop:t * hop + npoints] for t in range(n)]).astype(np.float64))


def median_utterances():
    return (sig("CS0")[::2].copy(), synth_utt(31, 8000 * 3 + 5, fs=8000), synth_utt(32, 120 + 80 * 2, fs=8000))  # the last: two frames


def median_inputs(cri, u):
    """The oracle at -vad_filter_order 1: the vectors that enter the filter and the raw decisions vad0."""
    rows1, vad1 = Oracle(MEDIAN_BASE + cri.split() + ["-vad_filter_order", "1"]).process(u, want_vad=True)
    return rows1, (np.asarray(vad1) == ord("1")).astype(np.uint8)


def identity_inputs():
    rng = np.random.default_rng(1)
    return rng.standard_normal((50, 4)), rng.integers(0, 2, 50).astype(np.uint8)


def list_frames(order):
    rng = np.random.default_rng(order)
    return [[int(x) for x in rng.integers(0, 12, 7)] + [9] for _ in range(LIST_TRIALS)]


def _median_filter(L, order, feats, vad0):
    T, nf = feats.shape
    feats = np.ascontiguousarray(feats, dtype=np.float64)
    vad0 = np.ascontiguousarray(vad0, dtype=np.uint8)
    dec = np.zeros(T + order, dtype=np.uint8)
    out = np.zeros((T + order, nf), dtype=np.float64)
    n = L.ref_median_run(order, nf, feats.ctypes.data, vad0.ctypes.data, T, dec.ctypes.data, out.ctypes.data)
    return dec[:n], out[:n]


def _median_list(L, order, fr):
    fr = np.array(fr, dtype=np.int32)
    out = np.zeros(int(fr.sum()) + 2 * order * fr.size + 8)
    n = np.zeros(fr.size, dtype=np.int32)
    L.ref_median_list(order, fr.ctypes.data, fr.size, out.ctypes.data, n.ctypes.data)
    return out[:int(n.sum())].astype(np.int32), n


def main():
    def load(name):
        path = os.path.join(REF, name)
        if not os.path.exists(path):
            raise SystemExit(f"{path} is missing: build it first (make -C oracle ref REF=<reference tree>)")
        return ctypes.CDLL(path)

    z = {}
    am = load("libref_amulaw.so")
    for key, mode in (("amulaw_mu", 0), ("amulaw_a", 1)):
        t = np.zeros(256, dtype=np.int16)
        am.ref_amulaw_table(mode, t.ctypes.data_as(ctypes.c_void_p))
        z[key] = t

    bg = load("libref_burg.so")
    bg.ref_burg_cepstrum.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    for npoints, ncoefs in BURG_CASES:
        a_all, c_all, al_all = [], [], []
        for seg in burg_segments(npoints):
            a, c, al = np.zeros(ncoefs), np.zeros(ncoefs), ctypes.c_double()
            bg.ref_burg_cepstrum(seg.ctypes.data, npoints, ncoefs, a.ctypes.data, c.ctypes.data, ctypes.byref(al))
            a_all.append(a)
            c_all.append(c)
            al_all.append(al.value)
        z[f"burg_{npoints}_{ncoefs}_a"], z[f"burg_{npoints}_{ncoefs}_c"] = np.array(a_all), np.array(c_all)
        z[f"burg_{npoints}_{ncoefs}_alpha"] = np.array(al_all)

    cd = load("libref_cepdet.so")
    cd.ref_cepdet_new.restype = ctypes.c_void_p
    cd.ref_cepdet_new.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]
    cd.ref_cepdet_run.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    cd.ref_cepdet_delete.argtypes = [ctypes.c_void_p]
    for case in CEPDET_CASES:
        npoints, hop, ninit, ncoefs, p, q = case
        for name in ("CS0", "CS3"):
            fr = frames(sig(name), npoints, hop)
            dec = np.zeros(fr.shape[0], dtype=np.uint8)
            h = cd.ref_cepdet_new(npoints, ninit, ncoefs, p, q)
            cd.ref_cepdet_run(h, fr.ctypes.data, npoints, fr.shape[0], dec.ctypes.data)
            cd.ref_cepdet_delete(h)
            z[f"{cepdet_key(*case)}_{name}"] = dec

    md = load("libref_median.so")
    md.ref_median_run.restype = ctypes.c_int
    md.ref_median_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    md.ref_median_list.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    for ci, cri in enumerate(MEDIAN_CRITERIA):
        for k, u in enumerate(median_utterances()):
            rows1, vad0 = median_inputs(cri, u)
            for order in MEDIAN_ORDERS:
                dec, out = _median_filter(md, order, rows1.astype(np.float64), vad0)
                z[f"median_{ci}_{order}_{k}_dec"], z[f"median_{ci}_{order}_{k}_out"] = dec, out.astype(np.float32)
    dec, out = _median_filter(md, 1, *identity_inputs())
    z["median_identity_dec"], z["median_identity_out"] = dec, out
    for order in LIST_ORDERS:
        for trial, fr in enumerate(list_frames(order)):
            z[f"medlist_{order}_{trial}_frames"] = np.array(fr, dtype=np.int32)
            z[f"medlist_{order}_{trial}_rows"], z[f"medlist_{order}_{trial}_n"] = _median_list(md, order, fr)
    for j, fr in enumerate(DEFAULT_ORDER_LISTS):
        z[f"medlist_3_default{j}_frames"] = np.array(fr, dtype=np.int32)
        z[f"medlist_3_default{j}_rows"], z[f"medlist_3_default{j}_n"] = _median_list(md, 3, fr)

    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
