"""Pins the oracle's majority filter - decisions, the delay of the feature vectors through its ring and the flush - against the
reference's own medianFilter.

src/vad/vad.h:79-176 is header-only and FFTW-free (it pulls in io/opts.h and base/types.h): oracle/Makefile compiles it where it lies
into oracle/_ref/libref_median.so, driven as VAD::process_frame / BATCH::flush_vad drive it (src/vad/vad.cc:692-699, 742-745;
src/io/batch.cc:230-249); tests/golden/make_ref_fixtures.py recorded what it wrote in tests/golden/ref_outputs.npz.  The raw decisions vad0 do not depend on the filter (the thresholds and the
background update consume vad0, src/vad/vad.cc:696-697): the oracle's run with -vad_filter_order 1 supplies them and the vectors that
enter the filter, and its runs with orders 3, 5, 7 must equal the reference class fed with those.
"""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.golden.make_ref_fixtures import (MEDIAN_BASE, MEDIAN_CRITERIA, MEDIAN_ORDERS, identity_inputs, list_frames, median_inputs,
                                            median_utterances)
from tests.util import ref_outputs, synth_utt


@pytest.mark.parametrize("cri", MEDIAN_CRITERIA)
@pytest.mark.parametrize("order", MEDIAN_ORDERS)
def test_majority_filter_and_feature_delay_identical_to_reference_header(cri, order):
    z = ref_outputs()
    ci = MEDIAN_CRITERIA.index(cri)
    base = MEDIAN_BASE + cri.split()
    for k, u in enumerate(median_utterances()):   # the last one: two frames
        rows1, vad0 = median_inputs(cri, u)
        rows, vad = Oracle(base + ["-vad_filter_order", str(order)]).process(u, want_vad=True)
        T = vad0.size
        assert rows1.shape[0] == T
        dec, out = z[f"median_{ci}_{order}_{k}_dec"], z[f"median_{ci}_{order}_{k}_out"]   # the reference class fed with rows1, vad0
        # the filter delays by (order-1)/2 frames and the flush makes up for it: frame count unchanged - unless the file has no more
        # frames than the delay: the filter never gets `ready`, BATCH::flush_vad's loop does not start, nothing is written at all
        assert dec.size == (T if T > (order - 1) // 2 else 0)
        assert rows.shape[0] == dec.size and len(vad) == dec.size
        assert np.array_equal(dec, (np.asarray(vad) == ord("1")).astype(np.uint8))
        assert np.array_equal(out, rows)      # the vectors the writer sees: delayed by (order-1)/2 frames, the ring's
                                                                 # oldest entries at the flush


def test_order_one_is_the_identity():
    z = ref_outputs()
    feats, vad0 = identity_inputs()
    dec, out = z["median_identity_dec"], z["median_identity_out"]
    assert np.array_equal(dec, vad0) and np.array_equal(out, feats)


def _ref_list(z, key, frames):
    """The reference class driven over a list of files with these frame counts: per file, the frame numbers of the rows it writes."""
    assert z[key + "_frames"].tolist() == list(frames)
    rows, n = z[key + "_rows"].astype(int), z[key + "_n"]
    res, w = [], 0
    for k in range(len(frames)):
        res.append(rows[w:w + n[k]])
        w += n[k]
    return res


@pytest.mark.parametrize("order", [3, 5])
def test_the_filter_ring_runs_on_from_file_to_file(order):
    """One VAD object serves the whole list and VAD::clean() = cleanFilter() resets `start`, the ring and the decisions but neither
    historyIdx nor historySize (src/vad/vad.h:110-121): the next file's vectors land in ring slots out of phase with the slots its outputs
    are read from.  The reference class driven over lists of files (value = frame index + 1, 0 = an untouched slot) against the oracle's
    list mode: which frame's vector each written row carries, all-zero rows and row counts included."""
    z = ref_outputs()
    base = "-fs 8000 -format_in raw -format_out htk -preset mfcc -fea_kind spec -vad_out_mode vad -vad_cri_mode energy -vad_thr_mode adapt".split()
    cfg = base + ["-vad_filter_order", str(order)]
    for trial, frames in enumerate(list_frames(order)):
        utts = [synth_utt(200 + 10 * trial + i, 120 + 80 * T + (0 if T else 40), fs=8000) for i, T in enumerate(frames)]
        want = _ref_list(z, f"medlist_{order}_{trial}", frames)
        o = Oracle(cfg)
        got = o.process_list(utts, want_vad=True)
        alone = [Oracle(cfg).process(u) for u in utts]           # every file as the first of its own process: the undisturbed vectors
        for k, (T, (rows, vad), src) in enumerate(zip(frames, got, want)):
            assert rows.shape[0] == src.size == len(vad), (order, frames, k)
            for r, t1 in zip(rows, src):
                if t1 == 0:
                    assert not r.any()                           # a ring slot this file has not written yet: zeros
                else:
                    # the frame's own vector; a file no longer than the delay writes nothing when alone, so take it from a longer run
                    full = alone[k] if alone[k].shape[0] == T else None
                    if full is not None:
                        assert np.array_equal(r, full[t1 - 1]), (order, frames, k, t1)
    # the first file of a process, and process() by default, start in phase
    assert Oracle(cfg).vad_ring() == (0, 0)


def test_reference_list_behaviour_at_the_default_order():
    """What a user of the reference gets at -vad_filter_order 3 (its default): rows of a file shifted by one frame either way, depending on
    the frame counts of the files in front of it."""
    z = ref_outputs()
    assert [r.tolist() for r in _ref_list(z, "medlist_3_default0", [6, 6, 6, 7])] == [[1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5], [2, 3, 4, 5, 6, 4],
                                                                                    [1, 2, 3, 4, 5, 6, 7]]
    assert [r.tolist() for r in _ref_list(z, "medlist_3_default1", [1, 6])] == [[], [2, 3, 4, 5, 6, 4]]
