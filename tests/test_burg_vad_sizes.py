"""The VAD's Burg-cepstral criterion (-vad burg -vad_cri_mode cepdist -vad_cepdist_mode lpc, src/vad/vad.cc:149-294) at every FFT
size: 1024 .. 4096 points (bigfft_kernel exports the spectra, bigburg_kernel.h runs the inverse transform and the lattice with a
workgroup per frame) and 32 .. 128 points (vad_burg_kernel on every (256 / N)-th bin of the 256-point mode's spectra).

Decisions are states: a flipped byte moves the threshold recurrences for the rest of the file, so every byte of every file must
equal the float64 oracle's.  The oracle's own counts (frames, ones, transitions per file) are asserted too: a file of empty or
constant decisions cannot pass for a detector.
"""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.util import C2, C4, sig, synth_utt

pytestmark = pytest.mark.gpu

TOL = 1e-4   # the suite's bound on rows (tests/test_gpu_parity.py)

V = "-vad burg -vad_out_mode vad -vad_cri_mode cepdist -vad_cepdist_mode lpc".split()


def M(fs):
    return f"-fs {fs} -format_in raw -format_out htk -preset mfcc -preem 0.97".split()


def rel_err(got, ref):
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)).max()) if ref.size else 0.0


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


def u16():
    return [sig("CS0")[:50000], synth_utt(71, 30000), sig("CS3")[:44000], synth_utt(73, 9000)]


def u44():
    return [synth_utt(130 + i, 40000 + 7111 * i) for i in range(3)] + [sig("CS0")[:50000]]


def u8():
    return [synth_utt(90 + i, 5000 + 1777 * i, fs=8000) for i in range(3)] + [sig("CS3")[:20000]]


def counts(v):
    """(frames, ones, transitions) of a file's decision bytes."""
    one = v == ord("1")
    return int(v.size), int(one.sum()), int((one[1:] != one[:-1]).sum())


def agreement(Engine, cfg, utts, expect):
    """Engine against Oracle(cfg): every decision byte equal; rows within TOL (drop off) or as many rows as '1' bytes (drop on).
    `expect`: the oracle's (frames, ones, transitions) per file."""
    eng = Engine(cfg)
    rows, vads = eng.extract(utts, want_vad=True)
    orc = Oracle(cfg)
    drop = "drop" in cfg
    for i, (u, r, v) in enumerate(zip(utts, rows, vads)):
        ref_rows, ref_vad = orc.process(u, want_vad=True)
        assert counts(ref_vad) == expect[i], (i, counts(ref_vad))
        assert v.size == ref_vad.size and set(np.unique(v)) <= {ord("0"), ord("1")}
        diff = np.flatnonzero(v != ref_vad)
        print(f"file {i}: {counts(v)} differing bytes {diff.size}" + (f" first at frame {diff[0]}" if diff.size else ""))
        assert diff.size == 0, (i, diff[:8])
        assert r.shape == ref_rows.shape
        if drop:
            assert r.shape[0] == int((v == ord("1")).sum())
        print(f"file {i}: rows rel err {rel_err(r, ref_rows):.3g}")
        assert rel_err(r, ref_rows) <= TOL
    return eng, rows, vads


def batch_invariance(eng, utts, rows, vads, i):
    r1, v1 = eng.extract([utts[i]], want_vad=True)
    assert np.array_equal(v1[0], vads[i]) and np.array_equal(r1[0], rows[i])


W40 = ["-w", "40", "-s", "10"]   # 640 samples -> 1024 points


def test_1024_points_adapt(Engine):
    cfg = C2 + W40 + V + ["-vad_thr_mode", "adapt"]
    utts = u16()
    eng, rows, vads = agreement(Engine, cfg, utts, [(309, 237, 1), (184, 45, 12), (272, 189, 1), (53, 0, 0)])
    assert eng.kernel_name() == "bigfft_kernel<4>"
    batch_invariance(eng, utts, rows, vads, 1)
    # the criterion matters: the energy criterion decides differently on at least one file
    _, ven = Engine(C2 + W40 + "-vad_out_mode vad -vad_cri_mode energy -vad_thr_mode adapt".split()).extract(utts, want_vad=True)
    assert any(not np.array_equal(a, b) for a, b in zip(vads, ven))


def test_1024_points_exten_dyn(Engine):
    cfg = C2 + W40 + ["-nr_mode", "exten", "-nr_a", "2"] + V + ["-vad_thr_mode", "dyn"]
    utts = u16()[:2]
    eng, rows, vads = agreement(Engine, cfg, utts, [(309, 179, 22), (184, 77, 18)])
    batch_invariance(eng, utts, rows, vads, 1)


def test_1024_points_delta_drop_filter5(Engine):
    cfg = C2 + W40 + ["-fea_delta", "d_a", "-vad_apply_mode", "drop", "-vad_filter_order", "5"] + V + ["-vad_thr_mode", "adapt"]
    agreement(Engine, cfg, u16()[:2], [(309, 241, 1), (184, 27, 8)])


def test_1024_points_odd_window_20_coefficients(Engine):
    cfg = C2 + ["-w", "40.0625", "-s", "10.0625", "-vad_lpc_coefs", "20"] + V + ["-vad_thr_mode", "adapt"]   # 641 / 161 samples
    agreement(Engine, cfg, u16()[:2], [(307, 235, 1), (183, 35, 8)])


def test_2048_points_adapt(Engine):
    cfg = M(44100) + V + ["-vad_thr_mode", "adapt"]   # 1103 samples
    utts = u44()
    eng, rows, vads = agreement(Engine, cfg, utts, [(89, 13, 6), (105, 10, 6), (121, 37, 17), (111, 85, 1)])
    assert eng.kernel_name() == "bigfft_kernel<8>"
    batch_invariance(eng, utts, rows, vads, 2)


def test_2048_points_exten_dyn(Engine):
    cfg = M(44100) + ["-nr_mode", "exten"] + V + ["-vad_thr_mode", "dyn"]
    utts = u44()
    eng, rows, vads = agreement(Engine, cfg, utts, [(89, 27, 14), (105, 35, 18), (121, 41, 21), (111, 93, 14)])
    batch_invariance(eng, utts, rows, vads, 3)


def test_4096_points_adapt(Engine):
    cfg = M(48000) + ["-w", "64", "-s", "20"] + V + ["-vad_thr_mode", "adapt"]   # 3072 samples
    utts = u44()
    eng, rows, vads = agreement(Engine, cfg, utts, [(39, 9, 3), (46, 0, 0), (54, 4, 4), (49, 5, 4)])
    assert eng.kernel_name() == "bigfft_kernel<16>"
    batch_invariance(eng, utts, rows, vads, 0)


def test_128_points_8k(Engine):
    cfg = M(8000) + ["-w", "16", "-s", "8"] + V + ["-vad_thr_mode", "adapt"]
    utts = u8()
    eng, rows, vads = agreement(Engine, cfg, utts, [(77, 0, 0), (104, 17, 4), (132, 20, 6), (311, 76, 13)])
    batch_invariance(eng, utts, rows, vads, 1)


def test_128_points_16k_dyn(Engine):
    agreement(Engine, C2 + ["-w", "8", "-s", "4"] + V + ["-vad_thr_mode", "dyn"], [synth_utt(95, 20000)], [(311, 148, 58)])


def test_64_points(Engine):
    """32 samples at 8 kHz -> 64 points; the preset's bank has a filter with no spectral bin there (the oracle refuses it), so the
    bank of tests/test_gpu_parity.py::test_fft_sizes_below_256.  The oracle accepts it and its decisions are mixed."""
    cfg = M(8000) + ["-w", "8", "-s", "4", "-fb_definition", "1-10/10filters", "-fea_ncepcoefs", "8"] + V + ["-vad_thr_mode", "dyn"]
    agreement(Engine, cfg, u8()[:2] + [sig("CS3")[:20000]], [(155, 65, 20), (210, 58, 16), (624, 291, 101)])


def test_256_and_512_point_paths_are_untouched(Engine):
    assert Engine(C4).kernel_name() == "frontend_kernel<13, DCTC, MODE 1, exten, MD, VF>"
    assert Engine(C2 + V).kernel_name() == "frontend_kernel<13, DCTC, MODE 0, plain, MD, VF>"
