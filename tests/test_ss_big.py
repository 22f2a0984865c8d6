"""hwss / fwss / 2fwss (-nr_mode, src/nr/nr.cc:181-442) on 2048- and 4096-point frames - 44.1 / 48 kHz audio at the presets' 25 ms, or long
windows: bigfft_kernel exports the spectra once, bigssdet_kernel and ss_decide_kernel give the Burg cepstral detector's decisions,
bigss_kernel<8|16> subtracts along chains of whole utterances once per pass of the seed iteration (bigss_kernel.h).

Everything is held against ONE Oracle(cfg) instance walking the same list in order: a file's noise estimate starts from the vector
the previous file left.  The bound is the suite's bound for an NR configuration (tests/test_gpu_parity.py::_assert_rows): element-wise
|a-b| <= 1e-3 max(|b|, 1) AND 1e-4 of the row's largest value.  For 2fwss only, the suite allows frames outside that rule - at most
max(1, frames // 100) per file, none above 5e-2 (test_spectral_subtraction_at_16khz) - and the clause is taken over unchanged; the
count and the worst value per file are printed.  Measured on an MI355X over the 70 files of this module: no frame outside the rule in
any mode (2fwss: the clause was not needed, worst element-wise 3.6e-5); worst element-wise 7.0e-4 (hwss, a = 2, b = 1.5), 4.8e-6 of the
row's largest value; speech within 1 LSB.
"""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.test_ss_big_cpu import B, FEATURE_CONFIGS, M, SIGNAL_CONFIGS, W64, ident
from tests.util import C2, sig, synth_utt

pytestmark = pytest.mark.gpu

FRAMES = {2048: [89, 105, 121, 111, 0, 66], 4096: [39, 46, 54, 49, 0, 29]}   # the oracle's counts: 1103 / 441 and 3072 / 960 samples


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


def points(cfg):
    return 4096 if "48000" in cfg else 2048


def the_list(cfg):
    frameless = synth_utt(18, 700) if points(cfg) == 2048 else synth_utt(18, 2200)   # the pre-load and no hop
    return [synth_utt(130 + i, 40000 + 7111 * i) for i in range(3)] + [sig("CS0")[:50000], frameless, synth_utt(140, 30000)]


def errors(g, ref):
    """Per frame: the element-wise error relative to max(|b|, 1), and the row's error relative to its largest value."""
    e = (np.abs(g - ref) / np.maximum(np.abs(ref), 1.0)).max(axis=1)
    rn = np.abs(g - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1.0)
    return e, rn


def assert_rows(g, ref, cfg, tag):
    assert g.shape == ref.shape, (tag, g.shape, ref.shape)
    assert np.isfinite(g).all(), tag
    if not ref.size:
        return
    e, rn = errors(g, ref)
    out = (e > 1e-3) | (rn > 1e-4)
    print(f"{tag}: {ref.shape[0]} frames, element-wise {e.max():.3g}, of the row's largest {rn.max():.3g}, frames outside the rule {int(out.sum())}")
    if "2fwss" in cfg:
        assert out.sum() <= max(1, ref.shape[0] // 100) and e.max() <= 5e-2, (tag, int(out.sum()), float(e.max()))
    else:
        assert e.max() <= 1e-3 and rn.max() <= 1e-4, (tag, float(e.max()), float(rn.max()))


# beside the configurations of tests/test_ss_big_cpu.py: the raw energy (the export pass writes the column) behind a delta chain and CMS, and
# LP analysis on uncompressed bands with its energy column (log R[0], the double tail inside big_project)
MORE_CONFIGS = [
    M(44100) + B + ["-nr_mode", "fwss", "-fea_E", "on", "-fea_rawenergy", "on", "-fea_delta", "d_a", "-fea_Z_exp", "0.95"],
    M(48000) + W64 + B + ["-nr_mode", "hwss", "-fea_kind", "lpc", "-fea_lporder", "10", "-fea_E", "on"],
]


@pytest.mark.parametrize("cfg", FEATURE_CONFIGS + MORE_CONFIGS, ids=ident)
def test_feature_configurations_against_the_oracles_walk_of_the_list(Engine, cfg):
    utts = the_list(cfg)
    eng, orc = Engine(cfg), Oracle(cfg)
    assert eng.kernel_name() == ("bigss_kernel<8>" if points(cfg) == 2048 else "bigss_kernel<16>")
    got = eng.extract(utts)
    refs = [orc.process(u) for u in utts]
    assert [r.shape[0] for r in refs] == FRAMES[points(cfg)]
    for i, (g, ref) in enumerate(zip(got, refs)):
        assert_rows(g, ref, cfg, f"file {i}")
    # the chain is real: the same file alone (zero seed) comes out differently from its place in the list
    alone = Engine(cfg).extract([utts[1]])[0]
    d = float(np.abs(alone - got[1]).max())
    print(f"file 1 alone against its place in the list: {d:.3g}")
    assert d > 1e-3


@pytest.mark.parametrize("cfg", [FEATURE_CONFIGS[0], FEATURE_CONFIGS[8]], ids=ident)
def test_the_chain_survives_between_runs_and_reset_forgets_it(Engine, cfg):
    utts = the_list(cfg)
    whole = Engine(cfg).extract(utts)
    eng = Engine(cfg)
    parts = eng.extract(utts[:3]) + eng.extract(utts[3:5]) + eng.extract(utts[5:])   # cut after file 3 and after the frameless file
    for a, b in zip(whole, parts):
        assert np.array_equal(a, b)
    eng.reset_chain()
    fresh = Engine(cfg).extract(utts[3:])
    for a, b in zip(eng.extract(utts[3:]), fresh):
        assert np.array_equal(a, b)
    assert not np.array_equal(fresh[0], whole[3])


def test_rows_do_not_depend_on_the_batch_beyond_the_seed(Engine):
    cfg = FEATURE_CONFIGS[0]
    utts = the_list(cfg)
    a, b = Engine(cfg).extract(utts), Engine(cfg).extract(utts)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # more utterances than one chain holds: 300 files of 3 to 40 frames, every one against the oracle's sequential walk
    rng = np.random.default_rng(5)
    base = synth_utt(77, 44100 * 20)
    short = []
    for _ in range(300):
        n = 662 + 441 * int(rng.integers(3, 41)) + int(rng.integers(0, 441))
        o = int(rng.integers(0, base.size - n))
        short.append(base[o:o + n])
    got = Engine(cfg).extract(short)
    orc = Oracle(cfg)
    worst = rown = 0.0
    for u, g in zip(short, got):
        ref = orc.process(u)
        assert g.shape == ref.shape and 3 <= ref.shape[0] <= 40
        e, rn = errors(g, ref)
        worst, rown = max(worst, float(e.max())), max(rown, float(rn.max()))
    print(f"300 short files: element-wise {worst:.3g}, of the row's largest {rown:.3g}")
    assert worst <= 1e-3 and rown <= 1e-4, (worst, rown)


@pytest.mark.parametrize("mode,fs", [("fwss", 44100), ("hwss", 44100), ("2fwss", 48000)])
def test_decisions_from_a_file(Engine, tmp_path, mode, fs):
    # -vad file=<f> (src/nr/nr.cc:205-209, 297-302): one byte per frame out of ONE stream for the whole list, every byte but NUL = speech
    from ctucopy_amd import CtuError
    base = M(fs) + (W64 if fs == 48000 else []) + ["-nr_mode", mode]
    if mode == "hwss":  # half-wave rectification under arbitrary decisions empties whole bands: band energies instead of their logarithms
        base += ["-fea_kind", "spec"]
    utts = the_list(base)
    probe = Oracle(base + B)
    frames = [max(probe.num_frames(u.size), 0) for u in utts]
    assert frames == FRAMES[points(base)]
    stream = np.random.default_rng(9).choice(np.array([0, 0, 1, 7, ord("0")], np.uint8), sum(frames))
    f = tmp_path / "vad.bin"
    f.write_bytes(bytes(stream))
    cfg = base + ["-vad", f"file={f}"]
    eng, orc = Engine(cfg), Oracle(cfg)
    assert eng.kernel_name().startswith("bigss_kernel<")
    got = eng.extract(utts[:3]) + eng.extract(utts[3:])          # two runs: the stream (and the noise seed) carry over
    for i, (u, g) in enumerate(zip(utts, got)):
        assert_rows(g, orc.process(u), cfg, f"file {i}")
    with pytest.raises(CtuError, match="Unexpected end of VAD file"):   # the stream is spent
        eng.extract(utts[:1])
    eng.reset_chain()                                            # rewinds it (a new process)
    again = eng.extract(utts[:3])
    assert all(np.array_equal(x, y) for x, y in zip(again, got[:3]))
    eng.set_vad_stream(bytes(stream[:5]) + b"\xff" + bytes(stream[5:]))   # 0xFF == EOF in the reference's signed char
    with pytest.raises(CtuError, match="Unexpected end of VAD file"):
        eng.extract(utts[:1])


@pytest.mark.parametrize("cfg", SIGNAL_CONFIGS, ids=ident)
def test_speech_output(Engine, cfg):
    """bigss_kernel leaves the subtracted magnitudes for bigsynth_kernel; the next file's seed carries sigOUT's sign flip of the Nyquist
    entry (src/io/out.cc:419).  The suite's bound on enhanced speech: at most 2 LSB, mean below 0.3."""
    utts = the_list(cfg)[:3]
    eng, orc = Engine(cfg), Oracle(cfg)
    assert eng.dims.signal_out == 1 and eng.kernel_name() == ("bigss_kernel<8>" if points(cfg) == 2048 else "bigss_kernel<16>")
    got = eng.enhance(utts)
    refs = [orc.enhance(u) for u in utts]
    if points(cfg) == 2048:
        assert [r.size for r in refs] == [39535, 46595, 53655]
    for k, (g, ref) in enumerate(zip(got, refs)):
        assert g.shape == ref.shape and g.dtype == np.int16, k
        d = np.abs(g.astype(int) - ref.astype(int))
        print(f"file {k}: {ref.size} samples, worst {d.max()} LSB, mean {d.mean():.3g}")
        assert d.max() <= 2 and d.mean() < 0.3, (k, d.max(), d.mean())


def test_every_other_configuration_keeps_its_kernel(Engine):
    assert Engine(M(44100)).kernel_name() == "bigfft_kernel<8>"
    assert Engine(M(44100) + ["-nr_mode", "exten"]).kernel_name() == "bigfft_kernel<8>"
    assert ", SS" in Engine(C2 + B + ["-nr_mode", "fwss"]).kernel_name()
