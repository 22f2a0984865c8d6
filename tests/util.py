"""Shared test helpers: configurations of BASELINE.json and fixture loading."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# egs/conf/01_mfcc_0_16k_2510_30.ctuconf of the reference, written out as a command line (C1).
C1 = ("-fs 16000 -format_in raw -format_out htk -endian_in little -endian_out little -w 25 -s 10 -preem 0.97 "
      "-fb_scale mel -fb_shape triang -fb_power on -fb_definition 30filters -nr_mode none -fb_eqld off "
      "-fb_inld off -fea_kind dctc -fea_ncepcoefs 12 -fea_c0 on -fea_E off -fea_lifter 22 -fea_rawenergy off").split()
# SURVEY.md Appendix B command lines (C2..C5)
C2 = "-fs 16000 -format_in raw -format_out htk -preset mfcc -preem 0.97".split()
C3 = "-fs 16000 -format_in raw -format_out htk -preset plpc".split()
C4 = ("-fs 8000 -format_in raw -format_out htk -preset mfcc -nr_mode exten -nr_a 2 -vad burg -vad_out_mode vad "
      "-vad_cri_mode cepdist -vad_cepdist_mode lpc -vad_thr_mode adapt").split()
C4_NOVAD = "-fs 8000 -format_in raw -format_out htk -preset mfcc -nr_mode exten -nr_a 2".split()
C5 = ("-fs 16000 -format_in raw -format_out htk -preset mfcc -fb_definition 23filters "
      "-fea_kind trapdct,101,16").split()


def sig(name):
    """Bundled reference signals (egs/sig of the reference: 16 kHz int16 LE raw)."""
    return np.fromfile(os.path.join(GOLDEN, "SA000CB1." + name), dtype="<i2")


def synth_utt(seed, nsamples, fs=16000, noise=300.0):
    """Small deterministic speech-like utterance for tests (harmonics of a gliding f0 + AM + white noise)."""
    rng = np.random.default_rng(seed)
    t = np.arange(nsamples) / fs
    f0 = 90 + 160 * (0.5 + 0.5 * np.sin(2 * np.pi * 0.31 * t + rng.uniform(0, 6.28)))
    ph = 2 * np.pi * np.cumsum(f0) / fs
    x = np.zeros(nsamples)
    for h in range(1, 5):
        x += np.sin(h * ph + rng.uniform(0, 6.28)) / h
    x *= 6000 * (0.6 + 0.4 * np.sin(2 * np.pi * 4 * t))
    x += rng.normal(0, noise, nsamples)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def ref_outputs():
    """What the reference's own FFTW-free pieces computed on the inputs of the *_ref tests (made by tests/golden/make_ref_fixtures.py)."""
    return np.load(os.path.join(GOLDEN, "ref_outputs.npz"))


# ---- the compiled reference end to end: tests/golden/ref_e2e.npz (made by tests/golden/make_ref_e2e_fixtures.py from oracle/_ref/ctucopy4_ref)
def square_fs(n):
    return np.where((np.arange(n) // 40) % 2 == 0, 32767, -32768).astype(np.int16)


def alt_fs(n):
    return np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)


def const_max(n):
    return np.full(n, 32767, np.int16)


def const_min(n):
    return np.full(n, -32768, np.int16)


def lsb_noise(n):
    return np.random.default_rng(1).integers(-1, 2, n).astype(np.int16)


def clipped(n):
    return np.clip(synth_utt(3, n).astype(np.int32) * 8, -32768, 32767).astype(np.int16)


def sine_fs_4(n):
    return np.array([0, 32767, 0, -32767], np.int16)[np.arange(n) % 4]   # round(32767 sin(2 pi t / 4))


def zeros_mid_parts(n):
    """(speech, zeros, speech) sample counts of zeros_mid: 3000 / 2000 / 3000 at n = 8000."""
    return 3 * n // 8, n // 4, 3 * n // 8


def zeros_mid(n):
    a, z, b = zeros_mid_parts(n)
    u = synth_utt(3, n)
    return np.concatenate([u[:a], np.zeros(z, np.int16), u[a:a + b]])


EDGE_INPUTS = ("square_fs", "alt_fs", "const_max", "const_min", "lsb_noise", "clipped", "sine_fs_4", "zeros_mid")
M8 = "-fs 8000 -format_in raw -format_out htk -preset mfcc -preem 0.97".split()
M44 = "-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97".split()
HIRES_BANK = ["-fb_definition", "1-40/40filters", "-fea_ncepcoefs", "39"]
SIG_EXTEN = "-fs 16000 -format_in raw -format_out raw -preset exten".split()
ENERGY_SILENCE = "-vad_out_mode vad -vad_cri_mode energy -vad_thr_mode dyn -fea_delta d_a -vad_apply_mode silence".split()

# name -> (command line, input set).  Input sets: "ord" = the two ordinary files (186 and 98 frames of 25 / 10 ms), "short" = the same two cut
# to 9000 samples (55 frames each: past half a 101-frame TRAP context) where rows are wide, samples come out or the chain is pinned at length
# elsewhere - the fixture's size is bounded; "cs3_8k" = CS3 read as 8 kHz; "edge<n>" = the eight edge inputs of n samples.
# All files of a case are ONE list of one process.
REF_E2E_CASES = {
    "c1": (C1, "ord"), "c2": (C2, "ord"), "c3": (C3, "ord"), "c5": (C5, "short"), "c4": (C4, "ord"),
    "c2_exten": (C2 + ["-nr_mode", "exten"], "ord"),
    "c2_fwss": (C2 + ["-nr_mode", "fwss", "-vad", "burg"], "ord"),
    "c2_da_zexp_e": (C2 + "-fea_delta d_a -fea_Z_exp 500 -fea_E on".split(), "short"),
    "c2_trap9": (C2 + ["-fea_trap", "9"], "short"),
    "c2_hires": (C2 + HIRES_BANK, "short"),
    "c2_w40": (C2 + ["-w", "40"], "short"),
    "c2_dc1": (C2 + ["-remove_dc1", "on"], "short"),
    "c2_silence_energy": (C2 + ENERGY_SILENCE, "ord"),
    "c3_inld_off": (C3 + ["-fb_inld", "off"], "short"),
    "m44": (M44, "ord"),
    "m48_w64": ("-fs 48000 -format_in raw -format_out htk -preset mfcc -preem 0.97 -w 64 -s 20".split(), "ord"),
    "m8_64pt": (M8 + "-w 8 -s 4 -fb_definition 1-10/10filters -fea_ncepcoefs 8".split(), "short"),
    "m8_cs3": (M8, "cs3_8k"),
    "sig_exten": (SIG_EXTEN, "short"),
    "sig_fwss": ("-fs 16000 -format_in raw -format_out raw -w 25 -s 12.5 -nr_mode fwss -vad burg".split(), "short"),
    "sig_44_exten": ("-fs 44100 -format_in raw -format_out raw -w 24 -s 12.5 -nr_mode exten".split(), "short"),
    "edge_a": (C2, "edge8000"), "edge_b": (C3, "edge8000"), "edge_c": (C2 + ["-nr_mode", "exten"], "edge8000"),
    "edge_d": (M8, "edge4000"), "edge_e": (C2 + ["-w", "40"], "edge8000"),
    "edge_f": (M44, "edge23151"),          # 3 windows of 1102 samples + 45 shifts of 441
    "edge_g": (C2 + HIRES_BANK, "edge8000"), "edge_h": (C2 + ["-preem", "0", "-remove_dc", "off"], "edge8000"),
    "edge_i": (SIG_EXTEN, "edge8000"),
    # -fea_Z_block with blocks below, between and above the files' 55 frames ("short") and 186 / 98 frames ("ord"), and the Burg assertion
    # behind `silence`: what the reference dies on is recorded with its exit status only
    "zblock_30": (C2 + ["-fea_Z_block", "30"], "short"), "zblock_55": (C2 + ["-fea_Z_block", "55"], "short"),
    "zblock_56": (C2 + ["-fea_Z_block", "56"], "short"), "zblock_300": (C2 + ["-fea_Z_block", "300"], "short"),
    "zblock_30_da": (C2 + ["-fea_Z_block", "30", "-fea_delta", "d_a"], "short"),
    "zblock_300_da": (C2 + ["-fea_Z_block", "300", "-fea_delta", "d_a"], "short"),
    "zblock_150_ord": (C2 + ["-fea_Z_block", "150"], "ord"),
    "zblock_300_e": (C2 + ["-fea_Z_block", "300", "-fea_E", "on"], "short"),
    "c4_da_silence": (C4 + ["-fea_delta", "d_a", "-vad_apply_mode", "silence"], "ord"),
}


def ref_e2e_inputs(name):
    """The files of one input set of REF_E2E_CASES / REF_E2E_OPT_CASES / REF_E2E_SILENCE_CASES, in list order."""
    if name.startswith("sil"):
        n = int(name[len("sil"):])
        return [zeros_mid(n), synth_utt(3, n // 2)]
    if name == "short3":
        a, b = ref_e2e_inputs("short")
        return [a, synth_utt(5, 300), b]
    if name == "ord":
        return [sig("CS0")[:30000].copy(), synth_utt(3, 16000)]
    if name == "short":
        return [sig("CS0")[:9000].copy(), synth_utt(3, 9000)]
    if name == "cs3_8k":
        return [sig("CS3")[:40000].copy()]
    n = int(name[len("edge"):])
    return [globals()[g](n) for g in EDGE_INPUTS]


def ref_e2e():
    """What the compiled reference wrote for REF_E2E_CASES (keys: tests/golden/make_ref_e2e_fixtures.py)."""
    return np.load(os.path.join(GOLDEN, "ref_e2e.npz"))


# ---- the rest of the option space against the compiled reference: tests/golden/ref_e2e_opts.npz (make_ref_e2e_fixtures.py opts)
def _swap(cfg, key, value):
    """cfg with the value behind option `key` replaced."""
    out = list(cfg)
    out[out.index(key) + 1] = value
    return out


VAD_FEA = "-vad_out_mode vad -vad_cri_mode cepdist -vad_cepdist_mode fea".split()
VAD_ENERGY = "-vad_out_mode vad -vad_cri_mode energy".split()
SIG_SS = "-format_in raw -format_out raw -w 25 -s 12.5".split()

# Same shape and rules as REF_E2E_CASES.  "short3" = the two "short" files with a 300-sample file between them: no frame at 16 kHz (the *ss
# modes and exten carry their state over it, window - shift <= 300 < window), two frames at 8 kHz.
REF_E2E_OPT_CASES = {
    # filter banks
    "bank_bark": (C2 + ["-fb_scale", "bark"], "short"),
    "bank_expolog": (C2 + ["-fb_scale", "expolog"], "short"),
    "bank_lin_rect": (C2 + "-fb_scale lin -fb_shape rect -fb_definition 20filters".split(), "short"),
    "bank_trapez": (C2 + ["-fb_shape", "trapez"], "short"),
    "bank_eqld": (C2 + "-fb_norm off -fb_eqld on".split(), "short"),
    "bank_two_ranges": (C2 + ["-fb_definition", "100-4000Hz:1-10/10filters,4000-8000Hz:3-6/8filters"], "short"),
    "bank_bark_hires": (C2 + "-fb_scale bark -fb_definition 1-30/30filters -fea_ncepcoefs 29 -fea_E on".split(), "short"),
    # feature kinds
    "kind_spec_mag": (C2 + "-fb_power off -fea_kind spec".split(), "short"),
    "kind_logspec_rawe": (C2 + "-fea_kind logspec -fea_E on -fea_rawenergy on".split(), "short"),
    "kind_nolifter_noc0": (C2 + "-fea_lifter 0 -fea_c0 off -fea_ncepcoefs 20".split(), "short"),
    "kind_lpc12": (C2 + "-fea_kind lpc -fea_lporder 12".split(), "short"),
    "kind_lpa": (C3 + ["-fea_kind", "lpa"], "short"),
    "kind_plp23": (C3 + "-fea_lporder 23 -fea_ncepcoefs 23 -fb_definition 30filters".split(), "short"),
    # the 19 one-bark bands of the PLP bank take no count from -fb_definition: order 23 is not below them (the engine refuses that, DESIGN.md
    # section 7, and the oracle is the reference's to the last bit all the same); order 23 on 30 mel bands is the case behind it
    "kind_lpc23_mel30": (("-fs 16000 -format_in raw -format_out htk -preem 0.97 -fb_scale mel -fb_shape triang -fb_norm off -fb_power on -fb_eqld on "
                         "-fb_inld on -fb_definition 30filters -fea_kind lpc -fea_lporder 23 -fea_ncepcoefs 23 -fea_E on").split(), "short"),
    "kind_trapdct51": (C2 + "-fb_definition 23filters -fea_kind trapdct,51,8".split(), "short"),
    "kind_odd_shift": (C2 + ["-s", "10.0625"], "short"),
    # noise reduction, the state carried over a frameless file
    "nr_hwss": (C2 + "-nr_mode hwss -vad burg".split(), "short3"),
    "nr_2fwss": (C2 + "-nr_mode 2fwss -vad burg".split(), "short3"),
    "nr_hwss_8k": (M8 + "-nr_mode hwss -vad burg -nr_a 2".split(), "short3"),
    "nr_fwss_da_zexp_e": (C2 + "-nr_mode fwss -vad burg -fea_delta d_a -fea_Z_exp 300 -fea_E on".split(), "short3"),
    "nr_exten_afterfb": (C2 + "-nr_mode exten -nr_when afterFB".split(), "short3"),
    "nr_dc1_exten": (C2 + "-remove_dc1 on -nr_mode exten".split(), "short3"),
    "sig_hwss": (["-fs", "16000"] + SIG_SS + "-nr_mode hwss -vad burg".split(), "short3"),
    "sig_2fwss_8k": (["-fs", "8000"] + SIG_SS + "-nr_mode 2fwss -vad burg".split(), "short3"),
    "nr_hwss_44k": (M44 + "-nr_mode hwss -vad burg".split(), "short"),
    # the VAD module with its stream
    "vad_c4_perc": (_swap(C4, "-vad_thr_mode", "perc"), "short3"),
    "vad_c4_absolute": (_swap(C4, "-vad_thr_mode", "absolute") + ["-vad_absolute_thr", "6"], "short3"),      # distances there run from 1.9 to 10.3
    "vad_c4_dyn": (_swap(C4, "-vad_thr_mode", "dyn"), "short3"),
    "vad_c4_drop": (C4 + ["-vad_apply_mode", "drop"], "short3"),
    "vad_c4_order7": (C4 + ["-vad_filter_order", "7"], "short3"),
    "vad_c4_zexp": (C4 + ["-fea_Z_exp", "500"], "short3"),
    "vad_fea_adapt": (C2 + VAD_FEA + ["-vad_thr_mode", "adapt"], "short"),
    "vad_fea_dyn_da": (C2 + VAD_FEA + "-vad_thr_mode dyn -fea_delta d_a".split(), "short"),
    "vad_fea_dyn_trap3": (C2 + VAD_FEA + "-vad_thr_mode dyn -fea_trap 3".split(), "short"),
    "vad_fea_adapt_trap9": (C2 + VAD_FEA + "-vad_thr_mode adapt -fea_trap 9".split(), "short"),
    "vad_energy_absolute": (C2 + VAD_ENERGY + "-vad_thr_mode absolute -vad_absolute_thr 96.5".split(), "short"),   # the first file's median
    "vad_energy_perc": (C2 + VAD_ENERGY + ["-vad_thr_mode", "perc"], "short"),
    "vad_energy_adapt_afterfb": (C2 + VAD_ENERGY + "-vad_thr_mode adapt -nr_mode exten -nr_when afterFB".split(), "short"),
    "vad_energy_dyn_64pt": (M8 + "-w 8 -s 4 -fb_definition 1-10/10filters -fea_ncepcoefs 8".split() + VAD_ENERGY + ["-vad_thr_mode", "dyn"], "short"),
    # delta chains of the third order
    "post_dat_windows": (C2 + "-fea_delta d_a_t -d_win 3 -a_win 1 -t_win 2".split(), "short"),
    "post_dat": (C2 + ["-fea_delta", "d_a_t"], "short"),
}


# ---- digital silence through the stateful chains: tests/golden/ref_e2e_silence.npz (make_ref_e2e_fixtures.py silence)
# Same shape and rules as REF_E2E_CASES.  "sil<n>" = zeros_mid(n) (3n/8 speech, n/4 zeros, 3n/8 speech: a muted telephone channel), then
# synth_utt(3, n // 2), which shows what the first file hands on.  An all-zero frame is the logarithm of an empty band in the reference
# (-inf / NaN), and every stage that carries state from frame to frame decides how far that spreads.
REF_E2E_SILENCE_CASES = {
    "sil_c4": (C4, "sil8000"),          # the reference dies on the first silent frame (Burg.h:72, den != 0.0): status only, DESIGN.md section 7
    "sil_c4_novad": (C4_NOVAD, "sil8000"),
    "sil_fwss": (C2 + "-nr_mode fwss -vad burg".split(), "sil12000"),
    "sil_2fwss_8k": (M8 + "-nr_mode 2fwss -vad burg".split(), "sil8000"),
    "sil_hwss_8k": (M8 + "-nr_mode hwss -vad burg".split(), "sil8000"),
    "sil_trapdct51": (C2 + "-fb_definition 23filters -fea_kind trapdct,51,8".split(), "sil16000"),
    "sil_da_zexp_e": (C2 + "-fea_delta d_a -fea_Z_exp 500 -fea_E on".split(), "sil12000"),
    "sil_trap9": (C2 + ["-fea_trap", "9"], "sil12000"),
    "sil_zblock30": (C2 + ["-fea_Z_block", "30"], "sil12000"),
    "sil_vad_energy_dyn": (C2 + VAD_ENERGY + ["-vad_thr_mode", "dyn"], "sil12000"),
    "sil_vad_energy_perc": (C2 + VAD_ENERGY + ["-vad_thr_mode", "perc"], "sil12000"),
    "sil_vad_fea_adapt": (C2 + VAD_FEA + ["-vad_thr_mode", "adapt"], "sil12000"),
    "sil_lpc12": (C2 + "-fea_kind lpc -fea_lporder 12".split(), "sil12000"),
    "sil_plp": (C3 + ["-fb_inld", "off"], "sil12000"),          # the double tail
    "sil_logspec_e": (C2 + "-fea_kind logspec -fea_E on".split(), "sil12000"),
    "sil_spec": (C2 + "-fea_kind spec".split(), "sil12000"),
    "sil_sig_fwss": (REF_E2E_CASES["sig_fwss"][0], "sil12000"),
    "sil_m48_w64": (REF_E2E_CASES["m48_w64"][0], "sil25152"),   # 4096 points; 3072 + 23 x 960 samples: 24 rows, the fewest with ten finite ones on either side
}
SILENCE_DIES = {"sil_c4": 134}


# What the reference does with the first file: (first, last non-finite row, rows); None for the first two where every row is finite, the
# silent frames included (0 is a value to `spec`, and fwss / 2fwss floor what they subtract); hwss leaves empty bands on speech too, so its
# entry is (number of non-finite rows, rows).  The smoothing chains spread the block: trapdct by half its context, -fea_trap and the deltas
# by their windows, and the exponential CMS never recovers.
REF_E2E_SILENCE_NONFINITE = {
    "sil_c4_novad": (38, 60, 98), "sil_fwss": (None, None, 73), "sil_2fwss_8k": (None, None, 98), "sil_hwss_8k": (60, 98),
    "sil_trapdct51": (13, 85, 98), "sil_da_zexp_e": (25, 72, 73), "sil_trap9": (25, 48, 73), "sil_zblock30": (29, 44, 73),
    "sil_vad_energy_dyn": (29, 44, 73), "sil_vad_energy_perc": (29, 44, 73), "sil_vad_fea_adapt": (29, 44, 73), "sil_lpc12": (29, 44, 73),
    "sil_plp": (29, 44, 73), "sil_logspec_e": (29, 44, 73), "sil_spec": (None, None, 73), "sil_m48_w64": (10, 13, 24),
}
SILENCE_VAD_ONES = {"sil_vad_energy_dyn": 31, "sil_vad_energy_perc": 42, "sil_vad_fea_adapt": 18}    # '1' bytes of the first file's 73


def zero_block_frames(cfg, n, rows):
    """Frames of zeros_mid(n) that lie wholly inside the zero block (with pre-emphasis: the sample in front of the frame too)."""
    opt = {k: v for k, v in zip(cfg[:-1], cfg[1:]) if k.startswith("-")}
    fs = int(opt["-fs"])
    window, shift = int(float(opt.get("-w", 25)) * fs / 1000), int(float(opt.get("-s", 10)) * fs / 1000)
    a, z, _ = zeros_mid_parts(n)
    starts = np.arange(rows) * shift
    return (starts - (1 if float(opt.get("-preem", 0)) > 0 else 0) >= a) & (starts + window <= a + z)


def check_silence_conditions(name, cfg, rows0, rows1):
    """What the GPU tests on REF_E2E_SILENCE_CASES rely on in the reference's rows of a case it survives: the recorded non-finite rows of
    the first file, at least 10 finite rows ahead of the block, at least 10 behind it (not sil_da_zexp_e, whose recurrence stays non-finite
    to the end of the file), and a second file that is finite throughout (not under hwss).  The block: the all-zero frames and every
    non-finite row around them (under hwss the all-zero frames alone)."""
    n = int(REF_E2E_SILENCE_CASES[name][1][len("sil"):])
    hwss = "hwss" in cfg
    bad = ~np.isfinite(rows0).all(axis=1)
    idx, rows = np.flatnonzero(bad), rows0.shape[0]
    silent = np.flatnonzero(zero_block_frames(cfg, n, rows))
    assert silent.size >= 2, (name, silent)
    want = REF_E2E_SILENCE_NONFINITE[name]
    if hwss:
        assert (int(bad.sum()), rows) == want and bad[silent].all(), (name, int(bad.sum()), rows)
    elif want[0] is None:
        assert not bad.any() and rows == want[2], (name, idx, rows)
    else:
        assert (int(idx[0]), int(idx[-1]), rows) == want and bad[idx[0]:idx[-1] + 1].all(), (name, idx, rows)
        assert idx[0] <= silent[0] and silent[-1] <= idx[-1], (name, idx, silent)
    lo, hi = int(silent[0]), int(silent[-1])
    if idx.size and not hwss:
        lo, hi = min(lo, int(idx[0])), max(hi, int(idx[-1]))
    ahead, behind = int((~bad[:lo]).sum()), int((~bad[hi + 1:]).sum())
    assert ahead >= 10 and (behind >= 10 or name == "sil_da_zexp_e"), (name, ahead, behind)
    if name == "sil_da_zexp_e":
        assert hi == rows - 1, (name, hi, rows)
    assert rows1.shape[0] >= 10 and (hwss or np.isfinite(rows1).all()), name
    return ahead, behind


def ref_e2e_silence():
    """What the compiled reference wrote for REF_E2E_SILENCE_CASES (make_ref_e2e_fixtures.py silence)."""
    return np.load(os.path.join(GOLDEN, "ref_e2e_silence.npz"))


def g711_codes(n=9000):
    return np.random.default_rng(711).integers(0, 256, size=n, dtype=np.uint8)


def wave_image(x, fs=16000):
    """int16 samples behind the 44-byte RIFF header."""
    import struct
    return (b"RIFF" + struct.pack("<I", 36 + 2 * x.size) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, fs, 2 * fs, 2, 16)
            + b"data" + struct.pack("<I", 2 * x.size) + x.astype("<i2").tobytes())


def _raw_files(utts):
    return {f"in{i}.raw": u.astype("<i2").tobytes() for i, u in enumerate(utts)}


def _no_format_out(cfg):
    i = cfg.index("-format_out")
    return cfg[:i] + cfg[i + 2:]


def ref_e2e_file_cases():
    """Cases whose target is the FILES the reference writes: name -> (command line, {input file: bytes}, list text, output files).  Every path is
    relative: the program runs in the directory that holds the inputs (the ark's .scp names the ark as the command line does)."""
    short = ref_e2e_inputs("short")
    two = "in0.raw out0\nin1.raw out1\n"
    spk3 = [short[0], short[1], synth_utt(7, 9000)]
    cmvn_list = "in0.raw out0 spkA\nin1.raw out1 spkB\nin2.raw out2 spkB\n"
    return {
        "file_ark": (_no_format_out(C2) + ["-format_out", "ark=out.ark"], _raw_files(short), "in0.raw utt0\nin1.raw utt1\n", ["out.ark", "out.scp"]),
        "file_pfile": (_no_format_out(C2) + ["-format_out", "pfile=out.pfile"], _raw_files(short), "in0.raw utt0\nin1.raw utt1\n", ["out.pfile"]),
        "file_big_endian": (C2 + ["-endian_out", "big"], _raw_files(short), two, ["out0", "out1"]),
        "file_cmvn": (C1 + ["-apply_cmvn", "stat"], _raw_files(spk3), cmvn_list, ["stat", "out0", "out1", "out2"]),
        "file_cmvn_da": (C1 + ["-fea_delta", "d_a", "-apply_cmvn", "stat"], _raw_files(spk3), cmvn_list, ["stat", "out0", "out1", "out2"]),
        "file_alaw": (_swap(C2, "-format_in", "alaw"), {"in0.raw": g711_codes().tobytes()}, "in0.raw out0\n", ["out0"]),
        "file_mulaw": (_swap(C2, "-format_in", "mulaw"), {"in0.raw": g711_codes().tobytes()}, "in0.raw out0\n", ["out0"]),
        "file_wave": (_swap(C2, "-format_in", "wave"), {f"in{i}.raw": wave_image(u) for i, u in enumerate(short)}, two, ["out0", "out1"]),
    }


def ref_e2e_opts():
    """What the compiled reference wrote for REF_E2E_OPT_CASES and ref_e2e_file_cases() (make_ref_e2e_fixtures.py opts)."""
    return np.load(os.path.join(GOLDEN, "ref_e2e_opts.npz"))


def split_written_file(name, data, big_endian=False):
    """(float32 rows of every utterance in the file, the file's bytes with those floats zeroed) for what a file case wrote: an HTK file,
    a Kaldi ark (key, " \\0BFM ", \\4 rows \\4 columns, little-endian floats) or a pfile (32768-byte header, rows of two big-endian
    uint32 + floats, sentence index); any other file (.scp, statistics text) has no float payload."""
    data = bytes(data)
    rest = bytearray(data)
    rows = []

    def take(off, n, d, e):
        rows.append(np.frombuffer(data, e + "f4", n * d, off).astype(np.float32).reshape(n, d))
        rest[off:off + 4 * n * d] = bytes(4 * n * d)

    if name.endswith(".ark"):
        off = 0
        while off < len(data):
            off = data.index(b" \0BFM \4", off) + 7
            n = int(np.frombuffer(data, "<i4", 1, off)[0])
            d = int(np.frombuffer(data, "<i4", 1, off + 5)[0])
            assert data[off + 4] == 4
            take(off + 9, n, d, "<")
            off += 9 + 4 * n * d
    elif name.endswith(".pfile"):
        head = data[:32768].split(b"\0")[0].decode()
        field = lambda k: int(head.split(k + " ")[1].split()[0])
        n, d, sents = field("-num_frames"), field("-num_features"), field("-num_sentences")
        table = np.frombuffer(data, ">u4", sents + 1, 32768 + n * (8 + 4 * d))
        body = np.frombuffer(data, ">f4", n * (2 + d), 32768).reshape(n, 2 + d)
        for a, b in zip(table[:-1], table[1:]):
            rows.append(body[a:b, 2:].astype(np.float32))
        mask = np.frombuffer(rest, np.uint8, n * (8 + 4 * d), 32768).reshape(n, 8 + 4 * d)
        mask[:, 8:] = 0
    elif name.startswith("out") and "." not in name:
        e = ">" if big_endian else "<"
        n = int(np.frombuffer(data, e + "u4", 1, 0)[0])
        size = int(np.frombuffer(data, e + "u2", 1, 8)[0])
        assert size % 4 == 0 and len(data) == 12 + n * size, (name, n, size, len(data))
        take(12, n, size // 4, e)
    return rows, bytes(rest)
