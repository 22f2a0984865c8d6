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
    """The files of one input set of REF_E2E_CASES, in list order."""
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
