"""Helpers of the buffer-contract tests (tests/test_device_contracts*.py, tests/test_stream_device_contracts.py): the cases, batches
whose utterances end on every gap width, arenas whose every no-utterance sample is junk, guarded and poisoned device buffers, and
the bit-level predicates the properties are stated in.  No tests here, and no tolerances: include/ctu_engine.h says which bytes a
run may depend on and which it may write, and both are exact."""
import ctypes
from collections import namedtuple

import numpy as np

from tests.test_rows_in_cpu import HTK
from tests.util import C2, C3, C4, C5, M8, M44, REF_E2E_CASES, REF_E2E_OPT_CASES, SIG_EXTEN, SIG_SS, VAD_ENERGY, synth_utt

Case = namedtuple("Case", "cfg kernel flags")

BURG_VAD = "-vad burg -vad_out_mode vad -vad_cri_mode cepdist -vad_cepdist_mode lpc".split()   # tests/test_burg_vad_sizes.py (V)
SIG_PLAIN = "-fs 16000 -format_in raw -format_out raw -nr_mode none -fea_kind none -fb_definition none -w 32 -s 16".split()
CMVN = ["-stat_cmvn", "unused.stat", "-apply_cmvn", "unused.stat"]


def _case(cfg, kernel="frontend_kernel", kind="rows", fs=16000, min_frames=1, ss=False, vad=False, drop=False):
    return Case(list(cfg), kernel, dict(kind=kind, fs=fs, min_frames=min_frames, ss=ss, vad=vad, drop=drop))


# name -> (command line, expected kernel_name() prefix or None, flags).  flags: kind = what a run takes and gives ("rows": PCM in, rows
# out; "signal": PCM in, speech out; "rows_in": feature rows in, rows out; "cmvn": "rows" with ctu_cmvn_apply behind it; "g711":
# ctu_decode_g711), fs = the sampling rate of the inputs, min_frames = the fewest frames a file with frames may have (the delta
# chains: the largest window + 2; stacking likewise; trapdct: (traplen + 1) / 2), ss = the state runs from file to file, vad = a
# byte per frame comes out, drop = -vad_apply_mode drop.
CASES = {
    # the 256- / 512-point front end
    "c2": _case(C2),
    "m8": _case(M8, fs=8000),
    "m8_64pt": _case(REF_E2E_CASES["m8_64pt"][0], fs=8000),
    "c2_odd_hop": _case(REF_E2E_OPT_CASES["kind_odd_shift"][0]),
    # LP tails
    "c3": _case(C3, "frontend_kernel<13, LP, MODE 0, inld, MD>"),
    "c3_inld_off": _case(REF_E2E_CASES["c3_inld_off"][0]),
    # NR / VAD in the front end
    "c2_exten": _case(REF_E2E_CASES["c2_exten"][0]),
    "c4": _case(C4, "frontend_kernel<13, DCTC, MODE 1, exten, MD, VF>", fs=8000, vad=True),
    "c2_silence_energy": _case(REF_E2E_CASES["c2_silence_energy"][0], vad=True, min_frames=4),
    "c2_energy_drop": _case(C2 + VAD_ENERGY + ["-vad_apply_mode", "drop"], vad=True, drop=True),
    # the -remove_dc1 pre-pass
    "c2_dc1": _case(REF_E2E_CASES["c2_dc1"][0]),
    "m44_dc1": _case(M44 + ["-remove_dc1", "on"], "bigfft_kernel<8>", fs=44100),
    # wide / trap / row stages
    "c2_hires": _case(REF_E2E_CASES["c2_hires"][0], "dct_wide_kernel"),
    "c5": _case(C5, min_frames=51),
    "c2_dat_e_zexp": _case(C2 + "-fea_delta d_a_t -fea_E on -fea_Z_exp 500".split(), min_frames=4),
    "c2_trap9": _case(REF_E2E_CASES["c2_trap9"][0], min_frames=6),
    "c2_zblock_30": _case(REF_E2E_CASES["zblock_30"][0]),
    # large FFT
    "c2_w40": _case(REF_E2E_CASES["c2_w40"][0], "wave1k_kernel"),
    "c2_w40_exten": _case(C2 + ["-w", "40", "-nr_mode", "exten"], "wave1k_kernel"),
    "m44": _case(M44, "bigfft_kernel<8>", fs=44100),
    "m44_exten": _case(M44 + ["-nr_mode", "exten"], "bigfft_kernel<8>", fs=44100),
    "m48_w64": _case(REF_E2E_CASES["m48_w64"][0], "bigfft_kernel<16>", fs=48000),
    "m44_burg_vad": _case(M44 + BURG_VAD + ["-vad_thr_mode", "adapt"], "bigfft_kernel<8>", fs=44100, vad=True),
    # hwss / fwss / 2fwss: the state runs from file to file
    "c2_fwss": _case(REF_E2E_CASES["c2_fwss"][0], ss=True),
    "m8_2fwss": _case(M8 + "-nr_mode 2fwss -vad burg".split(), fs=8000, ss=True),
    "m44_hwss": _case(REF_E2E_OPT_CASES["nr_hwss_44k"][0], "bigss_kernel<", fs=44100, ss=True),
    # speech out
    "sig_exten": _case(SIG_EXTEN, kind="signal"),
    "sig_plain": _case(SIG_PLAIN, kind="signal"),
    "sig_fwss": _case(["-fs", "16000"] + SIG_SS + "-nr_mode fwss -vad burg".split(), kind="signal", ss=True),
    "sig_44_exten": _case(REF_E2E_CASES["sig_44_exten"][0], None, kind="signal", fs=44100),
    # others
    "htk_da_zexp": _case(HTK + "-nfeacoefs 13 -fea_delta d_a -fea_Z_exp 500".split(), None, kind="rows_in", min_frames=4),
    "cmvn_c2_d": _case(C2 + ["-fea_delta", "d"] + CMVN, kind="cmvn", min_frames=4),
    "cmvn_c2_d_e": _case(C2 + ["-fea_delta", "d", "-fea_E", "on"] + CMVN, kind="cmvn", min_frames=4),   # (with columns outside the statistics)
    "g711": _case(C2, kind="g711"),
}

PCM_KINDS = ("rows", "signal", "cmvn")
# Cases the oracle takes out of the unused-tail property by name (tests/test_device_contracts_cpu.py), with the reason: none.
P2_EXCLUDED = ()
TARGET = 2   # index of the target utterance in batch_lengths


def frame_counts(tile, min_frames=1):
    """The frame counts of a batch, in order: [1, tile-1, the target's tile+1, 0, 2*tile+1, tile]; counts a chain refuses
    (1 .. min_frames-1) are raised to min_frames, the two-tile utterance and the target stay."""
    want = [1, tile - 1, tile + 1, 0, 2 * tile + 1, tile]
    assert tile + 1 >= min_frames
    return [f if f == 0 or f >= min_frames else min_frames for f in want]


def batch_lengths(dims, tile, min_frames=1):
    """Utterance lengths for frame_counts: (window - wshift) + f * wshift + r with r = wshift - 1 for the target (the largest unused
    tail) and cycling through 0, 1, 7 for the others, so that the starts behind them fall on every gap width pcm_align leaves.
    A chain that starts from rows takes the counts themselves."""
    counts = frame_counts(tile, min_frames)
    if dims.rows_in:
        return counts
    pre, sh = dims.window - dims.wshift, dims.wshift
    out, k = [], 0
    for i, f in enumerate(counts):
        if i == TARGET:
            r = sh - 1
        else:
            r = (0, 1, 7)[k % 3] % sh
            k += 1
        out.append(pre + f * sh + r)
    return out


def num_frames(dims, n):
    """ctu_num_frames by its rule in include/ctu_engine.h."""
    pre = dims.window - dims.wshift
    return -1 if n < pre else (n - pre) // dims.wshift


def covered(dims, n):
    """Samples of a file of n samples that a frame's window covers: window + (frames - 1) * wshift."""
    f = num_frames(dims, n)
    return dims.window + (f - 1) * dims.wshift if f > 0 else 0


def batch_utts(lengths, fs, seed0=100):
    return [synth_utt(seed0 + i, int(n), fs=fs) for i, n in enumerate(lengths)]


class Layout:
    """What junk_arena and own_mask read of a Plan - sample_off and total_samples - from ctu_arena_layout alone (no device)."""

    def __init__(self, lengths):
        from ctucopy_amd import load_library
        ns = np.ascontiguousarray(lengths, dtype=np.int64)
        off = np.zeros(ns.size + 1, dtype=np.int64)
        i64p = ctypes.POINTER(ctypes.c_int64)
        self.total_samples = int(load_library().ctu_arena_layout(ns.ctypes.data_as(i64p), int(ns.size), off.ctypes.data_as(i64p)))
        assert self.total_samples >= 0
        self.sample_off = off


def own_mask(plan, utts, total=None):
    """True where a sample of the arena (`total` samples, default the plan's) belongs to an utterance."""
    m = np.zeros(plan.total_samples if total is None else int(total), dtype=bool)
    for u, off in zip(utts, plan.sample_off[:-1]):
        m[off:off + len(u)] = True
    return m


def junk(n, fill, seed=0):
    """n int16 samples of "zeros", "rails" (+32767 / -32768 alternating per sample) or "random" (seeded, the full int16 range)."""
    if fill == "zeros":
        return np.zeros(n, dtype=np.int16)
    if fill == "rails":
        return np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)
    assert fill == "random", fill
    return np.random.default_rng(4242 + seed).integers(-32768, 32768, n).astype(np.int16)


def junk_arena(plan, utts, fill, total=None, seed=0):
    """Plan.pack's arena with every sample that belongs to no utterance - the head, the gaps, the tail, the slack of a tensor longer
    than total_samples - set by `fill`."""
    total = plan.total_samples if total is None else int(total)
    assert total >= plan.total_samples
    arena = junk(total, fill, seed)
    for u, off in zip(utts, plan.sample_off[:-1]):
        arena[off:off + len(u)] = u
    return arena


# ---- guarded, poisoned buffers
GUARD_ROWS, GUARD_BYTES, GUARD_SAMPLES = 128, 256, 4096   # conditions, not measurements
POISON = {"float32": (0x7FC0DEAD, 0x7FC0BEEF), "uint8": (0xA5, 0x5A), "int16": (0x5A5A, -0x5A5B)}


def _dtype_name(dtype):
    return str(dtype).split(".")[-1]


def guarded(shape, dtype, guard, poison, device="cuda"):
    """(whole, view): one tensor with `guard` rows (elements, for a 1-d shape) of `poison` on both sides of `view`, which has
    `shape` and is poisoned too.  A guard is a multiple of 64 bytes, so the view keeps the base alignment of a plain allocation."""
    import torch
    shape = tuple(int(x) for x in np.atleast_1d(shape))
    row = int(np.prod(shape[1:]))
    g, n = int(guard) * row, int(np.prod(shape))
    item = {"float32": 4, "uint8": 1, "int16": 2}[_dtype_name(dtype)]
    assert (g * item) % 64 == 0, "guards are multiples of 64 bytes"
    if dtype == torch.float32:
        whole = torch.full((2 * g + n,), int(np.array(poison, np.uint32).view(np.int32)), dtype=torch.int32, device=device).view(torch.float32)
    else:
        whole = torch.full((2 * g + n,), int(poison), dtype=dtype, device=device)
    return whole, whole[g:g + n].view(shape)


def bits(x):
    """x (numpy or torch, any device) as a numpy array of integers: float32 through its int32 view."""
    if not isinstance(x, np.ndarray):
        x = x.detach().cpu().numpy()
    return x.view(np.int32) if x.dtype == np.float32 else x


def bits_equal(x, y):
    """Shape, dtype and integer view equal: NaN and -inf rows are equal when their bits are."""
    a, b = bits(x), bits(y)
    return _dtype_name(x.dtype) == _dtype_name(y.dtype) and a.shape == b.shape and bool(np.array_equal(a, b))


def _word(p, like):
    return np.array(p).astype(np.uint32).astype(np.int32) if like.dtype == np.int32 else np.array(p).astype(like.dtype)


def untouched(a, b, pa, pb):
    """Mask of the words left alone by the same run into two buffers poisoned with pa and pb: each still holds its poison."""
    a, b = bits(a), bits(b)
    return (a == _word(pa, a)) & (b == _word(pb, b))


def written(a, b):
    """Mask of the words that run wrote: the two runs agree on them (the poisons differ, so a word left alone does not)."""
    return bits(a) == bits(b)


def guards_intact(whole, view, poison):
    """Both guards of a guarded() pair still hold `poison`."""
    w = bits(whole).reshape(-1)
    g = (w.size - view.numel()) // 2
    p = _word(poison, w)
    return bool(np.all(w[:g] == p)) and bool(np.all(w[w.size - g:] == p))
