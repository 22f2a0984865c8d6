"""Stream sets with detector state (CTU_STREAMS_VAD_STATE), the parts that need no GPU: the exported symbols, which configurations
with the VAD module such a set takes, which it refuses and with what words, that the flag changes no other answer, the arithmetic of
the rows and decisions a stream has delivered against the oracle's frame count, and - on the CPU oracle - the property the feature
rests on: the detector is causal, so the decisions and rows of a file's prefix are those of the whole file, h = (order - 1) / 2
frames late, and a file of h frames writes nothing.  The planner's VAD descriptors are checked by a program of its own
(tests/host/stream_vad_plan_check.cc) under Address + UndefinedBehavior sanitizers."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import ctucopy_amd
from ctucopy_amd import config_dims, streams_config_check, streams_vad_step
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_streams import _signal
from tests.util import C2, C3, C4, _swap, synth_utt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSED = "ENGINE: configuration cannot be streamed: "
SYMBOLS = ("ctu_streams_push_vad", "ctu_streams_push_vad_host", "ctu_streams_finish_vad", "ctu_streams_finish_vad_host", "ctu_streams_vad_step")
BURG = "-vad burg -vad_out_mode vad -vad_cri_mode cepdist -vad_cepdist_mode lpc".split()
ENERGY = "-vad_out_mode vad -vad_cri_mode energy".split()
TODAY = REFUSED + "the VAD module (-vad_apply_mode / -vad_out_mode: thresholds and the majority filter run along the file)"

# (command line, also needs nr_state)
ACCEPTED = {
    "c4_adapt": (C4, True),
    "c4_dyn": (_swap(C4, "-vad_thr_mode", "dyn"), True),
    "c4_perc": (_swap(C4, "-vad_thr_mode", "perc"), True),
    "c4_absolute": (_swap(C4, "-vad_thr_mode", "absolute") + ["-vad_absolute_thr", "6"], True),
    "c4_order7": (C4 + ["-vad_filter_order", "7"], True),
    "c4_order31": (C4 + ["-vad_filter_order", "31"], True),
    "mfcc_burg_adapt_512": (C2 + BURG + ["-vad_thr_mode", "adapt"], False),
    "mfcc_burg_dyn_w20": (C2 + ["-w", "20"] + BURG + ["-vad_thr_mode", "dyn"], False),
    "mfcc_burg_20_coefs": (C2 + BURG + ["-vad_thr_mode", "adapt", "-vad_lpc_coefs", "20"], False),
    "mfcc_energy_dyn": (C2 + ENERGY + ["-vad_thr_mode", "dyn"], False),
    "mfcc_energy_perc_order5": (C2 + ENERGY + ["-vad_thr_mode", "perc", "-vad_filter_order", "5"], False),
    "mfcc_energy_order1": (C2 + ENERGY + ["-vad_thr_mode", "adapt", "-vad_filter_order", "1"], False),
    "energy_silence": (C2 + ENERGY + ["-vad_thr_mode", "dyn", "-vad_apply_mode", "silence"], False),
    "energy_fea_E_order1": (C2 + ENERGY + ["-vad_thr_mode", "dyn", "-fea_E", "on", "-vad_filter_order", "1"], False),
    "plp_energy": (C3 + ENERGY + ["-vad_thr_mode", "adapt"], False),
    "64_points_burg": ("-fs 8000 -format_in raw -format_out htk -preset mfcc -w 8 -s 4 -fb_definition 1-10/10filters -fea_ncepcoefs 8".split()
                       + BURG + ["-vad_thr_mode", "dyn"], False),
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


def test_library_exports_and_binding_types_the_new_calls():
    lib = ctypes.CDLL(cbuild.LIB)
    L = ctucopy_amd.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in ceng.EXPORTS
        assert getattr(L, name).argtypes, name
    assert L.ctu_streams_vad_step.restype is ctypes.c_int64


def test_the_flag_is_a_bit_of_its_own_and_two_stays_no_flag():
    flags = (ceng.STREAMS_ROW_STATE, ceng.STREAMS_NR_STATE, ceng.STREAMS_VAD_STATE)
    assert ceng.STREAMS_VAD_STATE == 8 and len(set(flags)) == 3 and sum(flags) == 13
    assert all(f & (f - 1) == 0 for f in flags)
    L = ctucopy_amd.load_library()
    n, arr = ceng._argv(C2)
    buf = ctypes.create_string_buffer(256)
    for bad in (2, 2 | 8, 16):
        assert L.ctu_streams_config_check_ex(n, arr, bad, buf, len(buf), None) == ceng.CTU_ERR_INPUT
        assert "unknown stream set flags" in buf.value.decode()


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_what_a_set_with_detector_state_takes(name):
    cfg, exten = ACCEPTED[name]
    order = int(cfg[cfg.index("-vad_filter_order") + 1]) if "-vad_filter_order" in cfg else 3
    assert streams_config_check(cfg, nr_state=exten, vad_state=True) == (ceng.CTU_OK, "")
    # with row state the answer carries the halo: the majority filter's delay
    assert streams_config_check(cfg, row_state=True, nr_state=exten, vad_state=True) == (ceng.CTU_OK, "", (order - 1) // 2)
    # without the flag: today's words, whatever the other flags
    for kw in ({}, {"row_state": True}):
        got = streams_config_check(cfg, nr_state=exten, **kw)
        assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[1] == TODAY, got


def test_c4_needs_the_noise_state_as_well():
    got = streams_config_check(C4, vad_state=True)
    assert got == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + "-nr_mode exten (the noise estimate runs from frame to frame of a file)")
    assert streams_config_check(C4, nr_state=True) == (ceng.CTU_ERR_UNSUPPORTED, TODAY)


@pytest.mark.parametrize("cfg, exten, words", [
    (C2 + ENERGY + ["-vad_apply_mode", "drop"], False, ["-vad_apply_mode drop"]),
    (C2 + "-vad_out_mode vad -vad_cri_mode cepdist -vad_cepdist_mode fea".split(), False, ["-vad_cepdist_mode fea"]),
    (C2 + ENERGY + ["-fea_delta", "d_a"], False, ["-fea_delta", "VAD module"]),
    (C2 + ENERGY + ["-fea_trap", "3"], False, ["-fea_trap", "VAD module"]),
    (C2 + ENERGY + ["-fea_Z_exp", "500"], False, ["-fea_Z_exp", "VAD module"]),
    (C2 + ENERGY + ["-fea_Z_block", "50"], False, ["-fea_Z_block", "VAD module"]),
    (C2 + ENERGY + ["-fea_E", "on"], False, ["-fea_E"]),
    (C2 + ["-w", "40"] + ENERGY, False, ["1024-point"]),
    ("-fs 44100 -format_in raw -format_out htk -preset mfcc".split() + BURG, False, ["1024-point"]),
    (C2 + ["-nr_mode", "exten"] + ENERGY, True, ["-nr_mode exten"]),
    (C2 + ["-nr_mode", "exten", "-w", "20"] + BURG, True, ["-nr_mode exten"]),
    (C2 + ["-nr_mode", "exten", "-vad_lpc_coefs", "12"] + BURG, True, ["-nr_mode exten"]),
    (C2 + ["-remove_dc1", "on"] + "-vad_out_mode vad -vad_cri_mode cepdist -vad_cepdist_mode fea".split(), False, ["-remove_dc1"]),
    ("-fs 16000 -format_in raw -format_out htk -preset mfcc -fb_definition 23filters -fea_kind trapdct,101,16".split() + ENERGY, False, ["trapdct"]),
], ids=["drop", "fea", "delta", "stacking", "Zexp", "Zblock", "fea_E_shifted", "1024_energy", "2048_burg", "exten_energy", "exten_burg_w20",
        "exten_burg_12_coefs", "remove_dc1", "trapdct"])
def test_what_it_refuses_by_name_whatever_the_flags(cfg, exten, words):
    for row_state in (False, True):
        got = streams_config_check(cfg, row_state=row_state, nr_state=exten, vad_state=True)
        assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[1].startswith(REFUSED), got
        for w in words:
            assert w in got[1], got
    got = streams_config_check(cfg, row_state=True, nr_state=True, vad_state=True)
    assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[1].startswith(REFUSED) and got[2] == 0, got


@pytest.mark.parametrize("cfg", [C2, C3, C2 + ["-fea_delta", "d_a"], C2 + ["-nr_mode", "exten"], C2 + ["-w", "40"], "-fs 16000 -bogus 1".split()],
                         ids=["mfcc", "plp", "d_a", "exten", "1024", "bad_option"])
def test_without_the_vad_module_the_flag_changes_no_answer(cfg):
    assert streams_config_check(cfg, vad_state=True) == streams_config_check(cfg)
    assert streams_config_check(cfg, row_state=True, vad_state=True) == streams_config_check(cfg, row_state=True)
    assert streams_config_check(cfg, nr_state=True, vad_state=True) == streams_config_check(cfg, nr_state=True)
    assert streams_config_check(cfg, row_state=True, nr_state=True, vad_state=True) == streams_config_check(cfg, row_state=True, nr_state=True)


@pytest.mark.parametrize("order", [1, 2, 3, 7, 31])
def test_vad_step_one_sample_at_a_time_against_the_oracle(order):
    cfg = "-fs 8000 -format_in raw -format_out htk -preset mfcc".split()
    d = config_dims(cfg)
    orc = Oracle(cfg)
    h = (order - 1) // 2
    seen_held, seen_out = False, False
    for total in range(0, d.window + 40 * d.wshift + 3):
        F = max(orc.num_frames(total), 0)
        rows, pending = streams_vad_step(d.window, d.wshift, order, total)
        assert rows + pending == F, (order, total)
        assert rows == (F - h if F > h else 0), (order, total)
        seen_held |= 0 < F <= h and rows == 0
        seen_out |= rows > 0
    assert seen_out and (seen_held or h == 0)
    L = ctucopy_amd.load_library()
    for bad in ((0, 80, 3, 10), (200, 0, 3, 10), (200, 201, 3, 10), (200, 80, 0, 10), (200, 80, 32, 10), (200, 80, 3, -1)):
        assert L.ctu_streams_vad_step(*bad, None) == ceng.CTU_ERR_INPUT


PROBED = {
    "c4_adapt": C4,
    "c4_dyn": _swap(C4, "-vad_thr_mode", "dyn"),
    "c4_perc": _swap(C4, "-vad_thr_mode", "perc"),
    "c4_absolute": _swap(C4, "-vad_thr_mode", "absolute") + ["-vad_absolute_thr", "6"],
    "c4_order7": C4 + ["-vad_filter_order", "7"],
    "mfcc_burg_adapt": C2 + BURG + ["-vad_thr_mode", "adapt"],
    "mfcc_energy_dyn": C2 + ENERGY + ["-vad_thr_mode", "dyn"],
    "energy_order1": C2 + ENERGY + ["-vad_thr_mode", "adapt", "-vad_filter_order", "1"],
}


@pytest.mark.parametrize("name", list(PROBED))
def test_on_the_oracle_a_prefix_has_the_file_s_decisions_and_a_file_of_h_frames_writes_nothing(name):
    cfg = PROBED[name]
    order = int(cfg[cfg.index("-vad_filter_order") + 1]) if "-vad_filter_order" in cfg else 3
    h = (order - 1) // 2
    d = config_dims(cfg)
    orc = Oracle(cfg)
    for x in (_signal(SimpleNamespace(dims=d), 96), synth_utt(31, d.window + 95 * d.wshift + 9, fs=d.fs)):
        rows, vad = orc.process(x, want_vad=True)
        assert rows.shape[0] == 96 and vad.size == 96 and set(np.unique(vad)) <= {ord("0"), ord("1")}
        prows, pvad = orc.process(x[:d.window + 40 * d.wshift], want_vad=True)   # 41 frames
        assert prows.shape[0] == 41 and pvad.size == 41
        assert np.array_equal(pvad[:41 - h], vad[:41 - h])   # decisions 0 .. F - h - 1: what a stream has delivered after F frames
        assert np.array_equal(prows, rows[:41])
        if h:
            srows, svad = orc.process(x[:d.window + (h - 1) * d.wshift], want_vad=True)   # h frames
            assert orc.num_frames(d.window + (h - 1) * d.wshift) == h and srows.shape[0] == 0 and svad.size == 0


REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error")


def test_stream_vad_plan_check_under_sanitizers(tmp_path):
    exe = tmp_path / "stream_vad_plan_check"
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "ctucopy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "stream_vad_plan_check.cc"), "-o", str(exe)], check=True)
    cp = subprocess.run([str(exe)], capture_output=True, text=True)
    print(cp.stdout, cp.stderr)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert cp.stdout.strip().splitlines()[-1].startswith("stream_vad_plan_check ok"), cp.stdout
    assert not any(r in cp.stderr for r in REPORTS), cp.stderr
    assert cp.stderr.strip() == "", cp.stderr
