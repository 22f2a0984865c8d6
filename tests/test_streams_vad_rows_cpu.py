"""Stream sets with detector state behind row state (CTU_STREAMS_VAD_ROW_STATE beside CTU_STREAMS_ROW_STATE and CTU_STREAMS_VAD_STATE: the
VAD module with delta chains, stacking and CMS behind it), the parts that need no GPU: the flag and what it is a flag beside, how the binding passes it, which
configurations such a set takes and with what halo, that without the flag every answer keeps today's words (written out), the
refusals that stand with the flag, the arithmetic of ctu_streams_vad_rows_step against a walk of the exported frame and row counts,
and - on the CPU oracle - what the GPU tests of tests/test_streams_vad_rows.py rest on: the decisions of every configuration hold both
values on the 96-frame signal, and the end of a file changes the last decisions behind a chain.  The set's shape and its push and
finish plans are checked by a program of its own (tests/host/stream_vad_rows_shape_check.cc), built plainly and under Address +
UndefinedBehavior sanitizers."""
import ctypes
import inspect
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import ctucopy_amd
from ctucopy_amd import config_dims, streams_config_check, streams_config_check_ex, streams_rows_step, streams_step, streams_vad_rows_step
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_streams import C2_8K, _signal
from tests.util import C2, C4, C5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSED = "ENGINE: configuration cannot be streamed: "
BURG = "-vad burg -vad_out_mode vad -vad_cri_mode cepdist -vad_cepdist_mode lpc".split()
ENERGY = "-vad_out_mode vad -vad_cri_mode energy".split()
FEA = "-vad_out_mode vad -vad_cri_mode cepdist -vad_cepdist_mode fea".split()
DA = ["-fea_delta", "d_a"]

# name: (command line, delay, largest window, h)
CONFIGS = {
    "energy_dyn_d_a": (C2 + ENERGY + ["-vad_thr_mode", "dyn"] + DA, 4, 2, 1),
    "burg_adapt_d_a": (C2 + BURG + ["-vad_thr_mode", "adapt"] + DA, 4, 2, 1),
    "energy_perc_o7_d_a_t": (C2 + ENERGY + ["-vad_thr_mode", "perc", "-vad_filter_order", "7"] + ["-fea_delta", "d_a_t"], 6, 2, 3),
    "energy_dyn_trap9": (C2 + ENERGY + ["-vad_thr_mode", "dyn"] + ["-fea_trap", "9"], 4, 4, 1),
    "energy_dyn_Zexp": (C2 + ENERGY + ["-vad_thr_mode", "dyn"] + ["-fea_Z_exp", "500"], 0, 0, 1),
    "energy_dyn_Zblock": (C2 + ENERGY + ["-vad_thr_mode", "dyn"] + ["-fea_Z_block", "50"], 0, 0, 1),
    "burg_dyn_d_a_Zexp_8k": (C2_8K + BURG + ["-vad_thr_mode", "dyn"] + DA + ["-fea_Z_exp", "500"], 4, 2, 1),
    "burg_adapt_d_a_o1": (C2 + BURG + ["-vad_thr_mode", "adapt"] + DA + ["-vad_filter_order", "1"], 4, 2, 0),
    "energy_dyn_d_a_E_o1": (C2 + ENERGY + ["-vad_thr_mode", "dyn"] + DA + ["-fea_E", "on", "-vad_filter_order", "1"], 4, 2, 0),
}
C4_ZEXP = C4 + ["-fea_Z_exp", "500"]
THREE = ceng.STREAMS_ROW_STATE | ceng.STREAMS_VAD_STATE | ceng.STREAMS_VAD_ROW_STATE   # 1 | 8 | 16384
NR = ceng.STREAMS_NR_STATE

# the sentences accept.cc gives today for the row state and the detector state without the new flag
TODAY_DELTA = REFUSED + "-fea_delta together with the VAD module (the detector is called when a vector reaches the writer, on frame min(t + H, T - 1))"
TODAY_TRAP = REFUSED + "-fea_trap together with the VAD module (the detector is called when a vector reaches the writer, on frame min(t + H, T - 1))"
TODAY_ZEXP = REFUSED + "-fea_Z_exp together with the VAD module (CMS behind the detector's delayed rows is not carried by a stream set)"
TODAY_ZBLOCK = REFUSED + "-fea_Z_block together with the VAD module (CMS behind the detector's delayed rows is not carried by a stream set)"
TODAY = {"energy_dyn_d_a": TODAY_DELTA, "burg_adapt_d_a": TODAY_DELTA, "energy_perc_o7_d_a_t": TODAY_DELTA, "energy_dyn_trap9": TODAY_TRAP,
         "energy_dyn_Zexp": TODAY_ZEXP, "energy_dyn_Zblock": TODAY_ZBLOCK, "burg_dyn_d_a_Zexp_8k": TODAY_DELTA, "burg_adapt_d_a_o1": TODAY_DELTA,
         "energy_dyn_d_a_E_o1": TODAY_DELTA}
EXTEN_OUTSIDE = REFUSED + ("-nr_mode exten with a VAD criterion outside the fused shapes (25 ms frames at 8 or 16 kHz, the lpc criterion with 14 "
                           "coefficients: the exported spectra are not carried behind exten's state)")


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


def test_library_exports_and_binding_types_the_new_call():
    lib = ctypes.CDLL(cbuild.LIB)
    L = ctucopy_amd.load_library()
    assert hasattr(lib, "ctu_streams_vad_rows_step") and "ctu_streams_vad_rows_step" in ceng.EXPORTS
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    assert L.ctu_streams_vad_rows_step.restype is i64
    assert L.ctu_streams_vad_rows_step.argtypes == [i32, i32, i32, i32, i32, i64, ctypes.POINTER(i64)]
    assert ctucopy_amd.streams_vad_rows_step is ceng.streams_vad_rows_step


def test_the_flag_is_a_bit_of_its_own_and_a_flag_only_beside_the_two():
    V = ceng.STREAMS_VAD_ROW_STATE
    assert V == 16384 and V & (V - 1) == 0
    assert THREE == V | 8 | 1
    L = ctucopy_amd.load_library()
    n, arr = ceng._argv(C2)
    buf = ctypes.create_string_buffer(256)
    for bad in (V, V | 8, V | 1, V | 4, V | 8 | 4):
        assert L.ctu_streams_config_check_ex(n, arr, bad, buf, len(buf), None) == ceng.CTU_ERR_INPUT, bad
        assert buf.value.decode() == "ENGINE: unknown stream set flags"
    for good in (V | 8 | 1, V | 8 | 1 | 4):
        assert L.ctu_streams_config_check_ex(n, arr, good, buf, len(buf), None) == ceng.CTU_OK, good
        assert buf.value.decode() == ""
    for bad in (V, V | 8, V | 1):
        assert streams_config_check_ex(C2, bad) == (ceng.CTU_ERR_INPUT, "ENGINE: unknown stream set flags", 0)


def test_the_binding_takes_the_flags_themselves():
    """The keyword forms keep the signatures tests/test_streams_ss_large_cpu.py pins (ss_large_state last); the new bit has no keyword and
    is given to the forms that take the STREAMS_* bits: streams_config_check_ex, Engine.streams_ex, Streams.with_flags."""
    for f in (ceng._stream_flags, ceng.streams_config_check, ceng.Streams.__init__, ceng.Engine.streams):
        assert "vad_row_state" not in inspect.signature(f).parameters, f
    assert ctucopy_amd.streams_config_check_ex is ceng.streams_config_check_ex
    assert list(inspect.signature(ceng.streams_config_check_ex).parameters) == ["args", "flags"]
    assert list(inspect.signature(ceng.Engine.streams_ex).parameters) == ["self", "n", "max_push", "flags"]
    assert list(inspect.signature(ceng.Streams.with_flags).parameters) == ["engine", "n", "max_push", "flags"]
    cfg = CONFIGS["energy_dyn_d_a"][0]
    assert streams_config_check_ex(cfg, THREE) == (ceng.CTU_OK, "", 5)
    # on the bits the keywords name the two forms give one answer
    assert streams_config_check_ex(cfg, 1 | 8) == streams_config_check(cfg, row_state=True, vad_state=True)
    assert streams_config_check_ex(C2 + DA, 1) == streams_config_check(C2 + DA, row_state=True) == (ceng.CTU_OK, "", 4)
    assert streams_config_check_ex(C2, 0) == streams_config_check(C2) + (0,)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_what_a_set_with_the_three_flags_takes(name):
    cfg, delay, wmax, h = CONFIGS[name]
    order = int(cfg[cfg.index("-vad_filter_order") + 1]) if "-vad_filter_order" in cfg else 3
    assert h == (order - 1) // 2
    assert streams_config_check_ex(cfg, THREE) == (ceng.CTU_OK, "", delay + h)
    assert streams_config_check_ex(cfg, THREE | NR) == (ceng.CTU_OK, "", delay + h)


def test_c4_with_cms_takes_the_noise_state_beside_the_three():
    assert streams_config_check_ex(C4_ZEXP, THREE | NR) == (ceng.CTU_OK, "", 1)
    assert streams_config_check_ex(C4_ZEXP, THREE) == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + "-nr_mode exten (the noise estimate runs from frame to frame of a file)", 0)
    assert streams_config_check(C4_ZEXP, row_state=True, nr_state=True, vad_state=True) == (ceng.CTU_ERR_UNSUPPORTED, TODAY_ZEXP, 0)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_without_the_flag_every_answer_keeps_today_s_words(name):
    cfg = CONFIGS[name][0]
    assert streams_config_check(cfg, row_state=True, vad_state=True) == (ceng.CTU_ERR_UNSUPPORTED, TODAY[name], 0)
    assert streams_config_check(cfg, row_state=True, nr_state=True, vad_state=True) == (ceng.CTU_ERR_UNSUPPORTED, TODAY[name], 0)


def test_without_the_flag_c4_behind_a_chain_keeps_today_s_words():
    assert streams_config_check(C4 + DA, row_state=True, nr_state=True, vad_state=True) == (ceng.CTU_ERR_UNSUPPORTED, TODAY_DELTA, 0)


@pytest.mark.parametrize("cfg, sentence", [
    (C2 + ENERGY + DA + ["-vad_apply_mode", "drop"], "-vad_apply_mode drop (the row count of a push would depend on the data)"),
    (C2 + FEA + DA, "-vad_cepdist_mode fea (the criterion reads finished rows)"),
    (C5 + ENERGY, "-fea_kind trapdct (a vector spans traplen frames)"),
    (C2 + ["-remove_dc1", "on"] + FEA + DA, "-remove_dc1 (a frame's offset stays subtracted from the samples the later frames share with it)"),
    (C2 + ["-w", "40"] + ENERGY + DA,
     "the VAD module on 1024-point and larger frames (-w: a stream set carries the detector behind the 256- and 512-point front end)"),
    (C2 + ENERGY + DA + ["-fea_E", "on"], "-fea_E with the VAD module's majority filter (the offline run shifts the energy column along the file)"),
    (C2 + ENERGY + ["-fea_Z_exp", "500", "-fea_E", "on", "-vad_filter_order", "5"],
     "-fea_E with the VAD module's majority filter (the offline run shifts the energy column along the file)"),
    (C4 + DA, EXTEN_OUTSIDE[len(REFUSED):]),
    (C4 + ["-fea_trap", "9"], EXTEN_OUTSIDE[len(REFUSED):]),
    (C2 + ["-nr_mode", "exten"] + ENERGY + ["-fea_Z_exp", "500"], EXTEN_OUTSIDE[len(REFUSED):]),
], ids=["drop", "fea", "trapdct", "remove_dc1", "1024_points", "fea_E_order3", "fea_E_order5_cms", "c4_d_a", "c4_trap9", "exten_energy_Zexp"])
def test_what_stays_refused_by_name_with_all_four_flags(cfg, sentence):
    assert streams_config_check_ex(cfg, THREE | NR) == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + sentence, 0)


@pytest.mark.parametrize("cfg", [C2, C2 + DA, C2 + ["-fea_Z_exp", "500"], C2 + ENERGY, C2 + BURG + ["-vad_filter_order", "7"], C4, "-fs 16000 -bogus 1".split()],
                         ids=["mfcc", "d_a", "Zexp", "energy_vad", "burg_vad_o7", "c4", "bad_option"])
def test_beside_one_kind_of_state_alone_the_flag_changes_no_answer(cfg):
    for nr in (False, True):
        assert streams_config_check_ex(cfg, THREE | (NR if nr else 0)) == streams_config_check(cfg, row_state=True, nr_state=nr, vad_state=True)


CHAINS = [(4, 2), (6, 2), (4, 4), (0, 0)]


@pytest.mark.parametrize("window", [200, 400])
@pytest.mark.parametrize("order", [1, 3, 7])
def test_vad_rows_step_against_a_walk_of_the_frame_and_row_counts(window, order):
    wshift, h = window * 2 // 5, (order - 1) // 2
    seen = set()
    for H, wmax in CHAINS:
        for total in range(0, window + 19 * wshift + 1, 37):
            F = streams_step(window, wshift, total)[0]
            C = streams_rows_step(window, wshift, H, wmax, total)[0]   # chain rows complete: the detector's calls
            assert C == (F if H == 0 else (max(F - H, 0) if F >= wmax + 2 else 0))
            R = max(C - h, 0)
            assert streams_vad_rows_step(window, wshift, order, H, wmax, total) == (R, F - R), (H, wmax, total)
            seen.add((C > 0, R > 0, F > 0))
    assert {(False, False, True), (True, True, True)} <= seen and ((True, False, True) in seen or h == 0)
    L = ctucopy_amd.load_library()
    for bad in ((0, 80, 3, 4, 2, 10), (200, 0, 3, 4, 2, 10), (200, 201, 3, 4, 2, 10), (200, 80, 0, 4, 2, 10), (200, 80, 32, 4, 2, 10), (200, 80, 3, 4, 2, -1),
                (200, 80, 3, -1, 0, 10), (200, 80, 3, 2, 3, 10), (200, 80, 3, 4, 0, 10)):
        assert L.ctu_streams_vad_rows_step(*bad, None) == ceng.CTU_ERR_INPUT, bad
    assert L.ctu_streams_vad_rows_step(200, 80, 3, 4, 2, 200 + 9 * 80, None) == 5


_ORACLE = {}


def _oracle_vad(cfg, x):
    key = (tuple(cfg), x.tobytes())
    if key not in _ORACLE:
        _ORACLE[key] = Oracle(cfg).process(x, want_vad=True)[1]
    return _ORACLE[key]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_on_the_oracle_the_decisions_of_the_96_frames_hold_both_values(name):
    cfg = CONFIGS[name][0]
    x = _signal(SimpleNamespace(dims=config_dims(cfg)), 96)
    vad = _oracle_vad(cfg, x)
    assert vad.size == 96 and set(np.unique(vad)) == {ord("0"), ord("1")} and np.count_nonzero(np.diff(vad.astype(np.int16))) >= 1


@pytest.mark.parametrize("name, frames, index", [("energy_dyn_d_a", 72, 70), ("burg_adapt_d_a", 72, 70), ("energy_perc_o7_d_a_t", 72, 70),
                                                  ("energy_dyn_d_a", 12, 11), ("energy_perc_o7_d_a_t", 12, 11)])
def test_on_the_oracle_the_end_of_a_file_changes_a_decision_behind_a_chain(name, frames, index):
    """The calls of the last `delay` rows read the last frame's criterion, so a file cut from a longer one does not end in the longer
    one's decisions: what tests/test_streams_vad_rows.py::test_the_end_of_a_file_matters asks of the streamed finish."""
    cfg = CONFIGS[name][0]
    d = config_dims(cfg)
    x = _signal(SimpleNamespace(dims=d), 96)
    whole = _oracle_vad(cfg, x)
    cut = _oracle_vad(cfg, x[:d.window + (frames - 1) * d.wshift + d.wshift // 2].copy())
    assert cut.size == frames and cut[index] != whole[index]


REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_stream_vad_rows_shape_check(tmp_path, sanitize):
    exe = tmp_path / "stream_vad_rows_shape_check"
    csrc = os.path.join(ROOT, "ctucopy_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", *(["-fsanitize=address,undefined"] if sanitize else []), "-I", csrc,
                    os.path.join(ROOT, "tests", "host", "stream_vad_rows_shape_check.cc"), os.path.join(csrc, "opts.cc"), os.path.join(csrc, "design.cc"),
                    "-o", str(exe)], check=True)
    cp = subprocess.run([str(exe)], capture_output=True, text=True)
    print(cp.stdout, cp.stderr)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert cp.stdout.strip().splitlines()[-1].startswith("stream_vad_rows_shape_check ok"), cp.stdout
    assert not any(r in cp.stderr for r in REPORTS), cp.stderr
    assert cp.stderr.strip() == "", cp.stderr
