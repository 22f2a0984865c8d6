"""Stream sets with trap state (CTU_STREAMS_TRAP_STATE: the log-mel context of -fea_kind trapdct kept per stream), the parts that need
no GPU: the flag's value, which configurations such a set takes and with which halo, what it still refuses by name, that without the
flag every answer keeps the words it had, that on another feature kind the flag changes no answer, the row counts against the oracle,
and the column table of stream_trap_kernel (tests/host/stream_trap_plan_check.cc, a program of its own under sanitizers).

The answers "without the flag" are written out here from the words tests/test_streams_cpu.py, tests/test_streams_rows_cpu.py,
tests/test_streams_vad_cpu.py and tests/golden/host_tables.json pin, not taken from the code under test."""
import ctypes
import itertools
import os
import subprocess

import pytest

import ctucopy_amd
from ctucopy_amd import config_dims, streams_config_check, streams_rows_step
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.util import C2, C3, C5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error")
TRAP = 256
UNKNOWN = (ceng.CTU_ERR_INPUT, "ENGINE: unknown stream set flags")
REFUSED = "ENGINE: configuration cannot be streamed: "
WORDS_TRAP = REFUSED + "-fea_kind trapdct (a vector spans traplen frames)"   # tests/golden/host_tables.json, flags 0 and 8
WORDS_EXTEN = REFUSED + "-nr_mode exten (the noise estimate runs from frame to frame of a file)"
T31 = ["-fea_kind", "trapdct,31,8"]
ENERGY = "-vad_out_mode vad -vad_cri_mode energy".split()
# the trapdct lines of the three files named above
C5_ROWS = C2 + ["-fb_definition", "23filters", "-fea_kind", "trapdct,101,16"]
C5_VAD = "-fs 16000 -format_in raw -format_out htk -preset mfcc -fb_definition 23filters -fea_kind trapdct,101,16".split() + ENERGY


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


def _check(cfg, flags):
    L = ctucopy_amd.load_library()
    n, arr = ceng._argv(cfg)
    buf = ctypes.create_string_buffer(1024)
    halo = ctypes.c_int32(-1)
    rc = L.ctu_streams_config_check_ex(n, arr, flags, buf, len(buf), ctypes.byref(halo))
    return int(rc), buf.value.decode(), int(halo.value)


def _subsets(bits):
    return [sum(c) for k in range(len(bits) + 1) for c in itertools.combinations(bits, k)]


def test_the_flag_is_256_and_2_16_and_128_stay_no_flags():
    assert ceng.STREAMS_TRAP_STATE == TRAP == 256
    assert (ceng.STREAMS_ROW_STATE, ceng.STREAMS_NR_STATE, ceng.STREAMS_VAD_STATE, ceng.STREAMS_SIGNAL_STATE, ceng.STREAMS_LARGE_STATE) == (1, 4, 8, 32, 64)
    for cfg in (C2, C5, C2 + T31):
        assert "unknown stream set flags" not in _check(cfg, TRAP)[1], cfg
        for bad in (2, 16, 128, 2 | TRAP, 16 | TRAP, 128 | TRAP, 512, 512 | TRAP):
            assert _check(cfg, bad)[:2] == UNKNOWN, (cfg, bad)
        # 64 is a flag only beside the noise state or the signal state: the trap state is neither
        for alone in (64, 64 | TRAP, 64 | TRAP | 1, 64 | TRAP | 8):
            assert _check(cfg, alone)[:2] == UNKNOWN, (cfg, alone)
        for beside in (64 | 4 | TRAP, 64 | 32 | TRAP):
            assert "unknown stream set flags" not in _check(cfg, beside)[1], (cfg, beside)


@pytest.mark.parametrize("cfg, flags, halo", [
    (C5, TRAP, 50), (C5, TRAP | 4, 50),
    (C2 + T31, TRAP, 15), (C2 + T31, TRAP | 4, 15),
    (C2 + ["-w", "40"] + T31, TRAP, 15), (C2 + ["-w", "40"] + T31, TRAP | 4, 15),
    (C2 + ["-nr_mode", "exten"] + T31, TRAP | 4, 15),
    (C2 + ["-nr_mode", "exten", "-w", "40"] + T31, TRAP | 4 | 64, 15),
    ("-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97".split() + T31, TRAP, 15),
], ids=["C5", "C5_nr", "31_8", "31_8_nr", "1024", "1024_nr", "exten", "exten_1024_large", "2048"])
def test_trapdct_is_taken_with_half_a_context_as_the_halo(cfg, flags, halo):
    assert _check(cfg, flags) == (ceng.CTU_OK, "", halo)
    # ... whatever other flags come with it (the detector and signal flags change nothing on a configuration without either)
    assert _check(cfg, flags | 1 | 8 | 32) == (ceng.CTU_OK, "", halo)


def test_the_binding_answers_with_the_halo_as_row_state_does():
    assert streams_config_check(C5, trap_state=True) == (ceng.CTU_OK, "", 50)
    assert streams_config_check(C2 + T31, trap_state=True, nr_state=True) == (ceng.CTU_OK, "", 15)
    assert streams_config_check(C2, trap_state=True) == (ceng.CTU_OK, "", 0)
    assert streams_config_check(C5) == (ceng.CTU_ERR_UNSUPPORTED, WORDS_TRAP)
    assert streams_config_check(C5, row_state=True) == (ceng.CTU_ERR_UNSUPPORTED, WORDS_TRAP, 0)
    assert ceng._stream_flags(False, False, False, trap_state=True) == 256
    assert ceng._stream_flags(True, True, True, True, True, True) == 1 | 4 | 8 | 32 | 64 | 256


def test_exten_needs_the_noise_state_beside_it():
    cfg = C2 + ["-nr_mode", "exten"] + T31
    assert _check(cfg, TRAP) == (ceng.CTU_ERR_UNSUPPORTED, WORDS_EXTEN, 0)   # today's words for exten without its flag
    assert _check(cfg, TRAP | 1)[:2] == (ceng.CTU_ERR_UNSUPPORTED, WORDS_EXTEN)
    big = C2 + ["-nr_mode", "exten", "-w", "40"] + T31
    rc, why, _ = _check(big, TRAP | 4)
    assert rc == ceng.CTU_ERR_UNSUPPORTED and why.startswith(REFUSED + "-nr_mode exten on 1024-point frames")


def test_without_the_flag_every_answer_is_the_one_it_was():
    # trapdct alone: no other flag bears on it, and the sentence is the one pinned for flags 0
    for cfg in (C5, C5_ROWS, C2 + T31, C2 + ["-w", "40"] + T31):
        for flags in _subsets([1, 4, 8, 32]):
            assert _check(cfg, flags) == (ceng.CTU_ERR_UNSUPPORTED, WORDS_TRAP, 0), (cfg, flags)
    # trapdct beside the VAD module: the module's refusal without the detector flag, the trapdct sentence (pinned for flags 8) with it
    for flags in _subsets([1, 4, 8, 32]):
        rc, why, halo = _check(C5_VAD, flags)
        assert rc == ceng.CTU_ERR_UNSUPPORTED and halo == 0 and why.startswith(REFUSED), flags
        if flags & 8:
            assert why == WORDS_TRAP, flags
        else:
            assert why.startswith(REFUSED + "the VAD module (-vad_apply_mode / -vad_out_mode"), flags
    # behind exten: exten's words without the noise flag, trapdct's with it
    for flags in _subsets([1, 4, 8, 32]):
        assert _check(C2 + ["-nr_mode", "exten"] + T31, flags) == (ceng.CTU_ERR_UNSUPPORTED, WORDS_TRAP if flags & 4 else WORDS_EXTEN, 0), flags


@pytest.mark.parametrize("cfg", [C2, C2 + ["-fea_delta", "d_a"], C3], ids=["C2", "C2_d_a", "C3"])
def test_on_another_feature_kind_the_flag_changes_no_answer(cfg):
    for flags in _subsets([1, 4, 8, 32]) + [64 | 4, 64 | 32, 64 | 4 | 32 | 1 | 8]:
        assert _check(cfg, flags | TRAP) == _check(cfg, flags), flags
    assert _check(C2 + ["-fea_delta", "d_a"], TRAP | 1) == (ceng.CTU_OK, "", 4)   # the chain's halo, not the flag's


@pytest.mark.parametrize("cfg, flags, word", [
    (C5_VAD, TRAP | 8, "-fea_kind trapdct (a vector spans traplen frames)"),
    (C2 + T31 + ENERGY, TRAP | 8, "-fea_kind trapdct (a vector spans traplen frames)"),
    (C2 + T31 + ENERGY, TRAP, "the VAD module"),
    (C5 + ["-remove_dc1", "on"], TRAP, "-remove_dc1"),
    (C2 + T31 + ["-nr_mode", "exten", "-nr_when", "afterFB"], TRAP | 4, "-nr_when afterFB"),
    (C2 + T31 + ["-s", "30"], TRAP, "-s above -w"),
], ids=["C5_vad", "31_8_vad", "vad_without_its_flag", "remove_dc1", "exten_afterFB", "s_above_w"])
def test_what_stays_refused_with_the_flag_by_the_names_it_has(cfg, flags, word):
    rc, why, halo = _check(cfg, flags)
    assert rc == ceng.CTU_ERR_UNSUPPORTED and halo == 0 and why.startswith(REFUSED) and word in why, why
    assert _check(cfg, flags & ~TRAP)[0] == ceng.CTU_ERR_UNSUPPORTED


@pytest.mark.parametrize("cfg, word", [
    (C5 + ["-nr_mode", "fwss", "-vad", "burg"], "hwss / fwss / 2fwss"),
    (C5 + ["-stat_cmvn", "stat.txt"], "CMVN"),
], ids=["fwss_burg", "stat_cmvn"])
def test_what_the_engine_refuses_for_trapdct_keeps_the_engine_s_words(cfg, word):
    """hwss / fwss / 2fwss and CMVN on trapdct are outside what ctu_engine_create accepts, so the words are unsupported_reason's, ahead
    of anything a stream set is asked - with the flag as without."""
    got = _check(cfg, TRAP | 4)
    assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[2] == 0 and word in got[1], got
    assert got == _check(cfg, 4)


@pytest.mark.parametrize("half", [1, 15, 50, 127])
def test_rows_delivered_and_held_back_against_the_oracle(half):
    cfg = C2 + ["-fb_definition", "23filters", "-fea_kind", "trapdct,%d,%d" % (2 * half + 1, min(2 * half, 16))]
    assert _check(cfg, TRAP) == (ceng.CTU_OK, "", half)
    d = config_dims(cfg)
    w, s = d.window, d.wshift
    orc = Oracle(cfg)

    def check(n):
        rows, pending = streams_rows_step(w, s, half, half - 1, n)
        F = max(orc.num_frames(n), 0)
        assert rows + pending == F, n
        assert rows == (F - half if F >= half + 1 else 0), n   # trapdct's rule: a file of 1 .. half frames has no defined rows
        return rows

    edge = [0, 1, w - s - 1, w - s, w - 1, w, w + 1, 100 * w + 17]
    for f in (1, half, half + 1, half + 2, 2 * half + 1):   # the sample that completes frame f, and its neighbours
        edge += [w + (f - 1) * s - 1, w + (f - 1) * s, w + (f - 1) * s + 1]
    for n in edge:
        if n >= 0:
            check(n)
    last = 0
    for total in range(w + (half - 2) * s, w + (half + 3) * s):   # sample by sample across the frame that lets the first row out
        if total >= 0:
            now = check(total)
            assert now >= last
            last = now


def test_stream_trap_plan_check_under_sanitizers(tmp_path):
    exe = tmp_path / "stream_trap_plan_check"
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "ctucopy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "stream_trap_plan_check.cc"), "-o", str(exe)], check=True)
    cp = subprocess.run([str(exe)], capture_output=True, text=True)
    print(cp.stdout, cp.stderr)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert cp.stdout.strip().splitlines()[-1].startswith("stream_trap_plan_check ok"), cp.stdout
    assert not any(r in cp.stderr for r in REPORTS), cp.stderr
    assert cp.stderr.strip() == "", cp.stderr
