"""Stream sets with row state (CTU_STREAMS_ROW_STATE), the parts that need no GPU: the exported symbols, which configurations such
a set takes and with what halo, which it still refuses and with what words, and the arithmetic of the rows a stream has delivered
and holds back against the oracle's frame count."""
import ctypes

import pytest

import ctucopy_amd
from ctucopy_amd import CtuError, config_dims, streams_config_check, streams_rows_step
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.util import C2, C3

C2_8K = "-fs 8000 -format_in raw -format_out htk -preset mfcc -preem 0.97".split()
SYMBOLS = ("ctu_streams_create_ex", "ctu_streams_config_check_ex", "ctu_streams_pending", "ctu_streams_finish_host", "ctu_streams_rows_step")


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
    assert L.ctu_streams_pending.restype is ctypes.c_int64 and L.ctu_streams_rows_step.restype is ctypes.c_int64
    assert ceng.STREAMS_ROW_STATE == 1
    assert callable(ctucopy_amd.Streams.pending) and callable(ctucopy_amd.streams_rows_step)


@pytest.mark.parametrize("extra, halo", [
    (["-fea_delta", "d_a"], 4),
    (["-fea_delta", "d_a_t", "-d_win", "3", "-a_win", "1", "-t_win", "2"], 6),
    (["-fea_trap", "9"], 4),
    (["-fea_Z_exp", "500"], 0),
    (["-fea_Z_block", "300", "-fea_delta", "d_a"], 4),
    ([], 0),
])
def test_chains_a_set_with_row_state_takes_and_their_halo(extra, halo):
    assert streams_config_check(C2 + extra, row_state=True) == (ceng.CTU_OK, "", halo)


def test_without_the_flag_the_answer_is_the_old_one():
    rc, why = streams_config_check(C2 + ["-fea_delta", "d_a"])
    assert rc == ceng.CTU_ERR_UNSUPPORTED and "-fea_delta" in why
    assert streams_config_check(C2) == (ceng.CTU_OK, "")


@pytest.mark.parametrize("cfg, word", [
    (C2 + ["-nr_mode", "exten"], "-nr_mode exten"),
    (C2 + ["-vad_out_mode", "vad", "-vad_out", "x.vad"], "VAD module"),
    (C2 + ["-vad_apply_mode", "silence"], "VAD module"),
    (C2 + ["-remove_dc1", "on"], "-remove_dc1"),
    (C2 + ["-fb_definition", "23filters", "-fea_kind", "trapdct,101,16"], "trapdct"),
    (C2 + ["-stat_cmvn", "stat.txt"], "-stat_cmvn"),
    ("-fs 16000 -format_in raw -format_out raw -preset exten".split(), "-format_out raw"),
    ("-fs 16000 -format_in htk -format_out htk -preset mfcc -fea_rawenergy on -nfeacoefs 13".split(), "-format_in htk"),
])
def test_what_a_set_with_row_state_still_refuses_by_name(cfg, word):
    rc, why, halo = streams_config_check(cfg, row_state=True)
    assert rc == ceng.CTU_ERR_UNSUPPORTED and halo == 0
    assert why.startswith("ENGINE: configuration cannot be streamed: ") and word in why, why


def test_the_offline_limits_keep_the_engine_s_words():
    rc, why, _ = streams_config_check(C2 + ["-fea_trap", "5", "-fea_Z_exp", "500"], row_state=True)
    assert rc == ceng.CTU_ERR_UNSUPPORTED and why.startswith("ENGINE: configuration not on the accelerated path: ") and "CMS on stacked vectors" in why
    rc, why, _ = streams_config_check("-fs 16000 -bogus 1".split(), row_state=True)
    assert rc == ceng.CTU_ERR_OPTS and "Syntax error" in why


@pytest.mark.parametrize("cfg, halo, wmax", [(C2, 4, 2), (C2, 6, 3), (C2_8K, 3, 1), (C2 + ["-s", "10.0625"], 4, 4), (C3, 0, 0)])
def test_rows_delivered_and_held_back_against_the_oracle(cfg, halo, wmax):
    d = config_dims(cfg)
    w, s = d.window, d.wshift
    orc = Oracle(cfg)

    def check(n):
        rows, pending = streams_rows_step(w, s, halo, wmax, n)
        F = max(orc.num_frames(n), 0)
        assert rows + pending == F, n
        if halo == 0:
            assert rows == F, n
        elif F < wmax + 2:
            assert rows == 0, n                     # a file that may still end here has no defined rows
        else:
            assert rows == max(F - halo, 0), n      # the rows no later frame can change
        return rows

    edge = [0, 1, w - s - 1, w - s, w - 1, w, w + 1, 100 * w + 17]
    for f in (1, wmax, wmax + 1, wmax + 2, wmax + 3, halo, halo + 1, halo + 2, 2 * halo + 1):  # the sample that completes frame f, and its neighbours
        edge += [w + (f - 1) * s - 1, w + (f - 1) * s, w + (f - 1) * s + 1]
    for n in edge:
        if n >= 0:
            check(n)
    # the count does not depend on how the samples came (one at a time is the extreme), and never goes down
    last = 0
    for total in range(1, w + (2 * halo + 3) * s):
        now = check(total)
        assert now >= last
        last = now


def test_bad_arguments_raise():
    for bad in ((0, 1, 4, 2, 5), (400, 0, 4, 2, 5), (400, 401, 4, 2, 5), (400, 160, 4, 2, -1), (400, 160, -1, 0, 5), (400, 160, 2, 3, 5),
                (400, 160, 4, -1, 5), (400, 160, 4, 0, 5)):
        with pytest.raises(CtuError):
            streams_rows_step(*bad)
    L = ctucopy_amd.load_library()
    assert L.ctu_streams_pending(None, 0) == ceng.CTU_ERR_INPUT
    assert L.ctu_streams_finish_host(None, 0, None, 0, None) == ceng.CTU_ERR_INPUT
    n, arr = ceng._argv(C2)
    buf = ctypes.create_string_buffer(256)
    assert L.ctu_streams_config_check_ex(n, arr, 2, buf, len(buf), None) == ceng.CTU_ERR_INPUT and b"flags" in buf.value
