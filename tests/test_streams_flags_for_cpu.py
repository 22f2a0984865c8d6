"""ctu_streams_flags_for (include/ctu_engine.h): the flag set a command line needs on a stream set, without a GPU.

For every configuration of the list: the flags are the ones written next to it (the union of the kinds of state its options call for);
an accepted one is accepted by ctu_streams_config_check_ex for those flags with the same halo, and refused with any one bit cleared (no
bit is set that is not needed); a refused one comes back with the code, the reason and the flags of ctu_streams_config_check_ex for that
very set.  A bad command line gives the parser's error and flags 0.
"""
import pytest

from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from ctucopy_amd import streams_config_check_ex, streams_flags_for
from tests.util import C1, C2, C3, C4, C5, M8, M44, SIG_EXTEN

ROW, NR, VAD, SIG, LARGE = ceng.STREAMS_ROW_STATE, ceng.STREAMS_NR_STATE, ceng.STREAMS_VAD_STATE, ceng.STREAMS_SIGNAL_STATE, ceng.STREAMS_LARGE_STATE
TRAP, SS, SS_SIG, SS_LARGE, VAD_ROW = (ceng.STREAMS_TRAP_STATE, ceng.STREAMS_SS_STATE, ceng.STREAMS_SS_SIGNAL_STATE, ceng.STREAMS_SS_LARGE_STATE,
                                       ceng.STREAMS_VAD_ROW_STATE)
ENERGY_VAD = "-vad_out_mode vad -vad_cri_mode energy -vad_thr_mode dyn".split()
SIG44 = "-fs 44100 -format_in raw -format_out raw -preset exten".split()
SIG_SS = "-fs 16000 -format_in raw -format_out raw -preset exten -w 25 -s 12.5 -vad burg".split()

# (name, command line, flags, halo) of what a set takes; (name, command line, flags, a word of the refusal) of what none does
ACCEPTED = [
    ("C1", C1, 0, 0),
    ("C3 plp", C3, 0, 0),
    ("delta d_a + CMS", C2 + ["-fea_delta", "d_a", "-fea_Z_exp", "500"], ROW, 4),
    ("stacking of 5 frames", C2 + ["-fea_trap", "5"], ROW, 2),
    ("block CMS alone", C2 + ["-fea_Z_block", "500"], ROW, 0),
    ("exten", C2 + ["-nr_mode", "exten"], NR, 0),
    ("exten + delta", C2 + ["-nr_mode", "exten", "-fea_delta", "d"], NR | ROW, 2),
    ("exten at 44.1 kHz", M44 + ["-nr_mode", "exten"], NR | LARGE, 0),
    ("exten at 44.1 kHz + delta", M44 + ["-nr_mode", "exten", "-fea_delta", "d_a"], NR | LARGE | ROW, 4),
    ("plain chain at 44.1 kHz", M44, 0, 0),
    ("energy VAD, order 5", C2 + ENERGY_VAD + ["-vad_filter_order", "5"], VAD, 2),
    ("C4", C4, NR | VAD, 1),                                   # (filter order 3: h = 1)
    ("C4 + CMS", C4 + ["-fea_Z_exp", "500"], NR | VAD | ROW | VAD_ROW, 1),
    ("energy VAD + d_a", C2 + ENERGY_VAD + ["-vad_filter_order", "3", "-fea_delta", "d_a"], VAD | ROW | VAD_ROW, 5),
    ("speech output", "-fs 16000 -format_in raw -format_out raw -w 25 -s 10 -preset mfcc".split(), SIG, 0),
    ("speech output, exten", SIG_EXTEN, SIG | NR, 0),
    ("speech output, wave", SIG_EXTEN[:5] + ["wave"] + SIG_EXTEN[6:], SIG | NR, 0),
    ("speech output at 44.1 kHz, exten", SIG44, SIG | NR | LARGE, 0),
    ("speech output at 44.1 kHz, plain", SIG44 + ["-nr_mode", "none"], SIG | LARGE, 0),
    ("C5 trapdct", C5, TRAP, 50),
    ("trapdct behind exten", C5 + ["-nr_mode", "exten"], TRAP | NR, 50),
    ("fwss", C2 + ["-nr_mode", "fwss", "-vad", "burg"], SS, 0),
    ("2fwss + d_a at 8 kHz", M8 + ["-nr_mode", "2fwss", "-vad", "burg", "-fea_delta", "d_a"], SS | ROW, 4),
    ("fwss at 44.1 kHz", M44 + ["-nr_mode", "fwss", "-vad", "burg"], SS | SS_LARGE, 0),
    ("hwss at 44.1 kHz + CMS", M44 + ["-nr_mode", "hwss", "-vad", "burg", "-fea_Z_exp", "300"], SS | SS_LARGE | ROW, 0),
    ("speech output behind fwss", SIG_SS + ["-nr_mode", "fwss"], SIG | SS | SS_SIG, 0),
]
REFUSED = [
    ("-remove_dc1", C1 + ["-remove_dc1", "on"], 0, "-remove_dc1"),
    ("-nr_when afterFB", C2 + ["-nr_mode", "exten", "-nr_when", "afterFB"], NR, "-nr_when afterFB"),
    ("the fea criterion", C2 + ["-vad_out_mode", "vad", "-vad_cri_mode", "cepdist", "-vad_cepdist_mode", "fea"], VAD, "-vad_cepdist_mode fea"),
    ("-vad_apply_mode drop", C4 + ["-vad_apply_mode", "drop"], NR | VAD, "-vad_apply_mode drop"),
    ("-vad file=", C2 + ["-nr_mode", "fwss", "-vad", "file=/nonexistent/decisions"], SS, "-vad file="),
    ("-format_in htk", "-fs 16000 -format_in htk -format_out htk -preset mfcc -fea_rawenergy on -nfeacoefs 13 -fea_delta d".split(), ROW, "-format_in htk"),
    ("CMVN", C2 + ["-stat_cmvn", "stats.txt"], 0, "-stat_cmvn"),
    ("-s above -w", C1 + ["-s", "30"], 0, "-s above -w"),
    ("VAD beside trapdct", C5 + ENERGY_VAD, TRAP | VAD, "-fea_kind trapdct"),
    ("VAD at 44.1 kHz", M44 + ENERGY_VAD, VAD, "1024-point and larger"),
    ("-fea_E behind the majority filter", C2 + ENERGY_VAD + ["-vad_filter_order", "5", "-fea_E", "on"], VAD, "-fea_E"),
    ("speech output behind fwss at 44.1 kHz", SIG44 + ["-nr_mode", "fwss", "-vad", "burg"], SIG | SS | SS_SIG | SS_LARGE, "2048-point frames"),
    ("-nr_rasta: outside the engine", C2 + ["-nr_rasta", "rasta.txt"], 0, "not on the accelerated path"),
]


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


def _bits(flags):
    return [1 << k for k in range(32) if flags >> k & 1]


@pytest.mark.parametrize("name,cfg,flags,halo", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_accepted_configuration_gets_the_flags_it_needs_and_no_more(name, cfg, flags, halo):
    rc, got, reason, h = streams_flags_for(cfg)
    assert (rc, got, reason, h) == (ceng.CTU_OK, flags, "", halo)
    assert streams_config_check_ex(cfg, got) == (ceng.CTU_OK, "", halo)
    for bit in _bits(got):
        less = streams_config_check_ex(cfg, got & ~bit)
        assert less[0] != ceng.CTU_OK and less[1], (name, bit, less)


@pytest.mark.parametrize("name,cfg,flags,word", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_configuration_gets_the_refusal_of_its_own_flag_set(name, cfg, flags, word):
    rc, got, reason, h = streams_flags_for(cfg)
    assert rc == ceng.CTU_ERR_UNSUPPORTED and got == flags and word in reason, (rc, got, reason)
    assert (rc, reason, h) == streams_config_check_ex(cfg, got)
    assert h == 0


def test_every_flag_is_reached():
    seen = 0
    for _, cfg, flags, _ in ACCEPTED:
        seen |= flags
    assert seen == ROW | NR | VAD | SIG | LARGE | TRAP | SS | SS_SIG | SS_LARGE | VAD_ROW


def test_bad_command_line_gives_the_parsers_error():
    for cfg, text in ((["-preset", "mfcc"], "OPTS: Please specify sampling rate!"),
                      (C2 + ["-preset", "nonesuch"], "OPTS: Unknown preset!"),
                      (C2 + ["-preem", "1.5"], "OPTS: Preemphasis not in range <0,1)!")):
        rc, flags, reason, halo = streams_flags_for(cfg)
        assert (rc, flags, reason, halo) == (ceng.CTU_ERR_OPTS, 0, text, 0)
        assert streams_config_check_ex(cfg, 0) == (rc, reason, halo)


def test_binding_types_and_export():
    out = streams_flags_for(C1)
    assert isinstance(out, tuple) and [type(v) for v in out] == [int, int, str, int]
    assert "ctu_streams_flags_for" in ceng.EXPORTS
    assert streams_flags_for([str(a) for a in C1]) == streams_flags_for(tuple(C1))
    # the flags do not depend on the reason buffer: the C call with a NULL reason, NULL flags and NULL halo answers the same code
    import ctypes
    L = ceng.load_library()
    n, arr = ceng._argv(C4)
    assert L.ctu_streams_flags_for(n, arr, None, None, 0, None) == ceng.CTU_OK
    n, arr = ceng._argv(C1 + ["-remove_dc1", "on"])
    flags = ctypes.c_uint32(77)
    assert L.ctu_streams_flags_for(n, arr, ctypes.byref(flags), None, 0, None) == ceng.CTU_ERR_UNSUPPORTED and flags.value == 0
