"""What the compiled reference does with -online_in -online_out (tests/golden/ref_pipe.npz, recorded by tests/golden/make_ref_pipe_fixtures.py):
the specification of the pipe mode of bin/ctucopy.  The test reads the fixture alone; only the recorder runs the reference binary.

Recorded per case: the exit status and stdout of `... -online_in -online_out` with the input on stdin, and the exit status and the file
of `... -i in -o out` on the same bytes (with the VAD module: and the file of -vad_out of either run).

What the fixture shows.  The reference's single-file branch calls vad->new_file() whether or not a VAD module was built
(src/io/batch.cc:299-310; the list branch asks do_vad first, :398-399), so WITHOUT the VAD module both single-file runs - file to file and
stdin to stdout alike - die with status 139 ahead of their first frame and write nothing: C1, the a-law MFCC preset and -preset exten to raw,
the three cases the pipe mode was specified on, all do (DESIGN.md section 7 lists them as `ref_pipe:...`).  WITH the VAD module the runs end
with status 0, and what the pipe wrote is the file without its 12-byte HTK header (src/io/out.cc:115-137), the decisions byte for byte
those of the file run.  Speech output cannot be had either way: the reference builds no VAD ahead of sigOUT (batch.cc:62-66), so
out.cc:478's stream branch is never reached alive.  tests/test_cli_pipe.py compares bin/ctucopy's pipe output with the bytes of the runs
that lived.
"""
import os
import re
import zlib

import numpy as np
import pytest

from tests.util import C1, C4, GOLDEN, g711_codes, sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cs3():
    return sig("CS3")[:16000].astype("<i2").tobytes()


def _codes():
    return g711_codes(8000).tobytes()


# name -> (command line, input bytes, HTK output, VAD module)
REF_PIPE_CASES = {
    "c1": (C1, _cs3, True, False),
    "alaw_mfcc": ("-fs 8000 -format_in alaw -format_out htk -preset mfcc".split(), _codes, True, False),
    "exten_raw": ("-fs 16000 -format_in raw -format_out raw -preset exten".split(), _cs3, False, False),
    # the same front ends with the VAD module beside them: the runs the reference survives
    "c1_vad": (C1 + "-vad_out_mode vad -vad_cri_mode energy -vad_thr_mode dyn".split(), _cs3, True, True),
    "alaw_c4": (C4[:3] + ["alaw"] + C4[4:], _codes, True, True),
}
SURVIVES = sorted(n for n, c in REF_PIPE_CASES.items() if c[3])
DIES = sorted(n for n, c in REF_PIPE_CASES.items() if not c[3])


def ref_pipe():
    return np.load(os.path.join(GOLDEN, "ref_pipe.npz"))


@pytest.mark.parametrize("name", sorted(REF_PIPE_CASES))
def test_fixture_was_recorded_on_the_inputs_of_this_module(name):
    data = REF_PIPE_CASES[name][1]()
    assert ref_pipe()[name + "__input"].tolist() == [len(data), zlib.crc32(data)]


@pytest.mark.parametrize("name", SURVIVES)
def test_reference_pipe_output_is_the_file_without_its_header(name):
    z = ref_pipe()
    assert int(z[name + "__pipe_status"]) == 0 and int(z[name + "__file_status"]) == 0
    piped, filed = z[name + "__stdout"].tobytes(), z[name + "__file"].tobytes()
    assert piped == filed[12:]
    n, period = np.frombuffer(filed[:8], "<u4")
    size, kind = np.frombuffer(filed[8:12], "<u2")
    # 16000 samples at 16 kHz, 8000 codes at 8 kHz, 25 / 10 ms: 98 frames of 13 floats
    assert (int(n), int(size)) == (98, 52) and len(piped) == 98 * 52
    assert np.isfinite(np.frombuffer(piped, "<f4")).all()
    vp, vf = z[name + "__pipe_vad"].tobytes(), z[name + "__file_vad"].tobytes()
    assert vp == vf and len(vp) == 98 and set(vp) <= set(b"01")


@pytest.mark.parametrize("name", DIES)
def test_reference_single_file_mode_dies_without_the_vad_module(name):
    z = ref_pipe()
    assert int(z[name + "__pipe_status"]) == 139 and int(z[name + "__file_status"]) == 139
    assert z[name + "__stdout"].size == 0 and z[name + "__file"].size == 0


def test_the_design_lists_the_runs_the_reference_died_on():
    z = ref_pipe()
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("\n## 7"):]
    section = section[:section.index("\n## ", 1)] if "\n## " in section[1:] else section
    listed = {m.group(1): int(m.group(2)) for m in re.finditer(r"`ref_pipe:(\w+)` \(exit status (\d+)\)", section)}
    assert listed == {n: int(z[n + "__pipe_status"]) for n in REF_PIPE_CASES if int(z[n + "__pipe_status"])}
