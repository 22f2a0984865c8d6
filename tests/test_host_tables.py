"""What the engine decides and lays out on the host (ctucopy_amd/csrc/accept.cc, tables.cc) against the commit those units were moved
out of engine.hip at, without a GPU.

tests/golden/host_tables.json was recorded from that parent commit, not from this code (its `how` field says how):
  tables    per configuration the length and SHA-256 of ctu_config_table(..., "host_tables") - every scalar and every table image
            ctu_engine_create uploads, as 32-bit words, and the VAD parameter block (include/ctu_engine.h gives the order);
  refusals  per refused configuration the return code and the full text of ctu_create_error / ctu_streams_config_check_ex.
The same units, compiled without the engine under Address+UB sanitizers as a program of their own (tests/host/host_tables_check.cc),
must give the same answers with nothing for the sanitizers to report."""
import ctypes
import hashlib
import json
import os
import subprocess

import pytest

from ctucopy_amd import build as cbuild
from ctucopy_amd import config_table
from ctucopy_amd import engine as ceng
from tests.util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(GOLDEN, "host_tables.json")) as f:
    RECORDED = json.load(f)
TABLES, REFUSALS = RECORDED["tables"], RECORDED["refusals"]


@pytest.fixture(autouse=True)
def _recorded_environment(monkeypatch):
    for var in ("CTU_PHASE2_GENERIC", "CTU_WAVE1K", "CTU_DEBUG_MODE"):
        monkeypatch.delenv(var, raising=False)


def digest(values):
    return hashlib.sha256(values.astype("<f8").tobytes()).hexdigest()


def test_the_recorded_set_covers_what_it_should():
    with open(os.path.join(GOLDEN, "frontend_selection.json")) as f:
        assert set(json.load(f)["configs"]) <= set(TABLES)
    assert len(TABLES) >= 82 + 11 and len(REFUSALS) >= 40
    assert {r["call"] for r in REFUSALS.values()} == {"ctu_engine_create", "ctu_streams_config_check_ex"}
    assert {r["code"] for r in REFUSALS.values()} >= {ceng.CTU_ERR_OPTS, ceng.CTU_ERR_UNSUPPORTED, ceng.CTU_ERR_INPUT}
    assert all(r["code"] not in (ceng.CTU_OK, ceng.CTU_ERR_DEVICE) and r["text"] for r in REFUSALS.values())


@pytest.mark.parametrize("name", sorted(TABLES))
def test_tables_are_the_parents_bit_for_bit(name):
    rec = TABLES[name]
    v = config_table(rec["args"], "host_tables")
    assert (len(v), digest(v)) == (rec["length"], rec["sha256"])


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_are_the_parents_byte_for_byte(name):
    rec = REFUSALS[name]
    L = ceng.load_library()
    n, arr = ceng._argv(rec["args"])
    if rec["call"] == "ctu_engine_create":
        h = ctypes.c_void_p()
        rc = L.ctu_engine_create(n, arr, 0, ctypes.byref(h))
        text = L.ctu_create_error()
    else:
        buf = ctypes.create_string_buffer(4096)
        rc = L.ctu_streams_config_check_ex(n, arr, rec["flags"], buf, 4096, None)
        text = buf.value
        assert L.ctu_create_error() == text
    assert (int(rc), text) == (rec["code"], rec["text"].encode())


def test_host_units_under_sanitizers(tmp_path):
    """accept.cc, tables.cc, opts.cc and design.cc as a program of their own: nothing is loaded into python, nothing is preloaded."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(cbuild.HIPCC)))
    cxx = next((p for p in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")) if os.path.exists(p)), None)
    assert cxx, "the clang++ behind hipcc (tables.cc splits the TRAP table into _Float16 terms)"
    csrc = os.path.join(ROOT, "ctucopy_amd", "csrc")
    exe = tmp_path / "host_tables_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                    os.path.join(ROOT, "tests", "host", "host_tables_check.cc"),
                    *[os.path.join(csrc, s) for s in ("accept.cc", "tables.cc", "opts.cc", "design.cc")], "-o", str(exe)], check=True)
    lines = ["\t".join(["T", n, "0"] + r["args"]) for n, r in sorted(TABLES.items())]
    lines += ["\t".join(["C" if r["call"] == "ctu_engine_create" else "S", n, str(r.get("flags", 0))] + r["args"]) for n, r in sorted(REFUSALS.items())]
    cfg = tmp_path / "configs.tsv"
    cfg.write_text("\n".join(lines) + "\n")
    cp = subprocess.run([str(exe), str(cfg)], capture_output=True, text=True)  # (the fixture above has cleared the CTU_... switches)
    assert cp.returncode == 0, cp.stderr[-4000:]
    assert cp.stderr == "", cp.stderr[-4000:]
    out = cp.stdout.strip().splitlines()
    assert out[-1] == "host_tables_check ok: %d configurations" % len(lines)
    got_t = {p[1]: (int(p[2]), p[3]) for p in (l.split(" ") for l in out[:-1]) if p[0] == "T"}
    got_r = {p[1]: (int(p[2]), bytes.fromhex(p[3] if len(p) > 3 else "").decode()) for p in (l.split(" ") for l in out[:-1]) if p[0] == "R"}
    assert got_t == {n: (r["length"], r["sha256"]) for n, r in TABLES.items()}
    assert got_r == {n: (r["code"], r["text"]) for n, r in REFUSALS.items()}
