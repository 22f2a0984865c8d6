"""The plan of an offline run (ctucopy_amd/csrc/plan.cc) against the commit it was moved out of engine.hip at, without a GPU.

tests/golden/host_plans.json was recorded from that parent commit, not from this code (its `how` field says how, and in which order
the words of a report come).  Per case it holds the length and SHA-256 of a flat report of every HostPlan field - offsets, frames,
totals, the tiles with their links, chain heads and grid, utterance info, the chunk lists, tile_utt, vf_order, out_samples and the
element count of every device buffer the plan owns - or, for a refused batch, the code and the full text; likewise the lists of
ctu_plan_set_vad_ring / ctu_vad_ring_step / ctu_vad_ring_rows and the ranges of a host-buffer run.  The planner, compiled without the
engine under Address+UB sanitizers as a program of its own (tests/host/plan_check.cc), must give the same answers with nothing for the
sanitizers - or for its own checks of the chains - to report.  On a GPU, a created plan must be the host unit's."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from ctucopy_amd import build as cbuild
from tests.util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(GOLDEN, "host_plans.json")) as f:
    CASES = json.load(f)["cases"]
with open(os.path.join(GOLDEN, "host_tables.json")) as f:
    _TABLES = json.load(f)
CONFIGS = {**{n: r["args"] for n, r in _TABLES["refusals"].items()}, **{n: r["args"] for n, r in _TABLES["tables"].items()}}


def args_of(case):
    return CONFIGS[case["config"]] + case["extra"]


def test_the_recorded_set_covers_what_it_should():
    plans = {n: c for n, c in CASES.items() if c["kind"] == "P"}
    refused = {c["text"] for c in plans.values() if "code" in c}
    assert len(refused) == 5 and all(c["code"] == -4 for c in plans.values() if "code" in c)  # CTU_ERR_INPUT
    assert {c["n_cu"] for c in plans.values()} == {2, 256}
    forty = {(c["config"], tuple(c["extra"])) for c in plans.values() if "sha256" in c and len(c["lengths"]) == 40 and c["n_cu"] == 2}
    # plain 256- and 512-point, exten, hwss on 256 and on 2048 points, -vad burg fused and unfused, energy VAD, speech output, -remove_dc1,
    # trapdct, a delta chain with CMS, an LP kind on wave1k, -format_in htk
    assert forty >= {(n, ()) for n in ("md_mfcc_8k", "C2", "md_exten_16k", "ss_spec_8k", "big_ss_2048_file", "vf_plain_8k", "vx_burg_128pt", "vx_energy_16k",
                                       "sy_plain_16k", "dc1_mfcc_16k", "C5", "big_C3_w40", "st_htk")} | {("st_delta", ("-fea_Z_exp", "500"))}
    for n, e in forty:  # forty utterances on two CUs: more live utterances than chain slots
        assert sum(x > 0 for x in next(c for c in plans.values() if c["config"] == n and len(c["lengths"]) == 40)["lengths"]) > 32
    assert {(c["order"], c["hidx"][0]) for c in CASES.values() if c["kind"] == "G"} == {(1, 0), (1, 1), (3, 0), (3, 1), (3, 2), (5, 0), (5, 1), (5, 4)}
    ranges = [c for c in CASES.values() if c["kind"] == "S"]
    assert len(ranges) == 2 and all(c["nparts"] == 8 and len(c["lengths"]) == 16 for c in ranges)
    # eight ranges of two utterances; with the long second utterance goals 1 to 6 of 7 fall inside it: ranges [0, 2), [2, 8), [8, 16)
    assert sorted(c["first"] for c in ranges) == [[0, 2, 4, 6, 8, 10, 12, 14, 16], [0, 2, 8, 16]]


def test_plans_are_the_parents_word_for_word(tmp_path):
    """plan.cc with tables.cc, accept.cc, opts.cc and design.cc as a program of their own: nothing is loaded into python, nothing is preloaded."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(cbuild.HIPCC)))
    cxx = next((p for p in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")) if os.path.exists(p)), None)
    assert cxx, "the clang++ behind hipcc (tables.cc splits the TRAP table into _Float16 terms)"
    csrc = os.path.join(ROOT, "ctucopy_amd", "csrc")
    exe = tmp_path / "plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                    os.path.join(ROOT, "tests", "host", "plan_check.cc"),
                    *[os.path.join(csrc, s) for s in ("plan.cc", "tables.cc", "accept.cc", "opts.cc", "design.cc")], "-o", str(exe)], check=True)

    def csv(v):
        return ",".join(str(x) for x in v) if len(v) else "-"

    lines = []
    for n, c in sorted(CASES.items()):
        aux = {"P": [], "G": [c.get("order")] + c.get("hidx", []), "S": [c.get("nparts")]}[c["kind"]]
        lines.append("\t".join([c["kind"], n, str(c["n_cu"]), csv(c["lengths"]), csv(aux)] + args_of(c)))
    cfg = tmp_path / "cases.tsv"
    cfg.write_text("\n".join(lines) + "\n")
    env = {k: v for k, v in os.environ.items() if k not in ("CTU_PHASE2_GENERIC", "CTU_WAVE1K", "CTU_DEBUG_MODE")}  # the recorded environment
    cp = subprocess.run([str(exe), str(cfg)], capture_output=True, text=True, env=env)
    assert cp.returncode == 0, cp.stderr[-4000:]
    assert cp.stderr == "", cp.stderr[-4000:]
    out = cp.stdout.strip().splitlines()
    assert out[-1] == "plan_check ok: %d cases" % len(lines)
    got = {}
    for p in (l.split(" ") for l in out[:-1]):
        got[p[1]] = (int(p[2]), bytes.fromhex(p[3] if len(p) > 3 else "").decode()) if p[0] == "R" else (p[0], int(p[2]), p[3])
    want = {n: (c["code"], c["text"]) if "code" in c else (c["kind"], c["length"], c["sha256"]) for n, c in CASES.items()}
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["md_exten_16k", "st_htk"])
def test_a_created_plan_is_the_host_units(config):
    """ctu_plan_create's offsets and totals against ctu_arena_layout / ctu_rows_arena_layout and ctu_num_frames, the planner's own rules."""
    from ctucopy_amd import engine as ceng
    L = ceng.load_library()
    i64 = ctypes.c_int64
    eng = ceng.Engine(CONFIGS[config])
    try:
        d = eng.dims
        frames = [0, 1, 64, 65, 129]
        ns = np.array([f if d.rows_in else d.window - d.wshift + f * d.wshift for f in frames], dtype=np.int64)
        assert [eng.num_frames(n) for n in ns] == frames
        off = np.zeros(len(ns) + 1, dtype=np.int64)
        pn, po = ns.ctypes.data_as(ctypes.POINTER(i64)), off.ctypes.data_as(ctypes.POINTER(i64))
        total = L.ctu_rows_arena_layout(pn, len(ns), d.row_floats_in, po) if d.rows_in else L.ctu_arena_layout(pn, len(ns), po)
        plan = eng.plan(ns)
        assert plan.sample_off.tolist() == off.tolist() and plan.total_samples == total
        assert plan.row_off.tolist() == np.concatenate([[0], np.cumsum(frames)]).tolist() and plan.total_frames == sum(frames)
        plan.close()
    finally:
        eng.close()
