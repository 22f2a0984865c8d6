"""The front-end instantiation a configuration runs on (fe_select in tables.cc), checked without a GPU.

ctu_config_table(..., "frontend") reports frontend_kernel's template arguments as ctu_engine_create selects them.  The expected
values in tests/golden/frontend_selection.json are not this selector's: they are the template arguments of the frontend_kernel that
the launch tree of the commit named in the file (launch_vx / launch_nz / launch_walk, removed since) ended on for each configuration;
the file says how they were recorded."""
import json
import os

import pytest

from ctucopy_amd import config_table
from tests import util
from tests.util import GOLDEN

FIELDS = ("nz", "feat", "mode", "vx", "nc", "gen", "lpo", "md", "vf", "ss", "sy", "walk")
FEAT = {0: "BANDS", 2: "DCTC", 3: "LP", 4: "LPD"}            # layout_constants.h: FeatMode
GEN = {0: "plain", 1: "inld", 2: "exten", 3: "full", 4: "full"}  # GEN_PLAIN .. GEN_DC1 (-remove_dc1 is the run-time-flag kernel too)

with open(os.path.join(GOLDEN, "frontend_selection.json")) as f:
    RECORDED = json.load(f)
CONFIGS = RECORDED["configs"]


def selection(args):
    v = config_table(args, "frontend")
    assert len(v) == len(FIELDS)
    return [int(x) for x in v]


def name_of(sel):
    """ctu_engine_kernel_name's form: the export, the row width, LPO and the walk are not shown."""
    k = dict(zip(FIELDS, sel))
    return ("frontend_kernel<%d, %s, MODE %d, %s" % (k["nz"], FEAT[k["feat"]], k["mode"], GEN[k["gen"]]) +
            "".join(", " + t.upper() for t in ("md", "vf", "ss", "sy") if k[t]) + ">")


def is_dual(sel):
    """layout_constants.h, fe_dual: the instantiations whose window table is scaled by 1/2."""
    k = dict(zip(FIELDS, sel))
    return k["mode"] == 0 and k["gen"] in (0, 1) and not k["vx"] and k["nz"] < 16 and not (k["vf"] or k["ss"] or k["sy"])


@pytest.fixture(autouse=True)
def _no_generic_walk(monkeypatch):
    monkeypatch.delenv("CTU_PHASE2_GENERIC", raising=False)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_selection_is_the_instantiation_that_was_launched(name):
    rec = CONFIGS[name]
    assert selection(rec["args"]) == rec["frontend"], name_of(rec["frontend"])


@pytest.mark.parametrize("name", ["C1", "C2", "C3", "C4", "C4_NOVAD", "C5"])
def test_named_configurations_are_the_suites(name):
    assert CONFIGS[name]["args"] == getattr(util, name)


def test_every_branch_of_the_choice_is_pinned():
    seen = {tuple(r["frontend"][:11]) for r in CONFIGS.values()}
    k = [dict(zip(FIELDS, s)) for s in seen]
    assert any(x["sy"] and not x["ss"] and x["gen"] == 3 for x in k) and any(x["sy"] and x["ss"] for x in k) and any(x["sy"] and x["gen"] == 4 for x in k)
    assert any(x["gen"] == 4 and not x["sy"] for x in k)
    assert any(x["ss"] and x["lpo"] == 12 and x["md"] for x in k) and any(x["ss"] and x["lpo"] == 0 and x["md"] for x in k)
    assert any(x["ss"] and x["feat"] == 0 and x["gen"] == 0 and x["lpo"] == 12 for x in k) and any(x["ss"] and x["feat"] == 0 and x["gen"] == 0 and x["lpo"] == 0 for x in k)
    assert all(any(x["ss"] and x["gen"] == 3 and not x["sy"] and x["feat"] == f for x in k) for f in (0, 2, 3, 4))
    assert {(x["mode"], x["gen"]) for x in k if x["vf"]} >= {(0, 0), (1, 0), (0, 2), (1, 2)}
    assert any(x["md"] and x["feat"] == 3 and x["lpo"] == 12 for x in k) and any(x["md"] and x["feat"] == 3 and x["lpo"] == 0 for x in k)
    assert any(x["vx"] for x in k) and any(x["nc"] == 24 for x in k) and any(x["feat"] == 4 for x in k)
    assert {r["frontend"][11] for r in CONFIGS.values()} == {-1, 0, 1, 2}


def test_recorded_values_format_to_the_names_that_key_the_profiles():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "traffic.json")) as f:
        assert name_of(CONFIGS["C2"]["frontend"]) == json.load(f)["kernel"]
    assert name_of(CONFIGS["C2"]["frontend"]) == "frontend_kernel<13, DCTC, MODE 0, plain, MD>"
    assert name_of(CONFIGS["C3"]["frontend"]) == "frontend_kernel<13, LP, MODE 0, inld, MD>"
    assert name_of(CONFIGS["C4"]["frontend"]) == "frontend_kernel<13, DCTC, MODE 1, exten, MD, VF>"


def test_window_table_is_halved_for_exactly_the_dual_instantiations():
    dual = {n for n, r in CONFIGS.items() if is_dual(r["frontend"])}
    assert {"C1", "C2", "C3", "C5"} <= dual and not dual & {"C4", "C4_NOVAD"}
    for n, r in CONFIGS.items():
        assert is_dual(selection(r["args"])) == (n in dual), n


def test_large_fft_configurations_report_no_front_end():
    for extra in (["-w", "40"], ["-w", "80"]):  # wave1k_kernel, bigfft_kernel<8>
        assert selection(util.C2 + extra) == [0] * 11 + [-1]


def test_generic_walk_switch_reaches_the_selection(monkeypatch):
    monkeypatch.setenv("CTU_PHASE2_GENERIC", "1")
    for n in ("C2", "C3", "C5"):
        assert selection(CONFIGS[n]["args"]) == CONFIGS[n]["frontend"][:11] + [-1]
