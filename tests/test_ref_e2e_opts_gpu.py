"""The engine and `bin/ctucopy` against the compiled reference over the rest of the option space: tests/util.py's REF_E2E_OPT_CASES and
ref_e2e_file_cases() as tests/golden/ref_e2e_opts.npz holds them (recorded by tests/golden/make_ref_e2e_fixtures.py opts) - banks, feature
kinds, hwss / 2fwss and exten carried over a frameless file, the VAD's criteria, thresholds, drop and filter orders with its stream, third-order
deltas, and the files the writers produce (ark + scp, pfile, big-endian HTK, CMVN, G.711 and wave input).

The rules are those of tests/test_ref_e2e_gpu.py, through its own functions: 1e-4 element-wise for the well-conditioned class; 1e-3
element-wise and 1e-4 of the row's largest value otherwise; VAD bytes identical, the list as one process's with the case's filter order;
samples within 2 LSB, mean below 0.3.  2fwss takes the rule tests/test_gpu_parity.py states for it: at most one frame in 100 outside the
bound, and that below 5e-2.  Drop cases compare the rows that remain.  The file cases hold every byte that is not a float of the payload
equal to the recording and the floats to the row rule.  Every test prints its figures before it asserts; none reads anything but the .npz.
"""
import subprocess

import numpy as np
import pytest

from tests.test_oracle_ref_e2e import reference_kind
from tests.test_ref_e2e_gpu import Engine, _assert_rows, _assert_samples, _errors  # noqa: F401  (Engine: the module's fixture)
from tests.util import REF_E2E_OPT_CASES, ref_e2e_file_cases, ref_e2e_inputs, ref_e2e_opts, split_written_file

pytestmark = pytest.mark.gpu

FX = ref_e2e_opts()
DAT_KIND = 6 | 0o20000 | 0o400 | 0o1000 | 0o100000     # MFCC_0_D_A_T as HTK defines it
# The one list the engine does not reproduce: at filter orders of 5 and more a file with no more frames than the
# filter delays leaves the reference's historySize half drained, and the file behind it writes a row more than it has frames
HALF_DRAINED = "vad_c4_order7"

# Refused by the engine with CTU_ERR_UNSUPPORTED; the oracle holds these cases against the recording on the CPU
REFUSED = {"kind_plp23": "LP order not below the number of bands"}     # order 23 on the PLP bank's 19 bands; kind_lpc23_mel30 runs order 23

_INPUTS = {}


def inputs(name):
    if name not in _INPUTS:
        _INPUTS[name] = ref_e2e_inputs(name)
        for u in _INPUTS[name]:
            u.setflags(write=False)
    return _INPUTS[name]


def _filter_order(cfg):
    return int(cfg[len(cfg) - 1 - cfg[::-1].index("-vad_filter_order") + 1]) if "-vad_filter_order" in cfg else 3


def _assert_2fwss_rows(g, ref, what):
    assert g.shape == ref.shape and g.dtype == np.float32, (what, g.shape, ref.shape)
    if not ref.size:
        return
    e = (np.abs(g - ref) / np.maximum(np.abs(ref), 1.0)).max(axis=1)
    rn = np.abs(g - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1.0)
    out = (e > 1e-3) | (rn > 1e-4)
    print(f"ref e2e opts {what}: 2fwss, {int(out.sum())} of {ref.shape[0]} rows outside 1e-3 / 1e-4, worst element-wise {float(e.max()):.3e}, of the row's largest {float(rn.max()):.3e}")
    assert out.sum() <= max(1, ref.shape[0] // 100) and e.max() <= 5e-2, (what, int(out.sum()), float(e.max()))


def _check_rows_case(Engine, name, n_files=None):
    cfg, inp = REF_E2E_OPT_CASES[name]
    utts = inputs(inp)[:n_files]
    eng = Engine(cfg)     # one engine over the list: the *ss modes and exten go on from what the previous file left
    if f"{name}__0__pcm" in FX.files:
        assert eng.dims.signal_out == 1
        for i, g in enumerate(eng.enhance(utts)):
            _assert_samples(g, FX[f"{name}__{i}__pcm"], f"{name}[{i}]")
        return
    has_vad = f"{name}__0__vad" in FX.files
    if has_vad:
        got, vads = eng.extract(utts, want_vad=True, as_list_of_one_process=_filter_order(cfg))
    else:
        got, vads = eng.extract(utts), None
    hdr = FX[f"{name}__0__header"]
    assert [int(hdr[1]), int(hdr[2]), int(hdr[3])] == [eng.dims.htk_period, 4 * eng.dims.row_floats, reference_kind(eng.dims.htk_kind, cfg)], (name, hdr)
    failed = []
    for i, g in enumerate(got):
        ref = FX[f"{name}__{i}__rows"]
        if has_vad:
            v, rv = np.asarray(vads[i]), FX[f"{name}__{i}__vad"]
            print(f"ref e2e opts {name}[{i}]: {v.size} VAD bytes, {int((v != rv).sum()) if v.size == rv.size else -1} differ, {int((rv == ord('1')).sum())} ones, {ref.shape[0]} rows written")
            assert np.array_equal(v, rv), (name, i)
        assert g.shape == ref.shape, (name, i, g.shape, ref.shape)
        if not ref.shape[0]:
            continue
        # hwss sets what it over-subtracts to zero (src/nr/nr.cc:251-254), and a band of nothing but such bins is the logarithm of zero: the
        # reference writes -inf / NaN rows there.  The rule of tests/test_ref_e2e_gpu.py for such rows: the device's row has a non-finite
        # value as well, nothing is asked of its other values; every other row obeys the bounds
        fin = np.isfinite(ref).all(axis=1)
        if not fin.all():
            dev = ~np.isfinite(g).all(axis=1)
            print(f"ref e2e opts {name}[{i}]: {int((~fin).sum())} of {ref.shape[0]} rows non-finite in the reference, {int(dev.sum())} on the device, {int((dev != ~fin).sum())} differ")
            assert "hwss" in cfg and dev[~fin].all(), (name, i, np.flatnonzero(~fin & ~dev))
            g, ref = g[fin], ref[fin]
        try:
            if "2fwss" in cfg:
                _assert_2fwss_rows(g, ref, f"{name}[{i}]")
            else:
                _assert_rows(g, ref, cfg, f"{name}[{i}]")
        except AssertionError as e:     # the figures of every file are printed before the case fails
            failed.append(str(e))
    assert not failed, failed


@pytest.mark.parametrize("name", [n for n in REF_E2E_OPT_CASES if n != HALF_DRAINED and n not in REFUSED])
def test_option_space_matches_the_compiled_reference(Engine, name):
    _check_rows_case(Engine, name)


@pytest.mark.parametrize("name", list(REFUSED))
def test_cases_outside_the_accelerated_path_are_refused_by_name(Engine, name):
    from ctucopy_amd.engine import CTU_ERR_UNSUPPORTED, CtuError
    with pytest.raises(CtuError, match=REFUSED[name]) as ei:
        Engine(REF_E2E_OPT_CASES[name][0])
    assert ei.value.code == CTU_ERR_UNSUPPORTED


def test_filter_order_7_up_to_the_file_the_filter_never_gets_ready_on(Engine):
    """C4 with -vad_filter_order 7 on short3: the first file (111 frames) and the two-frame file behind it - which writes neither a row nor
    a decision - are the reference's, rows and VAD bytes.  The third file is where the reference writes 112 rows and decisions for 111
    frames (the fixture says so, and the oracle reproduces it: tests/test_oracle_ref_e2e_opts.py); the engine does not, and says so by name
    instead of writing other rows, as `bin/ctucopy` does for such a list."""
    from ctucopy_amd.engine import CTU_ERR_UNSUPPORTED, CtuError
    cfg, inp = REF_E2E_OPT_CASES[HALF_DRAINED]
    assert _filter_order(cfg) == 7
    _check_rows_case(Engine, HALF_DRAINED, n_files=2)
    assert FX[f"{HALF_DRAINED}__1__rows"].shape[0] == 0 and FX[f"{HALF_DRAINED}__1__vad"].size == 0
    eng = Engine(cfg)
    frames = eng.num_frames(inputs(inp)[2].size)
    assert FX[f"{HALF_DRAINED}__2__rows"].shape[0] == frames + 1 == FX[f"{HALF_DRAINED}__2__vad"].size
    with pytest.raises(CtuError, match="half drained") as ei:
        eng.extract(inputs(inp), want_vad=True, as_list_of_one_process=7)
    assert ei.value.code == CTU_ERR_UNSUPPORTED


# ---- the files `bin/ctucopy` writes
def _run_cli(cfg, files, list_text, d):
    from ctucopy_amd import build as cbuild
    cbuild.build_cli()
    for fn, data in files.items():
        (d / fn).write_bytes(data)
    (d / "list").write_text(list_text)
    r = subprocess.run([cbuild.CLI] + list(cfg) + ["-S", "list"], capture_output=True, text=True, cwd=str(d))
    assert r.returncode == 0, r.stderr
    return r


def _stat_values(text):
    return np.array([[float(v) for v in l.split("\t")[1].split()] for l in text.splitlines() if "\t" in l])


@pytest.mark.parametrize("name", list(ref_e2e_file_cases()))
def test_cli_files_match_the_files_the_reference_wrote(tmp_path, name):
    cfg, files, list_text, outputs = ref_e2e_file_cases()[name]
    _run_cli(cfg, files, list_text, tmp_path)
    big = name == "file_big_endian"
    failed = []
    for fn in outputs:
        mine, ref = (tmp_path / fn).read_bytes(), bytes(FX[f"{name}__file__{fn}"])
        if fn == "stat":     # the statistics text: labels equal, values under the bound tests/test_cli.py holds the same text to
            lab = lambda t: [l.split("\t")[0] for l in t.splitlines()]
            assert lab(mine.decode()) == lab(ref.decode()), name
            got_vals, want_vals = _stat_values(mine.decode()), _stat_values(ref.decode())
            bound = 2e-6 + 1e-6 * np.abs(want_vals).max()
            print(f"ref e2e opts {name}/stat: values differ by {np.abs(got_vals - want_vals).max():.3e} at the most (bound {bound:.3e})")
            assert got_vals.shape == want_vals.shape and np.abs(got_vals - want_vals).max() <= bound, name
            continue
        assert len(mine) == len(ref), (name, fn, len(mine), len(ref))
        grows, grest = split_written_file(fn, mine, big)
        rrows, rrest = split_written_file(fn, ref, big)
        assert grest == rrest, (name, fn)            # headers, keys, the pfile's counters and index, the .scp text
        for i, (g, r) in enumerate(zip(grows, rrows)):
            try:
                _assert_rows(g, r, cfg, f"{name}/{fn}[{i}]")
            except AssertionError as e:
                failed.append(str(e))
    assert not failed, failed


@pytest.mark.parametrize("name", ["post_dat", "post_dat_windows"])
def test_d_a_t_header_from_the_engine_and_the_cli(Engine, tmp_path, name):
    # HTK's T bit, not the reference's decimal 100000 (src/io/out.cc:159); the rows are the reference's
    cfg, inp = REF_E2E_OPT_CASES[name]
    assert Engine(cfg).dims.htk_kind == DAT_KIND
    utts = inputs(inp)
    _run_cli(cfg, {f"in{i}.raw": u.astype("<i2").tobytes() for i, u in enumerate(utts)}, "".join(f"in{i}.raw out{i}\n" for i in range(len(utts))), tmp_path)
    for i in range(len(utts)):
        img = (tmp_path / f"out{i}").read_bytes()
        n, period = np.frombuffer(img, "<u4", 2)
        size, kind = np.frombuffer(img, "<u2", 2, 8)
        ref, hdr = FX[f"{name}__{i}__rows"], FX[f"{name}__{i}__header"]
        assert [int(n), int(period), int(size)] == hdr[:3].tolist() and int(kind) == DAT_KIND and int(hdr[3]) == (DAT_KIND | 100000) & 0xFFFF == 0o123646
        _assert_rows(np.frombuffer(img, "<f4", offset=12).reshape(ref.shape).copy(), ref, cfg, f"{name}/out{i}")


# ---- the `fea` criterion's vector behind long stacking windows: the paths of vad_decide_kernel beyond the fixture's 39 and 117 entries
FEA_DYN = "-vad_out_mode vad -vad_cri_mode cepdist -vad_cepdist_mode fea -vad_thr_mode dyn".split()


@pytest.mark.parametrize("extra,entries", [(["-fea_trap", "33"], 429), (["-fea_ncepcoefs", "16", "-fea_trap", "29"], 493)])
def test_fea_criterion_on_long_stacked_vectors(Engine, extra, entries):
    # 7 and 8 entries per lane (429 = 6 x 64 + 45, 493 = 7 x 64 + 45: the last slot partly filled), against the oracle, whose criterion the
    # fixture pins at 39 and 117 entries and which agrees with the compiled reference on these two chains as well; decisions byte for byte, rows in the well-conditioned class
    from oracle.oracle import Oracle
    from tests.util import C2
    cfg = C2 + FEA_DYN + extra
    utts = inputs("short")
    eng, orc = Engine(cfg), Oracle(cfg)
    assert eng.dims.row_floats == entries
    got, vads = eng.extract(utts, want_vad=True, as_list_of_one_process=3)
    ones = 0
    for i, ((r, rv), g, v) in enumerate(zip(orc.process_list(utts, want_vad=True), got, vads)):
        print(f"fea criterion on {entries} entries [{i}]: {v.size} VAD bytes, {int((np.asarray(v) != rv).sum()) if v.size == rv.size else -1} differ, {int((rv == ord('1')).sum())} ones")
        assert np.array_equal(np.asarray(v), rv), (extra, i)
        _assert_rows(g, r, cfg, f"{' '.join(extra)}[{i}]")
        ones += int((rv == ord("1")).sum())
    assert 0 < ones < sum(v.size for v in vads)          # decisions of both kinds


def test_fea_criterion_beyond_512_entries_is_refused(Engine):
    from ctucopy_amd.engine import CTU_ERR_UNSUPPORTED, CtuError
    from tests.util import C2
    with pytest.raises(CtuError, match="more than 512 entries") as ei:
        Engine(C2 + FEA_DYN + ["-fea_ncepcoefs", "16", "-fea_trap", "31"])      # 17 x 31 = 527
    assert ei.value.code == CTU_ERR_UNSUPPORTED
