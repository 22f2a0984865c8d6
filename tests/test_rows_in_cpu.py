"""HTK feature input (-format_in htk): layout rule, flag parsing, refusals, and the checker the GPU tests compare
the engine with - a numpy restatement of what the reference does with a feature file (htkIN, src/io/in.cc:623-709; the delta chain,
src/fea/fea_delta.cc; cms_POST / cmvn_POST, src/fea/post_impl.cc; the writers' plain copy, src/io/out.cc:177-179).

The checker is pinned here, on the CPU, against the existing oracle wherever the two paths coincide by construction: the rows
Oracle(cfg).process(pcm) writes, stored as an HTK file and post-processed by the checker, against Oracle(cfg + post options).process(pcm).
The only numeric difference allowed is the float32 round trip of the intermediate rows; the bounds are derived where they are used."""
import ctypes

import numpy as np
import pytest

import ctucopy_amd
from ctucopy_amd import CtuError, config_dims
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle, htk_bytes, cmvn_slot_columns, cmvn_speakers, cmvn_stats, cmvn_apply
from tests.test_oracle_cms import block_cms, exp_cms
from tests.test_oracle_delta import delta
from tests.util import C2, C3, sig

# -fea_rawenergy on: for dctc the reference is only defined with it (or -nr_when afterFB), see test_what_stays_refused_says_why
HTK = "-fs 16000 -format_in htk -format_out htk -preset mfcc -fea_rawenergy on".split()
PCM = sig("CS0")[: 16000 * 2]


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


# ------------------------------------------------------------------------------------------------------------------------------
# the checker
def read_htk(data, big_endian=False):
    """htkIN::new_file + get_frame: (rows [T, sampSize / 4] float32, period, kind).  T is what the payload holds in whole rows - the
    header's nSamples is not looked at, a short last row ends the file (in.cc:694)."""
    e = ">" if big_endian else "<"
    period = int(np.frombuffer(data[4:8], e + "u4")[0])
    width = int(np.frombuffer(data[8:10], e + "u2")[0]) // 4
    kind = int(np.frombuffer(data[10:12], e + "u2")[0])
    T = (len(data) - 12) // (4 * width)
    rows = np.frombuffer(data[12:12 + 4 * width * T], e + "f4").astype(np.float32).reshape(T, width)
    return rows, period, kind


def stack(x, w):
    """-fea_trap on a feature file: deltaFEA::trap with in->_fvec in FILE order (entry i = file column i), the edge rows as
    tests/test_oracle_delta.py::test_stacking_layout_and_edge_rows has them."""
    T, fc = x.shape
    L = 2 * w + 1
    out = np.zeros((T, fc * L), x.dtype)
    for t in range(T):
        for j in range(L):
            f = (0 if j < w else max(1, j - w)) if t == 0 else min(max(t - w + j, 0), T - 1)
            if w == 1 and t == T - 1:
                f = T - 1
            out[t, j:fc * L:L] = x[f]
        if t == 0 or t >= T - w:
            out[t, :fc] = x[t]
    return out


def postprocess(rows, ws=(), trap=0, z_exp=None, block_L=None):
    """One file's rows through the chain, in double; the writers cast to float32 and copy in order (out.cc:177-179).
    ws: delta windows of the chained stages; trap: -fea_trap's window (odd) instead; z_exp: the forgetting factor; block_L: frames
    of the block-CMS window.  CMS acts on the first fea_ncepcoefs+1 entries of the vector about to be written (post_impl.cc:208,217),
    after the chain - and only behind a chain: BATCH::process_frame reaches post->process_frame() through cmvn_stat() alone
    (src/io/batch.cc:198-199), which feature input enters from fea_delta() (:217-218); with neither -fea_delta nor -fea_trap the frame
    goes straight to save_frame() (:223-226) and the file is copied unchanged, whatever -fea_Z_exp / -fea_Z_block say."""
    x = rows.astype(np.float64)
    fc = x.shape[1]
    if x.shape[0] == 0:
        width = fc * (2 * ((trap - 1) // 2) + 1) if trap else fc * (len(ws) + 1)
        return np.zeros((0, width), np.float32)
    if trap:
        out = stack(x, (trap - 1) // 2)
    else:
        blocks = [x]
        for w in ws:
            blocks.append(delta(blocks[-1], w))
        out = np.concatenate(blocks, 1)
    if not ws:
        return out.astype(np.float32)  # (stacking with CMS is refused; without a chain CMS is never applied)
    if z_exp is not None:
        out[:, :fc] = exp_cms(out[:, :fc], z_exp)
    if block_L is not None:
        out[:, :fc] = block_cms(out[:, :fc], block_L)
    return out.astype(np.float32)


def z_of(Z, shift_ms=10.0):
    return float(np.float32(np.float32(1) - (2 * shift_ms) / np.float32(Z)))  # src/io/opts.cc:273-274


def block_len(Zb, window_ms=25.0, shift_ms=10.0):
    return int(np.floor((Zb - window_ms) / shift_ms)) + 1  # src/io/opts.cc:270-271


def cmvn(files_rows, speakers):
    """cmvn_POST on feature input: statistic slot k is vector entry k = column k (post_impl.cc:55-57,82-84,109-111)."""
    table, spk = cmvn_speakers(speakers)
    cols = np.arange(files_rows[0].shape[1])
    live = [(r, s) for r, s in zip(files_rows, spk)]
    mean, var, _ = cmvn_stats([r for r, _ in live], [s for _, s in live], len(table), cols)
    return table, mean, var, [cmvn_apply(r, s, mean, var, cols) for r, s in live]


# ------------------------------------------------------------------------------------------------------------------------------
def test_rows_arena_layout_rule():
    L = ceng.load_library()
    i64 = ctypes.c_int64
    rng = np.random.default_rng(5)
    for width in (1, 13, 16, 39):
        for n in (0, 1, 2, 17, 400):
            ns = rng.integers(0, 3000, size=n).astype(np.int64)
            if n > 2:
                ns[1] = 0  # a zero-frame file takes no room
            off = np.full(n + 1, -1, dtype=np.int64)
            total = L.ctu_rows_arena_layout(ns.ctypes.data_as(ctypes.POINTER(i64)), n, width, off.ctypes.data_as(ctypes.POINTER(i64)))
            assert off[0] == 0 and total == off[n]
            assert np.all(off % 4 == 0)  # 16 bytes
            assert np.all(off[1:] - off[:-1] >= ns * width) and np.all(off[1:] - off[:-1] < ns * width + 4)  # no overlap, packed
            assert L.ctu_rows_arena_layout(ns.ctypes.data_as(ctypes.POINTER(i64)), n, width, None) == total
    bad = np.array([5, -1], dtype=np.int64)
    assert L.ctu_rows_arena_layout(bad.ctypes.data_as(ctypes.POINTER(i64)), 2, 13, None) < 0
    assert L.ctu_rows_arena_layout(None, 3, 13, None) < 0
    assert L.ctu_rows_arena_layout(bad.ctypes.data_as(ctypes.POINTER(i64)), 1, 0, None) < 0


def test_flag_parser_accepts_htk_input_and_its_geometry():
    d = config_dims(HTK)
    assert (d.rows_in, d.row_floats_in, d.row_floats, d.htk_kind, d.htk_period, d.swap_in) == (1, 13, 13, 6 | 0o20000, 100000, 0)
    d = config_dims(HTK + ["-fea_delta", "d_a", "-endian_in", "big"])
    assert (d.row_floats, d.htk_kind, d.swap_in) == (39, 6 | 0o20000 | 0o400 | 0o1000, 1)
    assert config_dims(HTK + ["-fea_trap", "5"]).row_floats == 65
    d = config_dims(HTK + ["-nfeacoefs", "39"])  # a plain conversion of wider files
    assert (d.row_floats_in, d.row_floats) == (39, 39)
    assert config_dims(HTK + ["-fea_Z_exp", "500"]).row_floats == 13
    d = config_dims("-fs 8000 -format_in htk -format_out htk -preset plpc -s 5".split())  # period and kind from the options (out.cc:146-159)
    assert (d.htk_period, d.htk_kind) == (50000, 11 | 0o20000)
    assert config_dims(C2).rows_in == 0


def test_htk_input_reaches_the_device_check():
    """Without a GPU the configuration is accepted and creation fails for want of a device (it was CTU_ERR_UNSUPPORTED before)."""
    import torch
    if torch.cuda.is_available():
        e = ctucopy_amd.Engine(HTK)
        assert e.kernel_name() == "rows_ingest_kernel"
        return
    for extra in ([], ["-fea_delta", "d_a_t"], ["-fea_trap", "7"], ["-fea_Z_exp", "500"], ["-fea_Z_block", "500", "-fea_delta", "d"],
                  ["-stat_cmvn", "s.txt"], ["-nfeacoefs", "39"], ["-endian_in", "big"], ["-fea_rawenergy", "off", "-nr_when", "afterFB"],
                  ["-fea_rawenergy", "off", "-fea_kind", "lpc"]):
        with pytest.raises(CtuError) as ei:
            ctucopy_amd.Engine(HTK + extra)
        assert ei.value.code == ceng.CTU_ERR_DEVICE and "no CPU fallback" in str(ei.value), extra


@pytest.mark.parametrize("extra,why", [
    (["-fea_rawenergy", "off"], "reads nr->E"),
    (["-format_out", "raw"], "signal output"), (["-format_out", "wave"], "signal output"),
    (["-vad_out_mode", "vad", "-vad_cri_mode", "cepdist", "-vad_cepdist_mode", "in"], "vad_cepdist_mode in"),
    (["-vad_out_mode", "vad"], "VAD"), (["-vad_apply_mode", "drop", "-vad_cri_mode", "cepdist", "-vad_cepdist_mode", "fea"], "VAD"),
    (["-nr_mode", "exten"], "noise reduction"), (["-nr_mode", "hwss", "-vad", "burg"], "noise reduction"), (["-nr_rasta", "x"], "noise reduction"),
    (["-fea_kind", "trapdct,11,3"], "trapdct on input features"),
    (["-fea_E", "on"], "past the vector"), (["-fea_c0", "off"], "last entry"), (["-fea_kind", "lpa"], "last entry"),
    (["-fea_kind", "td-iir-mfcc"], "fea_kind outside"),
    (["-nfeacoefs", "39", "-fea_delta", "d"], "nfeacoefs differs"), (["-nfeacoefs", "14", "-fea_Z_exp", "500", "-fea_delta", "d"], "nfeacoefs differs"),
    (["-nfeacoefs", "39", "-format_out", "pfile=x.pf"], "pfileOUT rotates"),
    (["-fea_kind", "logspec", "-fea_delta", "d"], "non-cepstral"), (["-fea_trap", "5", "-fea_Z_exp", "500"], "stacked"),
    (["-fea_delta", "d", "-d_win", "17"], "above 16"), (["-stat_cmvn", "s", "-fea_Z_exp", "500"], "CMVN together with CMS")])
def test_what_stays_refused_says_why(extra, why):
    with pytest.raises(CtuError) as ei:
        ctucopy_amd.Engine(HTK + extra)
    assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and why in str(ei.value)


# ------------------------------------------------------------------------------------------------------------------------------
def spacing32(v):
    return float(np.spacing(np.float32(np.max(np.abs(v)))))


def test_reader_takes_the_frame_count_from_the_payload_and_both_byte_orders():
    base = Oracle(C2).process(PCM)
    for big in (False, True):
        img = htk_bytes(base, 100000, 6 | 0o20000, big_endian=big)
        rows, period, kind = read_htk(img, big)
        assert np.array_equal(rows, base) and (period, kind) == (100000, 6 | 0o20000)
        assert np.array_equal(read_htk(img[:-7], big)[0], base[:-1])  # a truncated last row ends the file in front of it
        lying = htk_bytes(base, 100000, 6, big_endian=big)
        lying = np.array([5], ">u4" if big else "<u4").tobytes() + lying[4:]
        assert read_htk(lying, big)[0].shape == base.shape        # nSamples does not decide
    assert read_htk(htk_bytes(base[:0].reshape(0, 13), 100000, 6))[0].shape == (0, 13)


@pytest.mark.parametrize("cfg", [C2, C3])
@pytest.mark.parametrize("spec,ws", [("d", (2,)), ("d_a", (2, 2)), ("d_a_t", (2, 2, 2)), ("d_a", (1, 3)), ("d_a_t", (3, 1, 2))])
def test_delta_chain_on_a_file_equals_the_oracle_on_the_audio(cfg, spec, ws):
    """The file holds (c1..cN, c0) and the chain passes it on in that order; the audio path computes on (c0, c1..cN) and its writer
    rotates every block: the same row either way.  Difference: the file's rows are float32.  A base value x is off by at most
    u = spacing(x) / 2; a stage with window w maps an input error e to at most sum_i i * 2e / (2 sum_i i^2) = e * S1 / S2 with
    S1 = sum i, S2 = sum i^2 (<= e); both sides then round the result to float32 (half a spacing each)."""
    base = Oracle(cfg).process(PCM)
    d = Oracle(cfg).dims
    rows, _, _ = read_htk(htk_bytes(base, d.period, d.htk_kind))
    got = postprocess(rows, ws=ws).astype(np.float64)
    args = ["-fea_delta", spec] + [a for f, w in zip(("-d_win", "-a_win", "-t_win"), ws) for a in (f, str(w))]
    want = Oracle(cfg + args).process(PCM).astype(np.float64)
    assert got.shape == want.shape
    fc = base.shape[1]
    assert np.array_equal(got[:, :fc], want[:, :fc])
    e = np.array([spacing32(base[:, c]) / 2 for c in range(fc)])
    for k, w in enumerate(ws):
        e = e * sum(range(1, w + 1)) / sum(i * i for i in range(1, w + 1))
        blk = slice(fc * (k + 1), fc * (k + 2))
        tol = e[None, :] + np.spacing(np.abs(want[:, blk]).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got[:, blk] - want[:, blk]) <= tol), (spec, ws, k)


def test_cms_on_a_file_behind_a_chain_equals_the_oracle_on_the_audio_and_alone_it_is_not_applied():
    """CMS walks fea_ncepcoefs+1 entries, a column at a time: the order of the columns does not matter, so behind a delta chain the file
    path and the audio path coincide.  Bounds: the input is off by u = spacing(M) / 2 (M the column's largest value); the float mean of
    either side is rounded once per frame, spacing(M) / 2 each, and the exponential recursion damps a past error by z per frame: at most
    spacing(M) / (1 - z) in the mean.  The block mean adds L floats in float on either side: L roundings of at most spacing(L M) / 2 each
    per side, divided by L: spacing(L M).  Output rounding: spacing(out).
    Without a chain the two paths differ: from audio cmvn_stat() is reached for every frame, from a file it is not (batch.cc:217-226) -
    all fea_ncepcoefs+1 columns of the file come out as they went in, where the audio path subtracts the mean from each."""
    base = Oracle(C2).process(PCM)
    d = Oracle(C2).dims
    rows, _, _ = read_htk(htk_bytes(base, d.period, d.htk_kind))
    M = np.array([spacing32(base[:, c]) for c in range(13)])
    plain = postprocess(rows, ws=(2, 2)).astype(np.float64)
    for Z in (500.0, 2000.0):
        z = z_of(Z)
        got = postprocess(rows, ws=(2, 2), z_exp=z).astype(np.float64)
        want = Oracle(C2 + ["-fea_delta", "d_a", "-fea_Z_exp", str(Z)]).process(PCM).astype(np.float64)
        assert np.array_equal(got[:, 13:], plain[:, 13:])  # after the chain, on block 0 only
        tol = M[None, :] * (1 + 1 / (1 - z)) + np.spacing(np.abs(want[:, :13]).astype(np.float32))
        assert np.all(np.abs(got[:, :13] - want[:, :13]) <= tol), Z
    for Zb in (100.0, 500.0):
        L = block_len(Zb)
        got = postprocess(rows, ws=(2, 2), block_L=L).astype(np.float64)
        want = Oracle(C2 + ["-fea_delta", "d_a", "-fea_Z_block", str(Zb)]).process(PCM).astype(np.float64)
        assert np.array_equal(got[:, 13:], plain[:, 13:])
        ML = np.array([float(np.spacing(np.float32(L * np.max(np.abs(base[:, c]))))) for c in range(13)])
        tol = M[None, :] + ML[None, :] + np.spacing(np.abs(want[:, :13]).astype(np.float32))
        assert np.all(np.abs(got[:, :13] - want[:, :13]) <= tol), Zb
    # alone: a conversion on the file path, a subtraction in every one of the 13 columns on the audio path
    for kw, args in ((dict(z_exp=z_of(500.0)), ["-fea_Z_exp", "500"]), (dict(block_L=block_len(100.0)), ["-fea_Z_block", "100"])):
        got = postprocess(rows, **kw)
        want = Oracle(C2 + args).process(PCM)
        assert np.array_equal(got, rows)
        assert all(not np.array_equal(got[:, c], want[:, c]) for c in range(13))


@pytest.mark.parametrize("tw", [3, 5, 9])
def test_stacking_a_file_differs_from_the_audio_path_by_one_block(tw):
    """deltaFEA::trap lays entry i of its input at X[i*L .. i*L+L).  From audio entry 0 is c0; from a file (c1..cN, c0) entry 0 is c1:
    the file's stacked row holds c1's context in block 0 .. cN's in block N-1 and c0's in the last block, where the audio path has c0's in
    block 0 and c_i's in block i.  On the rows the edge rule does not touch (0 < t < T - w), block i of the file path is block (i + 1) mod
    (N + 1) of the audio path - every column moves by L, the c0 block from the front to the back."""
    base = Oracle(C2).process(PCM)
    w, L = (tw - 1) // 2, tw
    got = postprocess(base, trap=tw)
    want = Oracle(C2 + ["-fea_trap", str(tw)]).process(PCM)
    T = base.shape[0]
    assert got.shape == want.shape == (T, 13 * L)
    inner = slice(1, T - w)
    for i in range(13):
        assert np.array_equal(got[inner, i * L:(i + 1) * L], want[inner, ((i + 1) % 13) * L:((i + 1) % 13 + 1) * L]), i
    assert not np.array_equal(got[inner], want[inner])
    # the edge rows carry the centre frame's vector in their first N+1 slots, in the order of the input: file order here
    for t in (0, T - 1):
        assert np.array_equal(got[t, :13], base[t]) and np.array_equal(want[t, :13], np.concatenate([base[t, 12:], base[t, :12]]))


def test_cmvn_statistics_on_files_are_in_column_order():
    """cmvn_POST adds F[i] to slot i for feature input (post_impl.cc:55-57), and entry i+1 to slot i (entry 0 to the last slot) for audio
    (:59-61).  With one block both put c1..cN in slots 0..N-1 and c0 in slot N: the same statistics file.  With deltas the audio path's
    vector is (c0, c1..cN, dc0, dc1.. ), so its slot N is dc0 - row column 2N+1 - and c0 (column N) sits in the LAST slot; the file path's
    slot k is column k.  The normalised rows are the same either way (every column gets its own mean and variance)."""
    pcms = [PCM[:16000], PCM[8000:30000], PCM[4000:20000]]
    ids = ["a", "b", "a"]
    for args, nb in (([], 1), (["-fea_delta", "d_a"], 3)):
        rows = [Oracle(C2 + args).process(p) for p in pcms]  # what the chain hands to cmvn_POST, as rows
        table, mean, var, out = cmvn(rows, ids)
        t2, spk = cmvn_speakers(ids)
        cols = cmvn_slot_columns(12, nb)
        m2, v2, _ = cmvn_stats(rows, spk, len(t2), cols)
        assert table == t2 and np.array_equal(mean[:, cols], m2) and np.array_equal(var[:, cols], v2)
        if nb == 1:
            assert np.array_equal(cols, np.arange(13))
        else:
            assert cols[12] == 25 and cols[25] == 38 and cols[38] == 12 and np.array_equal(cols[:12], np.arange(12))
        for r, s, o in zip(rows, spk, out):
            assert np.array_equal(o, cmvn_apply(r, s, m2, v2, cols))
