"""HTK feature input on the GPU, through the C ABI (ctu_engine_run_rows[_host], ctu_cmvn_* on the resulting rows), against the checker of
tests/test_rows_in_cpu.py.  Values: |a - b| <= 1e-4 * max(|b|, 1); frame counts, widths and kind codes exactly; a plain conversion
bit for bit."""
import os

import numpy as np
import pytest

import ctucopy_amd
from ctucopy_amd import CtuError
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle, htk_bytes
from tests.test_rows_in_cpu import HTK, read_htk, postprocess, z_of, block_len, cmvn
from tests.util import C2, GOLDEN, sig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    ceng.load_library()  # fails loudly when the HIP extension is missing


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= 1e-4 * np.maximum(np.abs(b), 1.0)))


def mini_rows():
    z = np.load(os.path.join(GOLDEN, "mini_expected.npz"))
    return [z[k] for k in sorted(z.files) if k.startswith("c2_rows_")]


def recording_rows():
    return [Oracle(C2).process(sig(n)) for n in ("CS0", "CS3")]


def images(rows_list, big=False):
    return [htk_bytes(r, 100000, 6 | 0o20000, big_endian=big) for r in rows_list]


def pack(engine, imgs, big=False, pinned=False):
    """What a host reader does (bin/ctucopy's): header, width against -nfeacoefs, whole rows in the payload, payload bytes into the arena.
    The rows are counted by the checker's own read_htk here - the ABI takes row counts, it reads no file - so a truncated file at this
    level checks the engine on the shortened payload; the product's reader (probe_htk_rows) is exercised by tests/test_rows_in_cli.py."""
    W = engine.dims.row_floats_in
    Ts, payloads = [], []
    for img in imgs:
        rows, _, _ = read_htk(img, big)
        assert rows.shape[1] == W
        Ts.append(rows.shape[0])
        payloads.append(np.frombuffer(img[12:12 + 4 * W * rows.shape[0]], np.uint32))
    plan = engine.plan(Ts)
    arena = ceng.host_alloc((max(plan.total_samples, 1),), np.uint32) if pinned else np.zeros(max(plan.total_samples, 1), np.uint32)
    arena[:] = 0xFFFFFFFF  # the gaps between utterances are never read: NaNs there must not show
    for p, off in zip(payloads, plan.sample_off[:-1]):
        arena[off:off + p.size] = p
    return plan, arena


def run(args, imgs, big=False, how="host"):
    e = ctucopy_amd.Engine(args + (["-endian_in", "big"] if big else []))
    plan, arena = pack(e, imgs, big, pinned=(how == "pinned"))
    if how == "device":
        import torch
        words = torch.from_numpy(arena.view(np.int32)).cuda()
        rows = e.run_rows_device(plan, words).cpu().numpy()
    else:
        out = ceng.host_alloc((max(plan.total_frames, 1), e.dims.row_floats), np.float32) if how == "pinned" else None
        rows = e.run_rows_host(plan, arena, rows_out=out)[:plan.total_frames]
    res = [np.array(rows[plan.row_off[i]:plan.row_off[i + 1]]) for i in range(plan.n_utt)]
    dims = (e.dims.row_floats, e.dims.htk_kind, e.dims.htk_period)
    plan.close()
    e.close()
    return res, dims


OPTION_SETS = [
    ([], {}, 13, 6 | 0o20000),
    (["-fea_delta", "d"], dict(ws=(2,)), 26, 6 | 0o20000 | 0o400),
    (["-fea_delta", "d_a"], dict(ws=(2, 2)), 39, 6 | 0o20000 | 0o400 | 0o1000),
    (["-fea_delta", "d_a_t", "-d_win", "3", "-a_win", "1"], dict(ws=(3, 1, 2)), 52, 6 | 0o20000 | 0o400 | 0o1000 | 0o100000),
    (["-fea_trap", "5"], dict(trap=5), 65, 6 | 0o20000 | 0o400),
    (["-fea_trap", "3"], dict(trap=3), 39, 6 | 0o20000 | 0o400),
    (["-fea_Z_exp", "500"], dict(z_exp=z_of(500.0)), 13, 6 | 0o20000),
    (["-fea_Z_block", "500"], dict(block_L=block_len(500.0)), 13, 6 | 0o20000),
    (["-fea_delta", "d_a", "-fea_Z_exp", "500"], dict(ws=(2, 2), z_exp=z_of(500.0)), 39, 6 | 0o20000 | 0o400 | 0o1000),
    (["-fea_delta", "d_a", "-fea_Z_block", "300"], dict(ws=(2, 2), block_L=block_len(300.0)), 39, 6 | 0o20000 | 0o400 | 0o1000),
]


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("args,post,width,kind", OPTION_SETS)
def test_abi_equals_checker(args, post, width, kind, big):
    for name, rows_list in (("mini", mini_rows()), ("recordings", recording_rows())):
        got, dims = run(HTK + args, images(rows_list, big), big)
        assert dims == (width, kind, 100000)
        for g, r in zip(got, rows_list):
            want = postprocess(r, **post)
            assert g.shape == want.shape == (r.shape[0], width), name
            if not post or "ws" not in post and "trap" not in post:  # CMS alone is never applied to a file (src/io/batch.cc:217-226)
                assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), name  # a format conversion: the input's bits
            else:
                assert close(g, want), (name, float(np.abs(g - want).max()))


def test_plain_conversion_of_wide_rows_and_unaligned_widths_is_bit_identical():
    rng = np.random.default_rng(11)
    for W in (1, 3, 16, 39, 130):
        files = [rng.standard_normal((int(t), W)).astype(np.float32) for t in rng.integers(0, 200, 9)]
        files[3] = files[3][:0]
        for big in (False, True):
            imgs = [htk_bytes(f, 100000, 9, big_endian=big) for f in files]
            got, dims = run(HTK + ["-nfeacoefs", str(W)], imgs, big)
            assert dims[0] == W
            for g, f in zip(got, files):
                assert g.shape == f.shape and np.array_equal(g.view(np.uint32), f.view(np.uint32)), (W, big)


def test_file_shapes():
    rows = mini_rows()
    empty = rows[0][:0]
    # a zero-frame file among others; a truncated last row ends its file one row early
    imgs = images([rows[0], empty, rows[1]])
    imgs[2] = imgs[2][:-5]
    got, _ = run(HTK + ["-fea_delta", "d_a"], imgs)
    assert [g.shape for g in got] == [(rows[0].shape[0], 39), (0, 39), (rows[1].shape[0] - 1, 39)]
    assert close(got[0], postprocess(rows[0], ws=(2, 2))) and close(got[2], postprocess(rows[1][:-1], ws=(2, 2)))
    # all files empty
    got, _ = run(HTK + ["-fea_delta", "d"], images([empty, empty]))
    assert [g.shape for g in got] == [(0, 26), (0, 26)]
    # shorter than the delta window: a conversion passes it through; the chain on fewer than window + 2 frames is refused as it is
    # from audio (the reference's flush mixes frames there, tests/test_oracle_delta.py::test_window_plus_one_frames_is_not_the_closed_form)
    short = rows[2][:3]
    got, _ = run(HTK, images([short]))
    assert np.array_equal(got[0], short)
    with pytest.raises(CtuError) as ei:
        run(HTK + ["-fea_delta", "d"], images([rows[0], short]))
    assert ei.value.code == ceng.CTU_ERR_INPUT and "fewer than window+2" in str(ei.value)
    got, _ = run(HTK + ["-fea_delta", "d"], images([rows[2][:4]]))
    assert close(got[0], postprocess(rows[2][:4], ws=(2,)))
    # CMS without a chain is never applied to a file (src/io/batch.cc:217-226): no minimum, the file's bits
    got, _ = run(HTK + ["-fea_Z_block", "100"], images([short]))
    assert np.array_equal(got[0].view(np.uint32), short.view(np.uint32))


@pytest.mark.parametrize("args", [[], ["-fea_delta", "d_a"], ["-fea_delta", "d_a", "-fea_Z_exp", "500"], ["-fea_trap", "5"]])
def test_one_utterance_alone_equals_itself_in_a_batch(args):
    rows = mini_rows()
    batch, _ = run(HTK + args, images(rows))
    for i in (0, 7, len(rows) - 1):
        alone, _ = run(HTK + args, images([rows[i]]))
        assert np.array_equal(alone[0].view(np.uint32), batch[i].view(np.uint32)), i


def test_six_thousand_short_files():
    rng = np.random.default_rng(2)
    pool = np.concatenate(mini_rows())
    files = []
    for _ in range(6000):
        t = int(rng.integers(4, 24))
        a = int(rng.integers(0, pool.shape[0] - t))
        files.append(pool[a:a + t])
    got, _ = run(HTK + ["-fea_delta", "d_a", "-fea_Z_exp", "500"], images(files))
    assert len(got) == 6000
    for i in list(range(0, 6000, 97)) + [5999]:
        assert close(got[i], postprocess(files[i], ws=(2, 2), z_exp=z_of(500.0))), i
    plain, _ = run(HTK, images(files))
    assert all(np.array_equal(g, f) for g, f in zip(plain, files))


@pytest.mark.parametrize("args", [[], ["-fea_delta", "d_a", "-fea_Z_block", "300"]])
def test_host_entry_points_equal_the_device_run(args, monkeypatch):
    rows = mini_rows() * 2  # 32 utterances
    dev, _ = run(HTK + args, images(rows), how="device")
    for how in ("host", "pinned"):
        got, _ = run(HTK + args, images(rows), how=how)
        assert all(np.array_equal(g.view(np.uint32), d.view(np.uint32)) for g, d in zip(got, dev)), how
    monkeypatch.setenv("CTU_HOST_CHUNKS", "5")  # the ranges on two streams, from page-locked and from pageable buffers
    for how in ("pinned", "host"):
        got, _ = run(HTK + args, images(rows), how=how)
        assert all(np.array_equal(g.view(np.uint32), d.view(np.uint32)) for g, d in zip(got, dev)), how


def test_wrong_entry_point_is_an_error_not_a_run():
    import torch
    e = ctucopy_amd.Engine(HTK)
    plan = e.plan([10])
    with pytest.raises(CtuError, match="ctu_engine_run_rows"):
        e.run_device(plan, torch.zeros(plan.total_samples + 64, dtype=torch.int16, device="cuda"))
    with pytest.raises(CtuError, match="ctu_engine_run_rows_host"):
        e.run_host(plan, np.zeros(plan.total_samples + 64, np.int16))
    p = ctucopy_amd.Engine(C2)
    pplan = p.plan([16000])
    with pytest.raises(CtuError, match="-format_in htk"):
        p.run_rows_host(pplan, np.zeros(pplan.total_samples, np.uint32))
    with pytest.raises(CtuError, match="-format_in htk"):
        p.run_rows_device(pplan, torch.zeros(pplan.total_samples, dtype=torch.int32, device="cuda"))
    # a null arena on a plan that has frames is refused, as ctu_engine_run_rows_host refuses it
    L = ceng.load_library()
    out = np.empty((pplan.total_frames, p.dims.row_floats), np.float32)
    assert L.ctu_engine_run_host(p._h, pplan._h, None, out.ctypes.data, None, None) == ceng.CTU_ERR_INPUT
    assert L.ctu_last_error(p._h).decode() == "ENGINE: null host buffer"


def test_postprocess_binding():
    rows = mini_rows()[:3]
    for big in ([], ["-endian_in", "big"]):  # arrays are values: the byte order of files does not reach them
        e = ctucopy_amd.Engine(HTK + ["-fea_delta", "d_a"] + big)
        got = e.postprocess(rows)
        assert all(close(g, postprocess(r, ws=(2, 2))) for g, r in zip(got, rows))
        e.close()


@pytest.mark.parametrize("args,post", [([], {}), (["-fea_delta", "d_a"], dict(ws=(2, 2)))])
def test_cmvn_over_two_speakers(args, post):
    import torch
    rows = mini_rows()[:6]
    ids = ["s1", "s2", "s1", "s1", "s2", "s2"]
    e = ctucopy_amd.Engine(HTK + args + ["-apply_cmvn", "stats-not-there.txt"])
    plan, arena = pack(e, images(rows))
    d_rows = e.run_rows_device(plan, torch.from_numpy(arena.view(np.int32)).cuda())
    table, mean, var, want = cmvn([postprocess(r, **post) for r in rows], ids)
    spk = np.array([table.index(s) for s in ids], np.int32)
    cols = e.cmvn_cols()
    assert cols == e.dims.row_floats == want[0].shape[1]
    acc = e.cmvn_accumulate(plan, d_rows, spk, 2)
    assert np.array_equal(acc[:, cols], [sum(r.shape[0] for r, s in zip(rows, spk) if s == k) for k in (0, 1)])
    m = acc[:, :cols] / acc[:, cols:]
    acc2 = e.cmvn_accumulate(plan, d_rows, spk, 2, mean=m)
    v = acc2[:, :cols] / (acc2[:, cols:] - 1)
    assert close(m, mean) and close(v, var)   # statistic slot k = column k
    e.cmvn_apply(plan, d_rows, spk, 2, m, v)
    out = d_rows.cpu().numpy()
    for i, w in enumerate(want):
        assert close(out[plan.row_off[i]:plan.row_off[i + 1]], w), i
