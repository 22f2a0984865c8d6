"""bin/ctucopy --channels N, and wire input in file mode, on a device: every output file of a list of N-channel files equals, byte for
byte, the file the mono-split list gives - the list in which every `in out` line is replaced by N mono lines, channel 1 .. N, with the
targets out_<c> - under the default sharding, under --gpus 2 --gpu-map 0,0 and under --batch-mib 1.  The expected bytes come from the
plain path: the mono-split list over little-endian raw files of the channels' samples, which ctu_engine_run_host runs and no line of the
wire path touches.  The mono-split list in the files' own format (a-law, mu-law, big-endian, WAVE) is held to the same bytes, so a
mismatch names its side.  One further test pins a mono a-law list to the raw-PCM run of the samples expanded on the host (wire_expand,
pinned by tests/test_streams_wire_cpu.py), which is what the tool wrote for it before the codes went to the device as they lie.

The order of everything a list has an order for is file-major, channel-minor: the *ss noise seed (fwss), the majority filter's ring and
-vad_out (C4), the archive (ark), CMS and the delta chain per file (MFCC_0_D_A_Z), speech output (exten)."""
import os
import subprocess

import numpy as np
import pytest

from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from tests.util import C2, C4, synth_utt, wave_image

pytestmark = pytest.mark.gpu
CLI = cbuild.CLI


@pytest.fixture(scope="module", autouse=True)
def _built():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    cbuild.build_cli()


def _with(cfg, key, value):
    out = list(cfg)
    out[out.index(key) + 1] = value
    return out


def _without(cfg, key):
    i = cfg.index(key)
    return cfg[:i] + cfg[i + 2:]


def run(args, cwd):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, cwd=cwd, timeout=300)


def _codes(fmt, x):
    """G.711 codes whose expansion follows the samples x."""
    t = np.array([int(ceng.wire_expand(np.array([c], np.uint8), 0, 1, fmt=fmt)[0]) for c in range(256)])
    order = np.argsort(t, kind="stable")
    return order[np.clip(np.searchsorted(t[order], x), 0, 255)].astype(np.uint8)


def _image(kind, block, fs):
    """The bytes of a file that holds `block` ([samples, channels] int16) in the input format `kind`; extra: what the format adds to
    the command line."""
    if kind == "raw":
        return block.astype("<i2").tobytes()
    if kind == "raw_big":
        return block.astype(">i2").tobytes()
    if kind in ("alaw", "mulaw"):
        return _codes(kind, block.reshape(-1)).tobytes()
    assert kind == "wave"
    img = bytearray(wave_image(np.ascontiguousarray(block).reshape(-1), fs=fs))
    ch = block.shape[1]
    img[22:24] = ch.to_bytes(2, "little")
    img[28:32] = (fs * 2 * ch).to_bytes(4, "little")
    img[32:34] = (2 * ch).to_bytes(2, "little")
    return bytes(img)


def _format_args(cfg, kind):
    cfg = _with(cfg, "-format_in", {"raw_big": "raw"}.get(kind, kind))
    return cfg + (["-endian_in", "big"] if kind == "raw_big" else [])


def _target(name, c):
    stem, ext = os.path.splitext(name)
    return f"{stem}_{c}{ext}"


# Samples per channel of the three files.  They differ, so the sharding by length reorders them.  LONG: --batch-mib 1 is 524288 samples a
# batch, which the first channel of the second file passes - a batch that ended with the item that fills it would part that file's channels
SHORT, LONG = (5200, 3100, 7300), (180000, 170000, 60000)
# name -> (command line, sampling rate, input kind, channels, columns of a list line, output names per file, extra outputs of the run, lengths)
CASES = {
    "mfcc_0_d_a_z": (C2 + ["-fea_delta", "d_a", "-fea_Z_exp", "500"], 16000, "raw", 2, 2, ["{}.htk"], [], LONG),
    "fwss": (C2 + ["-nr_mode", "fwss", "-vad", "burg"], 16000, "raw_big", 2, 2, ["{}.htk"], [], LONG),
    "c4_vad_out": (C4, 8000, "alaw", 2, 4, ["{}.htk", "{}.vad"], [], SHORT),
    "ark": (_without(C2, "-format_out") + ["-format_out", "ark=out.ark"], 16000, "wave", 2, 2, [], ["out.ark", "out.scp"], SHORT),
    "exten_raw": ("-fs 16000 -format_in raw -format_out raw -preset exten".split(), 16000, "mulaw", 3, 2, ["{}.raw"], [], SHORT),
}
_blocks = {}


def _block(case, i):
    """File i of a case as [samples, channels] int16: what its channels are worth as samples."""
    if (case, i) not in _blocks:
        _, fs, kind, nch, _, _, _, lengths = CASES[case]
        block = np.stack([synth_utt(300 + 10 * i + c, lengths[i], fs=fs) for c in range(nch)], axis=1)
        if kind in ("alaw", "mulaw"):  # the samples of its codes
            block = np.stack([ceng.wire_expand(_codes(kind, block[:, c]), 0, lengths[i], fmt=kind) for c in range(nch)], axis=1)
        _blocks[(case, i)] = block
    return _blocks[(case, i)]


def _write_lists(cwd, case):
    """The N-channel files and their list (multi.scp), the mono files and theirs (mono.scp), in `cwd`; returns the names of the per-file
    outputs the two runs write."""
    cfg, fs, kind, nch, cols, outs, _, lengths = CASES[case]
    multi, mono, written = [], [], []
    for i in range(len(lengths)):
        block = _block(case, i)
        extra = b"\x01" if i == 1 and kind != "wave" else b""   # an incomplete [sample][channel] block at the end is dropped (WAVE: its header counts)
        (cwd / f"in{i}.bin").write_bytes(_image(kind, block, fs) + extra)
        names = [o.format(f"f{i}") for o in outs] or [f"utt{i}"]
        multi.append(" ".join([f"in{i}.bin", names[0]] + (["spk", names[1]] if cols == 4 else [])))
        for c in range(nch):
            (cwd / f"in{i}_{c + 1}.bin").write_bytes(_image(kind, block[:, c:c + 1], fs))
            (cwd / f"in{i}_{c + 1}.pcm").write_bytes(block[:, c].astype("<i2").tobytes())
            per = [_target(x, c + 1) for x in names]
            mono.append(" ".join([f"in{i}_{c + 1}.bin", per[0]] + (["spk", per[1]] if cols == 4 else [])))
            if outs:
                written += per
    (cwd / "multi.scp").write_text("\n".join(multi) + "\n")
    (cwd / "mono.scp").write_text("\n".join(mono) + "\n")
    (cwd / "plain.scp").write_text("\n".join(mono).replace(".bin ", ".pcm ") + "\n")
    return written


@pytest.mark.parametrize("case", list(CASES))
def test_channels_equal_the_mono_split_list(case, tmp_path):
    cfg, fs, kind, nch, cols, outs, extra_outs, _ = CASES[case]
    args = _format_args(cfg, kind)
    ref_dir = tmp_path / "plain"
    ref_dir.mkdir()
    written = _write_lists(ref_dir, case) + extra_outs
    r = run(_format_args(cfg, "raw") + ["-S", "plain.scp"], ref_dir)   # little-endian mono raw: ctu_engine_run_host
    assert r.returncode == 0, r.stderr
    want = {}
    for name in written:
        want[name] = (ref_dir / name).read_bytes()
        assert len(want[name]) > 0, name
    assert len(set(want.values())) > 1, "the channels differ, and so do their files"
    runs = [("mono", ["-S", "mono.scp"])]   # the mono-split list in the files' own format
    runs += [("multi" + "".join(v).replace("-", "").replace(",", ""), ["-S", "multi.scp", "--channels", nch] + v)
             for v in ([], ["--gpus", "2", "--gpu-map", "0,0"], ["--batch-mib", "1"])]
    for where, extra in runs:
        d = tmp_path / where
        d.mkdir()
        assert _write_lists(d, case) + extra_outs == written
        r = run(args + extra, d)
        assert r.returncode == 0, (where, r.stderr)
        for name in written:
            got = (d / name).read_bytes()
            if got != want[name]:
                a, b = np.frombuffer(got, np.uint8), np.frombuffer(want[name], np.uint8)
                at = int(np.argmax(a[:min(a.size, b.size)] != b[:min(a.size, b.size)])) if a.size and b.size else 0
                pytest.fail(f"{where}: {name} differs from the plain run: {a.size} against {b.size} bytes, first at byte {at}, "
                            f"{int((a[:min(a.size, b.size)] != b[:min(a.size, b.size)]).sum())} bytes in all; stderr: {r.stderr[-300:]!r}")


def _htk_rows(path):
    img = path.read_bytes()
    n, size = int(np.frombuffer(img, "<u4", 1, 0)[0]), int(np.frombuffer(img, "<u2", 1, 8)[0])
    assert size % 4 == 0 and len(img) == 12 + n * size, (str(path), n, size, len(img))
    return np.frombuffer(img, "<f4", offset=12).reshape(n, size // 4)


def test_an_idle_mu_law_channel_beside_a_speaking_one(tmp_path):
    """A call recording with a party per channel: channel 1 speaks, channel 2 is the same speech with its middle quarter muted - a run of
    code 0xFF, which expands to 0.  Behind the delta chain and the exponential CMS the all-zero frames' -inf / NaN stay to the end of the
    idle channel's file (the recurrence never recovers; tests/golden/ref_e2e_silence.npz, sil_da_zexp_e) and must not reach the other
    channel's: out_1 and out_2 hold the rows of Engine.extract on the two expanded channels, finite rows bit for bit, the same rows
    non-finite, out_1 finite throughout."""
    from ctucopy_amd import Engine
    from tests.util import zeros_mid_parts
    n = 8000
    cfg = "-fs 8000 -format_in mulaw -format_out htk -preset mfcc -fea_delta d_a -fea_Z_exp 500".split()
    speech = _codes("mulaw", synth_utt(3, n, fs=8000))
    a, z, _ = zeros_mid_parts(n)
    idle = speech.copy()
    idle[a:a + z] = 0xFF
    (tmp_path / "call.ul").write_bytes(np.stack([speech, idle], axis=1).tobytes())
    (tmp_path / "list.scp").write_text("call.ul out\n")
    x = [ceng.wire_expand(c, 0, n, fmt="mulaw") for c in (speech, idle)]
    assert not (x[1][a:a + z] != 0).any() and np.array_equal(x[1][:a], x[0][:a]) and np.abs(x[0][a:a + z].astype(int)).max() > 1000
    r = run(cfg + ["--channels", 2, "-S", "list.scp"], tmp_path)
    assert r.returncode == 0, r.stderr
    want = Engine(_with(cfg, "-format_in", "raw")).extract(x)
    got = [_htk_rows(tmp_path / f"out_{c}") for c in (1, 2)]
    for c, (g, w) in enumerate(zip(got, want), 1):
        assert g.shape == w.shape == (98, 39), (c, g.shape, w.shape)
        fg, fw = np.isfinite(g).all(axis=1), np.isfinite(w).all(axis=1)
        print(f"idle mu-law channel, out_{c}: {g.shape[0]} rows, non-finite in the file {np.flatnonzero(~fg).tolist()}, from Engine.extract {np.flatnonzero(~fw).tolist()}; "
              f"{int((g[fg & fw] != w[fg & fw]).any(axis=1).sum())} finite rows not bit-equal")
        assert np.array_equal(fg, fw), (c, np.flatnonzero(fg != fw).tolist())
        assert np.array_equal(g[fw], w[fw]), c
    f1, f2 = (np.isfinite(g).all(axis=1) for g in got)
    assert f1.all()
    # the idle channel: finite up to the delta chain's reach ahead of the first all-zero frame (sample a + 1 on: pre-emphasis), then never again
    first = -(-(a + 1) // 80) - 4
    assert f2[:first].all() and not f2[first:].any() and first >= 10, (first, np.flatnonzero(~f2).tolist())
    assert np.array_equal(got[0][:first - 4], got[1][:first - 4])      # what no window has reached yet is the speaking channel's


def test_mono_alaw_list_is_the_raw_run_of_the_expanded_samples(tmp_path):
    """-format_in alaw / mulaw / raw big-endian, mono: the files the tool writes are those of the little-endian raw run of the samples
    the host expansion gives - what it wrote when the readers expanded them."""
    for kind in ("alaw", "mulaw", "raw_big"):
        a, b = tmp_path / kind, tmp_path / (kind + "_pcm")
        a.mkdir()
        b.mkdir()
        lines = []
        for i, n in enumerate((4801, 3333)):
            x = synth_utt(500 + i, n)
            if kind == "raw_big":
                (a / f"in{i}").write_bytes(x.astype(">i2").tobytes())
            else:
                codes = _codes(kind, x)
                (a / f"in{i}").write_bytes(codes.tobytes())
                x = ceng.wire_expand(codes, 0, n, fmt=kind)
            (b / f"in{i}").write_bytes(x.astype("<i2").tobytes())
            lines.append(f"in{i} out{i}.htk")
        for d in (a, b):
            (d / "list.scp").write_text("\n".join(lines) + "\n")
        r = run(_format_args(C2, kind) + ["-S", "list.scp"], a)
        assert r.returncode == 0, r.stderr
        r = run(C2 + ["-S", "list.scp"], b)
        assert r.returncode == 0, r.stderr
        for i in range(2):
            got, want = (a / f"out{i}.htk").read_bytes(), (b / f"out{i}.htk").read_bytes()
            assert len(want) > 12 and got == want, (kind, i)
