"""bin/ctucopy -format_in htk over a list: htk -> htk, ark and pfile; one engine and two; CMVN over the list.  Files whose values are
exact (a plain conversion) are compared byte for byte with what the checker and the Python mirrors of the writers below produce,
the others value by value under |a - b| <= 1e-4 * max(|b|, 1) with everything else - sizes, headers, tables - exact."""
import os
import struct
import subprocess

import numpy as np
import pytest

from ctucopy_amd import build as cbuild
from oracle.oracle import htk_bytes, cmvn_stat_text
from tests.test_rows_in import close, mini_rows
from tests.test_rows_in_cpu import HTK, postprocess, cmvn

pytestmark = pytest.mark.gpu
CLI = cbuild.CLI
KIND = 6 | 0o20000
HTK_IN = "-fs 16000 -format_in htk -preset mfcc -fea_rawenergy on".split()  # HTK without its -format_out


@pytest.fixture(scope="module", autouse=True)
def _built():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    cbuild.build_all()


def run(args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def ark_bytes(keys, rows_list):
    """arkOUT (src/io/out.cc:680-754) as ctucopy_amd/host/main.cc writes it: key, " \\0BFM \\4", rows, "\\4", columns, float32 rows."""
    out, idx = b"", []
    for k, r in zip(keys, rows_list):
        out += k.encode() + b" \0BFM \4"
        idx.append(len(out) - 6)
        out += struct.pack("<i", r.shape[0]) + b"\4" + struct.pack("<i", r.shape[1]) + r.astype("<f4").tobytes()
    return out, idx


def pfile_rotate(r, fc):
    """pfileOUT::save_frame has no branch for feature input (src/io/out.cc:280-303): entry 0 of every block of fea_ncepcoefs+1 goes behind
    the block's other entries, although the file already has its c0 there."""
    out = r.copy()
    for b in range(r.shape[1] // fc):
        out[:, b * fc:(b + 1) * fc] = np.roll(r[:, b * fc:(b + 1) * fc], -1, axis=1)
    return out


def pfile_bytes(rows_list):
    nf = rows_list[0].shape[1]
    data, starts, n = b"", [0], 0
    for s, r in enumerate(rows_list):
        for t in range(r.shape[0]):
            data += struct.pack(">II", s, t) + r[t].astype(">f4").tobytes()
        n += r.shape[0]
        starts.append(n)
    h = "-pfile_header version 0 size 32768\n-num_sentences %d\n-num_frames %d\n-first_feature_column 2\n-num_features %d\n" % (len(rows_list), n, nf)
    h += "-first_label_column %d\n-num_labels 0\n-format dd%s\n" % (2 + nf, "f" * nf)
    h += "-data size %d offset 0 ndim 2 nrow %d ncol %d\n-sent_table_data size %d offset %d ndim 1\n-end\n" % ((nf + 2) * n, n, nf + 2, len(starts), (nf + 2) * n)
    return h.encode().ljust(32768, b"\0") + data + b"".join(struct.pack(">I", s) for s in starts)


def write_inputs(tmp_path, rows_list, big=False, tag="in"):
    names = []
    for i, r in enumerate(rows_list):
        p = tmp_path / f"{tag}{i}.htk"
        p.write_bytes(htk_bytes(r, 12345, 9, big_endian=big))  # period and kind of the input header are not carried over (src/io/out.cc:146-159)
        names.append(p)
    return names


def test_htk_to_htk_ark_and_pfile(tmp_path):
    rows = mini_rows()[:5]
    rows[2] = rows[2][:0]  # a zero-frame file
    for big_in in (False, True):
        names = write_inputs(tmp_path, rows, big_in, tag="b" if big_in else "l")
        endian = ["-endian_in", "big"] if big_in else []
        outs = [tmp_path / f"o{i}.htk" for i in range(len(rows))]
        lst = tmp_path / "l.scp"
        lst.write_text("".join(f"{a} {b}\n" for a, b in zip(names, outs)))
        # conversion: byte-identical, in both output byte orders
        for big_out in (False, True):
            r = run(HTK + endian + ["-S", str(lst)] + (["-endian_out", "big"] if big_out else []))
            assert r.returncode == 0, r.stderr
            for o, x in zip(outs, rows):
                assert o.read_bytes() == htk_bytes(x, 100000, KIND, big_endian=big_out)
        # delta + CMS: headers exact, values to the bound
        r = run(HTK + endian + ["-fea_delta", "d_a", "-fea_Z_exp", "500", "-S", str(lst)])
        assert r.returncode == 0, r.stderr
        for o, x in zip(outs, rows):
            img = o.read_bytes()
            assert struct.unpack("<IIHH", img[:12]) == (x.shape[0], 100000, 156, KIND | 0o400 | 0o1000) and len(img) == 12 + 156 * x.shape[0]
            z = float(np.float32(np.float32(1) - 20.0 / np.float32(500.0)))
            assert close(np.frombuffer(img[12:], "<f4").reshape(-1, 39), postprocess(x, ws=(2, 2), z_exp=z))
        # stacking keeps the kind code of the options in every header (htkOUT's branch for feature input does not rewrite fea_kind)
        r = run(HTK + endian + ["-fea_trap", "5", "-S", str(lst)])
        assert r.returncode == 0, r.stderr
        for o, x in zip(outs, rows):
            img = o.read_bytes()
            assert struct.unpack("<IIHH", img[:12]) == (x.shape[0], 100000, 260, KIND | 0o400)
            assert close(np.frombuffer(img[12:], "<f4").reshape(-1, 65), postprocess(x, trap=5))
        # ark + scp
        keys = [f"utt{i}" for i in range(len(rows))]
        lst.write_text("".join(f"{a} {k}\n" for a, k in zip(names, keys)))
        ark = tmp_path / "t.ark"
        r = run(HTK_IN + endian + ["-format_out", f"ark={ark}", "-S", str(lst)])
        assert r.returncode == 0, r.stderr
        want, idx = ark_bytes(keys, rows)
        assert ark.read_bytes() == want
        assert (tmp_path / "t.scp").read_text() == "".join(f"{k} {ark}:{i}\n" for k, i in zip(keys, idx))
        # pfile: the rotation the reference's pfile writer applies to feature input too
        pf = tmp_path / "t.pfile"
        r = run(HTK_IN + endian + ["-format_out", f"pfile={pf}", "-S", str(lst)])
        assert r.returncode == 0, r.stderr
        assert pf.read_bytes() == pfile_bytes([pfile_rotate(x, 13) for x in rows])
        # behind a delta chain: ark rows as they are, the pfile writer's rotation in each of the three blocks of 13
        want39 = [postprocess(x, ws=(2, 2)) for x in rows]
        r = run(HTK_IN + endian + ["-fea_delta", "d_a", "-format_out", f"ark={ark}", "-S", str(lst)])
        assert r.returncode == 0, r.stderr
        img, (ref, idx) = ark.read_bytes(), ark_bytes(keys, want39)
        assert len(img) == len(ref) and (tmp_path / "t.scp").read_text() == "".join(f"{k} {ark}:{i}\n" for k, i in zip(keys, idx))
        for k, i, x in zip(keys, idx, want39):
            n = x.shape[0]
            assert img[i - len(k) - 1:i + 15] == ref[i - len(k) - 1:i + 15]  # key, marker, rows, columns
            assert close(np.frombuffer(img[i + 15:i + 15 + 156 * n], "<f4").reshape(n, 39), x)
        r = run(HTK_IN + endian + ["-fea_delta", "d_a", "-format_out", f"pfile={pf}", "-S", str(lst)])
        assert r.returncode == 0, r.stderr
        img, ref = pf.read_bytes(), pfile_bytes([pfile_rotate(x, 13) for x in want39])
        n = sum(x.shape[0] for x in rows)
        assert len(img) == len(ref) and img[:32768] == ref[:32768] and img[32768 + 164 * n:] == ref[32768 + 164 * n:]
        got = np.frombuffer(img[32768:32768 + 164 * n], ">u4").reshape(n, 41)
        exp = np.frombuffer(ref[32768:32768 + 164 * n], ">u4").reshape(n, 41)
        assert np.array_equal(got[:, :2], exp[:, :2])   # sentence, frame
        assert close(got[:, 2:].astype("<u4").view("<f4"), exp[:, 2:].astype("<u4").view("<f4"))


def test_reader_refuses_what_it_cannot_reproduce(tmp_path):
    rows = mini_rows()[:2]
    names = write_inputs(tmp_path, rows)
    wide = tmp_path / "wide.htk"
    wide.write_bytes(htk_bytes(np.zeros((4, 14), np.float32), 100000, 9))
    lst = tmp_path / "l.scp"
    lst.write_text(f"{names[0]} {tmp_path / 'a.out'}\n{wide} {tmp_path / 'b.out'}\n")
    r = run(HTK + ["-S", str(lst)])
    assert r.returncode != 0 and "-nfeacoefs says 13" in r.stderr
    # a truncated last row ends its file one row early, whatever the header says
    cut = tmp_path / "cut.htk"
    cut.write_bytes(names[1].read_bytes()[:-9])
    lst.write_text(f"{cut} {tmp_path / 'c.out'}\n")
    r = run(HTK + ["-S", str(lst)])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "c.out").read_bytes() == htk_bytes(rows[1][:-1], 100000, KIND)


def test_one_engine_and_two_engines_write_the_same_files(tmp_path):
    import torch
    rows = mini_rows()
    names = write_inputs(tmp_path, rows)
    outs = {}
    for tag, extra in (("one", []), ("two", ["--gpus", "2"] + ([] if torch.cuda.device_count() >= 2 else ["--gpu-map", "0,0"]))):
        d = tmp_path / tag
        d.mkdir()
        (d / "list").write_text("".join(f"{a} {d / ('u%d.out' % i)}\n" for i, a in enumerate(names)))
        r = run(HTK + ["-fea_delta", "d_a", "-fea_Z_block", "300", "-S", str(d / "list"), "--batch-mib", "1"] + extra)
        assert r.returncode == 0, r.stderr
        outs[tag] = {p.name: p.read_bytes() for p in sorted(d.iterdir()) if p.name != "list"}
    assert len(outs["one"]) == len(rows) and outs["one"] == outs["two"]


def test_cmvn_over_the_list(tmp_path):
    rows = mini_rows()[:6]
    ids = ["s1", "s2", "s1", "s1", "s2", "s2"]
    names = write_inputs(tmp_path, rows)
    for args, post in (([], {}), (["-fea_delta", "d_a"], dict(ws=(2, 2)))):
        table, mean, var, want = cmvn([postprocess(r, **post) for r in rows], ids)
        # statistics only: "<in> <speaker>"
        lst = tmp_path / "stat.scp"
        lst.write_text("".join(f"{a} {s}\n" for a, s in zip(names, ids)))
        stat = tmp_path / "cmvn.stat"
        r = run(HTK + args + ["-stat_cmvn", str(stat), "-S", str(lst)])
        assert r.returncode == 0, r.stderr
        text, wtext = stat.read_text(), cmvn_stat_text(table, mean, var)
        assert [l.split("\t")[0] for l in text.splitlines()] == [l.split("\t")[0] for l in wtext.splitlines()]
        got_vals = np.array([[float(v) for v in l.split("\t")[1].split()] for l in text.splitlines() if "\t" in l])
        want_vals = np.array([[float(v) for v in l.split("\t")[1].split()] for l in wtext.splitlines() if "\t" in l])
        assert got_vals.shape == want_vals.shape == (4, want[0].shape[1]) and close(got_vals, want_vals)
        # compute + apply
        outs = [tmp_path / f"n{i}.out" for i in range(len(rows))]
        lst.write_text("".join(f"{a} {o} {s}\n" for a, o, s in zip(names, outs, ids)))
        stat2 = tmp_path / "cmvn2.stat"
        if stat2.exists():
            stat2.unlink()
        r = run(HTK + args + ["-apply_cmvn", str(stat2), "-S", str(lst)])
        assert r.returncode == 0, r.stderr
        for o, w in zip(outs, want):
            img = o.read_bytes()
            assert struct.unpack("<IIHH", img[:12])[::2] == (w.shape[0], 4 * w.shape[1])
            assert close(np.frombuffer(img[12:], "<f4").reshape(w.shape), w)
