"""Kaldi compressed matrices on a MI355X (csrc/kaldi_cm.hip): the device decode against the float64 oracle of
tests/kaldi_compress_ref.py and bitwise against kaldi_io_lite.load_mat, the device encode byte for byte against the oracle's
scalar float32 encoder, ResidentSegmentPool over a compressed archive, and prepare_kaldi_data.py --compress end to end.

Decode tolerance: 2^-21 (|min_value| + range) (kaldi_compress_ref.tol); everything else is equality."""
import os
import struct

import numpy as np
import pytest
import torch

import kaldi_compress_ref as R
from test_feats_cpu import _write_wav
from test_kaldi_compress_cpu import encode_cases, fbank_like, hand_built

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "tests", "golden", "kaldi_fbank.conf")


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


def device_decode(hb, entries, n_frames=None, fill=None):
    """entries: (token, min_value, range, rows, cols, payload) with one column count -> (list of decoded arrays, status)."""
    F = entries[0][4]
    rows = [e[3] for e in entries]
    row0 = np.concatenate([[0], np.cumsum(rows)[:-1]])
    desc, n_tiles, n_bytes = hb.kaldi_cm_descs([e[0] for e in entries], rows, F, row0, [(e[1], e[2]) for e in entries])
    buf = np.zeros(n_bytes, np.uint8)
    for e, off in zip(entries, desc["payload_off"]):
        buf[int(off):int(off) + len(e[5])] = np.frombuffer(e[5], np.uint8)
    out = torch.full((sum(rows) if n_frames is None else n_frames, F), 12345.0 if fill is None else fill, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    hb.kaldi_decompress(torch.from_numpy(buf).cuda(), torch.from_numpy(desc.view(np.uint8)).cuda(), n_tiles, out, status)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return [o[a:a + r] for a, r in zip(row0, rows)], int(status.item())


def coded(rng, token_method, rows, cols):
    m = fbank_like(rng, rows, cols)
    tok, header, payload = R.encode(m, token_method)
    mn, rg = struct.unpack("<ff", header[:8])
    return (tok, mn, rg, rows, cols, payload)


@pytest.mark.parametrize("cols", [80, 23, 260])
def test_decode_mixed_ragged_batch(hb, cols):
    """All three tokens, 1 row, 9 rows, row counts around the tile, many columns (more than one LDS pass), columns that are
    no multiple of 4 (the scalar store path)."""
    import kaldi_io_lite as K

    rng = np.random.default_rng(cols)
    T = hb.KALDI_CM_TILE_ROWS
    plan = [("auto", 9), ("auto", 1), ("one-byte", 1), ("auto", T), ("auto", T + 1), ("auto", 3 * T - 1), ("two-byte", 2 * T + 5),
            ("one-byte", T + 3), ("auto", 8), ("auto", 517), ("one-byte", 40), ("auto", 1001), ("auto", 10)]
    entries = [coded(rng, m, r, cols) for m, r in plan]
    assert {e[0] for e in entries} == {"CM", "CM2", "CM3"}
    got, status = device_decode(hb, entries)
    assert status == 0
    for e, g in zip(entries, got):
        want = R.decode(*e)
        host = K.decompress(*e)
        err = np.abs(g.astype(np.float64) - want).max()
        print("%s %dx%d: worst device decode error %.3g, tolerance %.3g" % (e[0], e[3], e[4], err, R.tol(e[1], e[2])))
        assert err <= R.tol(e[1], e[2])
        assert np.array_equal(g.view(np.uint32), host.view(np.uint32)), (e[0], e[3])


def test_decode_hand_built_entries(hb):
    import kaldi_io_lite as K

    for e in hand_built():
        (g,), status = device_decode(hb, [e])
        assert status == 0
        assert np.abs(g.astype(np.float64) - R.decode(*e)).max() <= R.tol(e[1], e[2])
        assert np.array_equal(g.view(np.uint32), K.decompress(*e).view(np.uint32))


def test_decode_refuses_bad_descriptors(hb):
    rng = np.random.default_rng(1)
    entries = [coded(rng, "auto", 200, 40), coded(rng, "auto", 50, 40)]
    # the matrix is one row short of what the descriptors name: nothing is written
    got, status = device_decode(hb, entries, n_frames=249)
    assert status == hb.KALDI_CM_BAD_DESC and all(np.all(g == 12345.0) for g in got)


def device_encode(hb, mats, method):
    import features as FE

    feats = torch.from_numpy(np.concatenate(mats, axis=0)).cuda()
    return FE.kaldi_compress(feats, [len(m) for m in mats], method)


def test_encode_bytes_equal_oracle(hb):
    groups = {}
    for name, m, method in encode_cases():
        groups.setdefault((m.shape[1], method), []).append((name, m))
    for (cols, method), items in groups.items():
        got = device_encode(hb, [m for _, m in items], method)  # one batch per column count and method
        for (name, m), c in zip(items, got):
            tok, header, payload = R.encode(m, method)
            assert c.token == tok and c.header == header, name
            if c.payload != payload:
                a, b = np.frombuffer(c.payload, np.uint8), np.frombuffer(payload, np.uint8)
                bad = np.flatnonzero(a != b)
                raise AssertionError("%s: %d of %d payload bytes differ, first at %d: %d != %d" % (name, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]]))


def test_encode_long_utterance_and_odd_columns(hb):
    rng = np.random.default_rng(77)
    long = fbank_like(rng, 200003, 4)  # beyond any buffer a workgroup could hold: the select streams it
    long[1000:5000, 1] = long[0, 1]  # a long run of equal values around the quartiles' buckets
    odd = fbank_like(rng, 333, 5)
    for m in (long, odd):
        (c,) = device_encode(hb, [m], "auto")
        tok, header, payload = R.encode(m)
        assert c.token == tok == "CM" and c.header == header
        assert c.payload[:8 * m.shape[1]] == payload[:8 * m.shape[1]], "column headers"
        assert c.payload == payload


def test_encode_names_non_finite_utterances(hb):
    import features as FE

    rng = np.random.default_rng(3)
    mats = [fbank_like(rng, 30, 8) for _ in range(3)]
    mats[1][7, 2] = np.nan
    with pytest.raises(ValueError, match="second"):
        FE.kaldi_compress(torch.from_numpy(np.concatenate(mats)).cuda(), [30, 30, 30], "auto", names=["first", "second", "third"])


def test_pool_over_compressed_archive_is_bitwise(hb, tmp_path):
    import datasets as D
    import kaldi_io_lite as K

    rng = np.random.default_rng(11)
    mats = [("spk%d_u%d" % (j % 3, j), fbank_like(rng, int(n), 80)) for j, n in enumerate((145, 20, 19, 388, 31, 8, 1030, 64))]
    cdir, fdir, xdir = tmp_path / "c", tmp_path / "f", tmp_path / "x"
    for d in (cdir, fdir, xdir):
        d.mkdir()
        K.write_len_scp(d / "len.scp", [(k, len(m)) for k, m in mats])
    K.write_ark_scp(str(cdir / "feats.ark"), str(cdir / "feats.scp"), mats, compress="auto")
    decoded = list(K.read_ark(cdir / "feats.ark"))
    K.write_ark_scp(str(fdir / "feats.ark"), str(fdir / "feats.scp"), decoded)
    # a mixed archive: every other entry compressed, the others stored as their decoded float32 copy
    K.write_ark_scp(str(xdir / "feats.ark"), str(xdir / "feats.scp"),
                    [(k, K.CompressedMatrix(K.compress_mat(m)[0], K.header_bytes(m), K.compress_mat(m)[1]) if j % 2 else dm)
                     for j, ((k, m), (_, dm)) in enumerate(zip(mats, decoded))])
    pools = []
    for d in (cdir, fdir, xdir):
        ds = D.KaldiDataset(d / "feats.scp", d / "len.scp", min_len=8, mvn_path=str(d / "mvn.json"), seg_len=8, seg_shift=4)
        pools.append(D.ResidentSegmentPool(ds))
    assert pools[0].pool.shape == (sum(len(m) for _, m in mats), 80)
    for p in pools[1:]:
        assert torch.equal(pools[0].pool.view(torch.int32), p.pool.view(torch.int32))
    ids = torch.arange(16, device="cuda")
    for a, b in zip(pools[0].batch(ids), pools[1].batch(ids)):
        assert torch.equal(a, b)
    # small batches: one decode launch per few utterances gives the same pool
    ds = D.KaldiDataset(cdir / "feats.scp", cdir / "len.scp", min_len=8, mvn_path=str(cdir / "mvn.json"), seg_len=8, seg_shift=4)
    old = D.ResidentSegmentPool.CM_BATCH_BYTES
    D.ResidentSegmentPool.CM_BATCH_BYTES = 40000
    try:
        small = D.ResidentSegmentPool(ds)
    finally:
        D.ResidentSegmentPool.CM_BATCH_BYTES = old
    assert torch.equal(small.pool.view(torch.int32), pools[0].pool.view(torch.int32))


def test_prepare_kaldi_data_compress_end_to_end(hb, tmp_path, capsys):
    import kaldi_fbank_ref as FR
    import kaldi_io_lite as K
    import prepare_kaldi_data as PK
    import train_model as TM

    sr = 16000
    rng = np.random.default_rng(3)
    roots = {}
    for mode in ("plain", "coded"):
        d = tmp_path / mode / "train"
        d.mkdir(parents=True)
        roots[mode] = d
    lines = {m: [] for m in roots}
    for j in range(5):
        key = "spk%d_utt%d" % (j % 2, j)
        n = int(rng.integers(8000, 20000))
        q = FR.probe(sr, n / sr + 0.01, 50 + j)[:n].astype(np.int64)
        for mode, d in roots.items():
            _write_wav(d / (key + ".wav"), q[:, None], sr, 2)
            lines[mode].append("%s %s\n" % (key, d / (key + ".wav")))
    for mode, d in roots.items():
        (d / "wav.scp").write_text("".join(lines[mode]))
    assert PK.main([str(tmp_path / "plain"), "--fbank_conf", CONF, "--set_name", "train", "--seed", "5"]) == 0
    assert PK.main([str(tmp_path / "coded"), "--fbank_conf", CONF, "--set_name", "train", "--seed", "5", "--compress"]) == 0
    capsys.readouterr()
    plain, codedd = roots["plain"], roots["coded"]
    ratio = os.path.getsize(codedd / "feats.ark") / os.path.getsize(plain / "feats.ark")
    print("feats.ark: compressed / uncompressed = %.4f" % ratio)
    assert ratio < 0.3
    assert (codedd / "len.scp").read_text() == (plain / "len.scp").read_text()
    pl, cl = (plain / "feats.scp").read_text().splitlines(), (codedd / "feats.scp").read_text().splitlines()
    assert [l.split()[0] for l in pl] == [l.split()[0] for l in cl] and len(pl) == 5
    for a, b in zip(pl, cl):
        want = K.load_mat(a.split(None, 1)[1])
        tok, mn, rg, rows, cols, payload = K.read_raw(b.split(None, 1)[1])
        got = K.load_mat(b.split(None, 1)[1])
        assert tok == "CM" and got.shape == want.shape == (rows, cols) and cols == 80
        # the device coded what the host codes from the same features
        assert (tok, payload) == K.compress_mat(want) and struct.pack("<ffii", mn, rg, rows, cols) == K.header_bytes(want)
        # half a quantisation step of the value's own segment, plus one step of the 16-bit levels and the decode tolerance
        for j in range(cols):
            P0, P25, P75, P100 = R.column_levels(mn, rg, struct.unpack_from("<4H", payload, 8 * j))
            v = want[:, j].astype(np.float64)
            half = np.where(v < P25, (P25 - P0) / 128, np.where(v < P75, (P75 - P25) / 256, (P100 - P75) / 126))
            err = np.abs(got[:, j].astype(np.float64) - v)
            assert np.all(err <= half + float(rg) / 65535 + R.tol(mn, rg)), (j, float(err.max()))
    exp = tmp_path / "exp"
    argv = ["--data-format", "kaldi", "--train-feat-scp", str(codedd / "feats.scp"), "--train-len-scp", str(codedd / "len.scp"),
            "--dev-feat-scp", str(codedd / "feats.scp"), "--dev-len-scp", str(codedd / "len.scp"),
            "--mvn-path", str(tmp_path / "mvn.json"), "--z1-hus", "16", "16", "--z2-hus", "16", "16", "--x-hus", "16", "16",
            "--z1-dim", "8", "--z2-dim", "8", "--epochs", "1", "--training-batch-size", "16", "--exp-dir", str(exp)]
    rc = TM.main(argv)
    text = capsys.readouterr().out
    assert rc == 0 and "Training complete!" in text and "KaldiDataset: 5 out of 5 kept" in text, text
    lb = [float(l.split("lower bound:")[1].split()[0]) for l in text.splitlines() if "Validation set lower bound" in l]
    assert len(lb) == 1 and np.isfinite(lb[0])
    import datasets as D

    ds = D.KaldiDataset(codedd / "feats.scp", codedd / "len.scp", min_len=20, mvn_path=str(tmp_path / "mvn.json"), seg_len=20, seg_shift=8)
    assert ds.num_segments >= 32  # at least two batches of 16 were trained on
