"""Kaldi compressed matrices (CM, CM2, CM3) without a GPU: kaldi_io_lite's decode of hand-built entries against the float64
oracle of tests/kaldi_compress_ref.py, compress_mat byte for byte against the oracle's scalar float32 encoder, the
container (scp offsets, mixed archives, refusals) and KaldiDataset over a compressed archive.

Decode tolerance: 2^-21 (|min_value| + range), eight half-ulps of float32 at the matrix's scale (kaldi_compress_ref.tol)."""
import os
import struct

import numpy as np
import pytest

import kaldi_compress_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def K():
    import kaldi_io_lite

    return kaldi_io_lite


def fbank_like(rng, rows, cols):
    """float32 values in [-16, 12] with a per-column level and spread, like log mel energies."""
    level = rng.uniform(-10.0, 6.0, size=(1, cols))
    m = level + rng.standard_normal((rows, cols)) * rng.uniform(0.5, 3.0, size=(1, cols))
    return np.clip(m, -16.0, 12.0).astype(np.float32)


ENCODE_SHAPES = [(9, 23), (10, 40), (11, 80), (64, 23), (129, 40), (517, 80), (1000, 23), (3000, 40)]


def encode_cases():
    """(name, matrix, method) of every encoder case: random fbank-like matrices, a constant matrix, a constant column,
    1 to 8 rows, and the two explicit methods."""
    rng = np.random.default_rng(2024)
    cases = [("fbank %dx%d" % s, fbank_like(rng, *s), "auto") for s in ENCODE_SHAPES]
    cases.append(("constant", np.full((20, 5), -3.25, np.float32), "auto"))
    cases.append(("constant zero", np.zeros((12, 3), np.float32), "auto"))
    for name, first, second in (("minus zero first", -0.0, 0.0), ("plus zero first", 0.0, -0.0)):
        m = np.abs(fbank_like(rng, 20, 7))  # minimum zero, both zeros present: the header holds +0.0
        m[3, 1], m[11, 4] = first, second
        cases.append((name, m, "auto"))
    cases.append(("all zeros of both signs", np.where(np.arange(36).reshape(12, 3) % 2 == 0, np.float32(-0.0), np.float32(0.0)), "auto"))
    m = fbank_like(rng, 50, 6)
    m[:, 2] = m[0, 2]
    cases.append(("constant column", m, "auto"))
    for rows in range(1, 9):
        cases.append(("%d rows" % rows, fbank_like(rng, rows, 23), "auto"))
    cases.append(("two-byte", fbank_like(rng, 40, 23), "two-byte"))
    cases.append(("one-byte", fbank_like(rng, 40, 23), "one-byte"))
    cases.append(("one-byte 3 rows", fbank_like(rng, 3, 40), "one-byte"))
    return cases


def hand_built():
    """One entry per token, built with struct: (token, min_value, range, rows, cols, payload)."""
    mn, rg = np.float32(-15.7), np.float32(27.3)
    # CM, 12 rows x 3 columns: header words at their clamps, the bytes at every segment edge
    heads = [(65532, 65533, 65534, 65535), (0, 1, 2, 3), (1000, 20000, 40000, 65535)]
    col = [0, 64, 65, 192, 193, 255, 1, 63, 128, 191, 254, 100]
    cm = b"".join(struct.pack("<4H", *h) for h in heads) + bytes(col) + bytes(col[::-1]) + bytes((7 * c + 3) % 256 for c in col)
    out = [("CM", mn, rg, 12, 3, cm)]
    # CM, one column
    out.append(("CM", np.float32(0.5), np.float32(1e-3), 9, 1, struct.pack("<4H", 10, 2000, 50000, 65535) + bytes([0, 64, 65, 192, 193, 255, 32, 96, 224])))
    # CM2, one row, and CM2 with several; CM3
    out.append(("CM2", mn, rg, 1, 5, struct.pack("<5H", 0, 1, 32768, 65534, 65535)))
    out.append(("CM2", np.float32(3.0), np.float32(1000.0), 3, 2, struct.pack("<6H", 65535, 0, 12345, 54321, 2, 65533)))
    out.append(("CM3", mn, rg, 2, 6, bytes([0, 64, 65, 192, 193, 255, 255, 1, 2, 127, 128, 254])))
    return out


# ------------------------------------------------------------------------------------------------------------------ decode
def test_decode_hand_built_entries(K, tmp_path):
    ark = tmp_path / "hand.ark"
    blob, offs = b"", []
    entries = hand_built()
    for j, (tok, mn, rg, rows, cols, payload) in enumerate(entries):
        assert len(payload) == R.payload_size(tok, rows, cols)
        key = "k%d" % j
        offs.append(len(blob) + len(key) + 1)
        blob += R.entry(key, tok, struct.pack("<ffii", mn, rg, rows, cols), payload)
    ark.write_bytes(blob)
    streamed = list(K.read_ark(ark))
    assert [k for k, _ in streamed] == ["k%d" % j for j in range(len(entries))]
    for (tok, mn, rg, rows, cols, payload), off, (_, via_ark) in zip(entries, offs, streamed):
        want = R.decode(tok, mn, rg, rows, cols, payload)
        got = K.load_mat("%s:%d" % (ark, off))
        assert got.dtype == np.float32 and got.shape == (rows, cols) and got.flags["C_CONTIGUOUS"]
        err = np.abs(got.astype(np.float64) - want).max()
        print("%s %dx%d: worst decode error %.3g, tolerance %.3g" % (tok, rows, cols, err, R.tol(mn, rg)))
        assert err <= R.tol(mn, rg)
        assert np.array_equal(got.view(np.uint32), via_ark.view(np.uint32))
        raw = K.read_raw("%s:%d" % (ark, off))
        assert raw[0] == tok and raw[1] == mn and raw[2] == rg and raw[3:5] == (rows, cols) and bytes(raw[5]) == payload
    # facts of the format: byte 0 / 255 of a column are P0 / P100, CM2 word 0 / 65535 are min and min + range
    tok, mn, rg, rows, cols, payload = entries[0]
    got = K.load_mat("%s:%d" % (ark, offs[0]))
    P = R.column_levels(mn, rg, (1000, 20000, 40000, 65535))
    assert abs(got[0, 0] - R.column_levels(mn, rg, (65532,))[0]) <= R.tol(mn, rg) and abs(got[5, 0] - (float(mn) + float(rg))) <= R.tol(mn, rg)
    assert P[0] < P[1] < P[2] < P[3]
    two = K.load_mat("%s:%d" % (ark, offs[2]))
    assert two[0, 0] == mn and abs(two[0, 4] - (float(mn) + float(rg))) <= R.tol(mn, rg)


def test_decode_of_encoded_matrices_matches_oracle(K):
    for name, m, method in encode_cases():
        tok, header, payload = R.encode(m, method)
        mn, rg, rows, cols = struct.unpack("<ffii", header)
        got = K.decompress(tok, mn, rg, rows, cols, payload)
        want = R.decode(tok, mn, rg, rows, cols, payload)
        assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - want).max() <= R.tol(mn, rg), name


# ------------------------------------------------------------------------------------------------------------------ encode
@pytest.mark.parametrize("case", encode_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_compress_mat_bytes_equal_oracle(K, case):
    name, m, method = case
    tok, header, payload = R.encode(m, method)
    got_tok, got_payload = K.compress_mat(m, method)
    assert got_tok == tok == ("CM" if method == "auto" and len(m) > 8 else "CM3" if method == "one-byte" else "CM2")
    assert K.header_bytes(m) == header
    assert len(got_payload) == len(payload) == R.payload_size(tok, *m.shape)
    if got_payload != payload:
        a, b = np.frombuffer(got_payload, np.uint8), np.frombuffer(payload, np.uint8)
        bad = np.flatnonzero(a != b)
        raise AssertionError("%s: %d of %d payload bytes differ, first at %d: %d != %d" % (name, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]]))


def test_constant_matrix_range(K):
    tok, header, payload = R.encode(np.full((20, 5), -3.25, np.float32))
    mn, rg, rows, cols = struct.unpack("<ffii", header)
    assert (mn, rg) == (-3.25, 4.25) and tok == "CM"  # range = 1 + |min|
    words = struct.unpack_from("<4H", payload, 0)
    assert words == (0, 1, 2, 3)  # every statistic quantises to 0; each word is at least one above the one before
    got = K.decompress(tok, mn, rg, rows, cols, K.compress_mat(np.full((20, 5), -3.25, np.float32))[1])
    assert np.abs(got + 3.25).max() <= 4.25 / 65535


def test_zero_minimum_is_written_as_plus_zero(K):
    for name, m, method in encode_cases():
        if "zero" in name:
            for header in (K.header_bytes(m), R.encode(m, method)[1]):
                assert header[:4] == struct.pack("<f", 0.0), name  # not the bytes of -0.0


def test_round_trip_within_half_a_step(K):
    rng = np.random.default_rng(9)
    for rows, cols in ((9, 23), (200, 40), (1500, 80)):
        m = fbank_like(rng, rows, cols)
        tok, payload = K.compress_mat(m)
        mn, rg = struct.unpack("<ff", K.header_bytes(m)[:8])
        back = K.decompress(tok, mn, rg, rows, cols, payload).astype(np.float64)
        t = R.tol(mn, rg)
        checked = 0
        for j in range(cols):
            P0, P25, P75, P100 = R.column_levels(mn, rg, struct.unpack_from("<4H", payload, 8 * j))
            v = m[:, j].astype(np.float64)
            inside = (v >= P0) & (v <= P100)
            half = np.where(v < P25, (P25 - P0) / 128, np.where(v < P75, (P75 - P25) / 256, (P100 - P75) / 126))
            bound = half + t
            err = np.abs(back[:, j] - v)
            assert np.all(err[inside] <= bound[inside]), (rows, cols, j, float((err - bound)[inside].max()))
            checked += int(inside.sum())
        assert checked > 0.9 * m.size


# --------------------------------------------------------------------------------------------------------------- container
def test_write_ark_scp_compressed_offsets_and_mixed_archive(K, tmp_path):
    rng = np.random.default_rng(4)
    mats = [("long_a", fbank_like(rng, 57, 23)), ("short_b", fbank_like(rng, 5, 23)), ("long_c", fbank_like(rng, 300, 23))]
    ark, scp = tmp_path / "c.ark", tmp_path / "c.scp"
    assert K.write_ark_scp(str(ark), str(scp), mats, compress="auto") == 3
    blob = ark.read_bytes()
    want = b"".join(R.entry(k, *R.encode(m)) for k, m in mats)
    assert blob == want
    lines = scp.read_text().splitlines()
    for (k, m), line, tok in zip(mats, lines, ("CM", "CM2", "CM")):
        key, spec = line.split(None, 1)
        off = int(spec.rpartition(":")[2])
        assert key == k and blob[off:off + 2] == b"\0B" and blob[off + 2:off + 3 + len(tok)] == tok.encode() + b" "
        t, header, payload = R.encode(m)
        want_m = R.decode(t, *struct.unpack("<ffii", header), payload)
        got = K.load_mat(spec)
        assert got.shape == m.shape and np.abs(got - want_m).max() <= R.tol(*struct.unpack("<ff", header[:8]))
        assert K.read_raw(spec)[0] == tok
    for method, tok in (("two-byte", "CM2"), ("one-byte", "CM3")):
        K.write_ark_scp(str(tmp_path / "m.ark"), str(tmp_path / "m.scp"), mats, compress=method)
        assert (tmp_path / "m.ark").read_bytes() == b"".join(R.entry(k, *R.encode(m, method)) for k, m in mats)
        assert [K.read_raw(l.split(None, 1)[1])[0] for l in (tmp_path / "m.scp").read_text().splitlines()] == [tok] * 3
    # without compress the bytes are what they were
    K.write_ark_scp(str(tmp_path / "f.ark"), str(tmp_path / "f.scp"), mats)
    assert (tmp_path / "f.ark").read_bytes() == b"".join(
        k.encode() + b" \0BFM \4" + struct.pack("<i", m.shape[0]) + b"\4" + struct.pack("<i", m.shape[1]) + m.tobytes() for k, m in mats)
    # a corpus that mixes CM, CM2 and FM entries: CompressedMatrix items are written as they are
    mixed = [("a", K.CompressedMatrix("CM", K.header_bytes(mats[0][1]), K.compress_mat(mats[0][1])[1])), ("b", mats[1][1]),
             ("c", K.CompressedMatrix("CM2", K.header_bytes(mats[1][1]), K.compress_mat(mats[1][1])[1])), ("d", mats[2][1])]
    K.write_ark_scp(str(tmp_path / "x.ark"), str(tmp_path / "x.scp"), mixed)
    back = dict(K.read_ark(tmp_path / "x.ark"))
    assert [K.read_raw(l.split(None, 1)[1])[0] for l in (tmp_path / "x.scp").read_text().splitlines()] == ["CM", "FM", "CM2", "FM"]
    assert np.array_equal(back["b"], mats[1][1]) and np.array_equal(back["d"], mats[2][1])
    assert np.array_equal(back["a"], mixed[0][1].decode()) and np.array_equal(back["c"], mixed[2][1].decode())
    assert len(mixed[0][1]) == 57 and mixed[0][1].shape == (57, 23)
    raw = K.read_raw((tmp_path / "x.scp").read_text().splitlines()[1].split(None, 1)[1])
    assert raw[1] is None and raw[2] is None and raw[3:5] == (5, 23) and np.array_equal(raw[5], mats[1][1])
    with pytest.raises(ValueError, match="compress"):
        K.write_ark_scp(str(tmp_path / "y.ark"), str(tmp_path / "y.scp"), mats, compress="three-byte")


def test_kaldi_dataset_over_a_compressed_archive(K, tmp_path):
    import datasets as D

    rng = np.random.default_rng(5)
    mats = [("spk%d_u%d" % (j % 3, j), fbank_like(rng, int(n), 12)) for j, n in enumerate((45, 20, 19, 88, 31, 8))]
    cdir, fdir = tmp_path / "c", tmp_path / "f"
    for d in (cdir, fdir):
        d.mkdir()
        K.write_len_scp(d / "len.scp", [(k, len(m)) for k, m in mats])
    K.write_ark_scp(str(cdir / "feats.ark"), str(cdir / "feats.scp"), mats, compress="auto")
    decoded = [(k, m) for k, m in K.read_ark(cdir / "feats.ark")]  # the host-decoded copy, stored uncompressed
    K.write_ark_scp(str(fdir / "feats.ark"), str(fdir / "feats.scp"), decoded)
    cd = D.KaldiDataset(cdir / "feats.scp", cdir / "len.scp", min_len=20, mvn_path=str(cdir / "mvn.json"), seg_len=20, seg_shift=8)
    fd = D.KaldiDataset(fdir / "feats.scp", fdir / "len.scp", min_len=20, mvn_path=str(fdir / "mvn.json"), seg_len=20, seg_shift=8)
    assert len(cd) == len(fd) == 4 and cd.num_segments == fd.num_segments > 10 and cd.seq_keys == fd.seq_keys
    assert (cdir / "mvn.json").read_text() == (fdir / "mvn.json").read_text()
    for i in range(cd.num_segments):
        a, b = cd[i], fd[i]
        assert a[0] == b[0] and a[2] == b[2] and a[1].shape == (20, 12) and np.array_equal(a[1], b[1])
    for i in range(len(cd)):
        assert cd.load_seq(i).dtype == np.float32 and np.array_equal(cd.load_seq(i), fd.load_seq(i))


# ---------------------------------------------------------------------------------------------------------------- refusals
def _cm_entry(tok, mn, rg, rows, cols, payload):
    return b"k1 \0B" + tok.encode() + b" " + struct.pack("<ffii", mn, rg, rows, cols) + payload


@pytest.mark.parametrize("tok", ["CM", "CM2", "CM3"])
def test_refusals_name_path_and_offset(K, tmp_path, tok):
    p = tmp_path / "bad.ark"
    good = bytes(R.payload_size(tok, 9, 2))
    cases = {"zero header": b"k1 \0B" + tok.encode() + b" " + bytes(16) + good,
             "negative range": _cm_entry(tok, 0.0, -1.0, 9, 2, good),
             "nan min": _cm_entry(tok, float("nan"), 1.0, 9, 2, good),
             "inf range": _cm_entry(tok, 0.0, float("inf"), 9, 2, good),
             "no rows": _cm_entry(tok, 0.0, 1.0, 0, 2, b""),
             "negative cols": _cm_entry(tok, 0.0, 1.0, 9, -2, b""),
             "truncated payload": _cm_entry(tok, 0.0, 1.0, 9, 2, good[:-1]),
             "truncated header": b"k1 \0B" + tok.encode() + b" " + bytes(7)}
    for what, blob in cases.items():
        p.write_bytes(blob)
        for read in (lambda: K.load_mat("%s:3" % p), lambda: K.read_raw("%s:3" % p), lambda: list(K.read_ark(p))):
            with pytest.raises(ValueError, match="compressed matrix \\(%s\\)" % tok) as e:
                read()
            assert "bad.ark:3" in str(e.value), (what, str(e.value))
    p.write_bytes(_cm_entry(tok, 0.0, 1.0, 9, 2, good))
    assert K.load_mat("%s:3" % p).shape == (9, 2)


def test_nan_and_inf_on_write_name_the_key(K, tmp_path):
    m = np.zeros((12, 4), np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        m2 = m.copy()
        m2[5, 1] = bad
        with pytest.raises(ValueError, match="utt_bad"):
            K.write_ark_scp(str(tmp_path / "n.ark"), str(tmp_path / "n.scp"), [("utt_ok", m), ("utt_bad", m2)], compress="auto")
        with pytest.raises(ValueError):
            K.compress_mat(m2)
    with pytest.raises(ValueError):
        K.compress_mat(np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError, match="method"):
        K.compress_mat(m, "fixed-range")


# -------------------------------------------------------------------------------------------------------------- the library
def test_symbols_cli_and_argument_errors():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb
    import prepare_kaldi_data as PK
    import train_model

    lib = hb.load_library()
    text = open(os.path.join(ROOT, "include", "fhvae_hip.h")).read()
    for name in ("fhvae_kaldi_decompress", "fhvae_kaldi_compress"):
        assert name + "(" in text and hasattr(lib, name) and name in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12
    assert lib.fhvae_kaldi_decompress(None, 0, None, 0, 0, None, 0, 0, None, None) == -1
    assert lib.fhvae_kaldi_compress(None, 0, 0, None, 0, 0, None, None, 0, None, None) == -1
    assert hb.KALDI_CM_DESC.itemsize == 40 and "FHVAE_KALDI_CM_TILE_ROWS %d" % hb.KALDI_CM_TILE_ROWS in text
    a = PK.build_parser().parse_args(["data"])
    assert a.compress is False and a.compression_method == "auto"
    a = PK.build_parser().parse_args(["data", "--compress", "--compression-method", "one-byte"])
    assert a.compress is True and a.compression_method == "one-byte"
    assert "uncompressed" not in train_model.build_parser().format_help()
