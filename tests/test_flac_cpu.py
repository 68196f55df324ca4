"""FLAC and SPHERE input without a GPU: the scalar oracle of tests/flac_ref.py against the two bitstreams of RFC 9639's
appendix (tests/golden/flac_rfc9639_*.hex) and against its own encoder over the case list the device tests reuse,
flac_lite.parse_flac and its refusals, features.read_sphere / read_audio, and the three preprocess tools on generated trees."""
import os
import sys

import numpy as np
import pytest

import flac_ref as R
from test_feats_cpu import _write_wav

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def F():
    import features

    return features


def golden(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return bytes.fromhex("".join(line.split("#")[0] for line in fh).replace(" ", "").replace("\n", ""))


def signal(rng, n, nch, bps, amp=0.6):
    """Tones plus noise, `amp` of full scale, (n, nch) integers of bps bits; the channels are related but not equal."""
    t = np.arange(n)[:, None]
    x = np.sin(t * (0.05 + 0.013 * np.arange(nch))[None]) * 0.7 + np.sin(t * 0.31) * 0.2 + rng.standard_normal((n, nch)) * 0.05
    top = (1 << (bps - 1)) - 1
    return np.clip(np.round(x * amp * top), -top - 1, top).astype(np.int64)


_CASES = {}


def cases():
    """name -> (file bytes, what it is for); built once.  Every file is small: the oracle reads bit by bit."""
    if _CASES:
        return _CASES
    S, E = R.Sub, R.encode_stream
    rng = np.random.default_rng(9639)
    c = _CASES
    mono = signal(rng, 200, 1, 16)
    c["constant"] = E(np.full((64, 1), -1234), 16, 16000, block=64, subs=S("constant"))
    c["verbatim"] = E(mono, 16, 16000, block=200, subs=S("verbatim"))
    for o in range(5):
        c["fixed%d" % o] = E(mono, 16, 16000, block=100, subs=S("fixed", order=o))
    for order in (1, 8, 32):
        small = rng.integers(-3, 4, size=order).tolist()  # shift 0: the prediction is the plain sum
        big = rng.integers(-(1 << 14), 1 << 14, size=order).tolist()  # shift 14: the sum passes 2^32 before the shift
        c["lpc%d_shift0" % order] = E(mono, 16, 16000, block=100, subs=S("lpc", coefs=small, precision=15, shift=0))
        c["lpc%d_shift14" % order] = E(mono, 16, 16000, block=100, subs=S("lpc", coefs=big, precision=15, shift=14, method=1))
    c["wasted_fixed"] = E(signal(rng, 150, 2, 13) * 8, 16, 16000, block=150, subs=[S("fixed", order=2, wasted=3), S("lpc", coefs=[3, -1], precision=4, shift=1, wasted=3)])
    long_ = signal(rng, 256, 1, 16)
    c["part0"] = E(long_, 16, 16000, block=256, subs=S("fixed", order=2, part_order=0))
    c["part3"] = E(long_, 16, 16000, block=256, subs=S("fixed", order=2, part_order=3))
    c["part_max"] = E(long_, 16, 16000, block=256, subs=S("fixed", order=1, part_order=7))  # partitions of 2 > order 1
    flat = np.concatenate([np.full(32, 77), signal(rng, 32, 1, 16)[:, 0] // 2])[:, None]
    c["escape0"] = E(flat, 16, 16000, block=64, subs=S("fixed", order=1, part_order=1, params=[("esc", 0), None]))
    c["escape17"] = E(flat, 16, 16000, block=64, subs=S("fixed", order=0, part_order=1, params=[None, ("esc", 17)]))
    c["rice5_24bit"] = E(signal(rng, 120, 2, 24, amp=0.9) + rng.integers(-(1 << 20), 1 << 20, size=(120, 2)) // 4, 24, 48000, block=120,
                         subs=S("fixed", order=0, method=1, params=[20]))
    c["rice_k0"] = E(rng.integers(-2, 3, size=(90, 1)), 16, 16000, block=90, subs=S("fixed", order=0, params=[0]))
    spike = np.zeros((40, 1), np.int64)
    spike[20] = 23  # folded 46: a run of 46 zeros under parameter 0
    spike[30] = -50  # folded 99
    c["long_quotient"] = E(spike, 16, 16000, block=40, subs=S("fixed", order=0, params=[0]))
    st = signal(rng, 130, 2, 16)
    st[:, 1] = st[:, 0] + rng.integers(-40, 41, size=130)  # left + right odd for about half the samples
    for mode in ("indep", "left_side", "side_right", "mid_side"):
        c["stereo_" + mode] = E(st, 16, 44100, block=65, stereo=mode, subs=S("fixed", order=2))
    full = np.array([[32767, -32768], [-32768, 32767], [32767, 32766], [-32768, -32767], [1, 0], [0, 1], [-1, 0], [0, -1]])
    c["stereo_mid_side_extremes"] = E(full, 16, 44100, block=8, stereo="mid_side", subs=S("verbatim"))
    for bps in (8, 12, 16, 20, 24):
        c["bps%d" % bps] = E(signal(rng, 100, 2, bps, amp=0.95), bps, 32000, block=50, stereo="mid_side" if bps != 16 else "indep", subs=S("fixed", order=2))
    c["bps4_size_code0"] = E(signal(rng, 40, 1, 4, amp=1.0), 4, 8000, block=40)
    for nch in (1, 2, 8):
        c["ch%d" % nch] = E(signal(rng, 70, nch, 16), 16, 22050, block=35, subs=lambda fi, ch: S("fixed", order=ch % 5))
    for bs in (192, 576, 1152, 256, 512):
        c["block%d" % bs] = E(signal(rng, bs + 17, 1, 16), 16, 16000, block=bs)  # (and a short last frame)
    c["block_8bit_field"] = E(signal(rng, 3 * 192, 1, 16), 16, 16000, block=192, block_code="8bit")
    c["block_16bit_field"] = E(signal(rng, 2 * 300 + 11, 1, 16), 16, 16000, block=300, block_code="16bit")
    c["variable_blocks"] = E(signal(rng, 16 + 192 + 40 + 256 + 1, 2, 16), 16, 16000, blocks=[16, 192, 40, 256, 1], strategy=1)
    c["variable_big_sample_number"] = E(signal(rng, 3 * 4608, 1, 8), 8, 8000, blocks=[4608] * 3, strategy=1, subs=S("fixed", order=1))
    c["frames_130"] = E(signal(rng, 130 * 16 + 5, 1, 16), 16, 16000, block=16)  # frame numbers 128.. take two bytes
    for rc, rate in ((12, 11000), (13, 11025), (14, 37800), (0, 12345)):
        c["rate_code%d" % rc] = E(signal(rng, 60, 1, 16), 16, rate, block=60, rate_code=rc)
    c["metadata_blocks"] = E(mono, 16, 16000, block=200, extra_blocks=[(4, b"\x00" * 40), (1, b"\xff\xf8" * 30)])
    c["no_md5_unknown_total"] = R.stream_file(R.encode_frame([mono[:, 0].tolist()], 0, 16, 16000, [S("fixed", order=2)]), 16000, 1, 16, 0, 200, 200)
    c["false_start"] = false_start(rng)
    c["fixture_A"] = golden("flac_rfc9639_file_a.hex")
    c["fixture_B"] = R.stream_file(golden("flac_rfc9639_frame_b.hex"), 44100, 2, 16, 16, 16, 16)
    return c


def false_start(rng):
    """A verbatim frame whose sample bytes hold a whole valid frame (header with its CRC-8, a subframe, its CRC-16) of the same
    stream, byte aligned: a decoder that trusts a sync code, or even a frame that parses, goes wrong here."""
    inner = R.encode_frame([signal(rng, 16, 1, 16)[:, 0].tolist()], 1, 16, 16000, [R.Sub("fixed", order=1)])
    inner += b"\x00" * (len(inner) % 2)
    hidden = np.frombuffer(inner, dtype=">i2").astype(np.int64)
    x = np.concatenate([signal(rng, 21, 1, 16)[:, 0], hidden, signal(rng, 30, 1, 16)[:, 0]])
    n = len(x)
    tail = signal(rng, 2 * n, 1, 16)[:, 0]
    return R.encode_stream(np.concatenate([x, tail])[:, None], 16, 16000, block=n, subs=lambda fi, ch: R.Sub("verbatim" if fi == 0 else "fixed", order=2))


# ----------------------------------------------------------------------------------------------------------------- oracle
def test_oracle_reproduces_the_rfc_examples():
    assert golden("flac_rfc9639_file_a.hex") == R.FIXTURE_A and golden("flac_rfc9639_frame_b.hex") == R.FIXTURE_B
    x, rate, bps, md5 = R.decode(R.FIXTURE_A)
    assert (rate, bps) == (44100, 16) and x.tolist() == [[25588, 10416]]
    assert md5.hex() == "3e84b41807dc690307586a3dad1a2e0f" == R.pcm_md5(x, 16).hex()
    assert R.crc8(R.FIXTURE_A[42:48]) == 0xBF and R.crc16(R.FIXTURE_A[42:55]) == 0xAA9A
    y = R.decode(cases()["fixture_B"])[0]
    assert y[:, 0].tolist() == R.B_LEFT and y[:, 1].tolist() == R.B_RIGHT
    assert R.crc8(R.FIXTURE_B[:6]) == 0x99 and R.crc16(R.FIXTURE_B[:-2]) == 0xB810


def test_encoder_to_oracle_round_trip():
    """Every case decodes to the PCM its STREAMINFO MD5 was computed from (the encoder hashes its input), frame CRCs verified."""
    for name, blob in cases().items():
        x, rate, bps, md5 = R.decode(blob)
        if md5 != bytes(16):
            assert R.pcm_md5(x, bps) == md5, name
    # and the encoder emits what it is told to: spot checks on the bits
    c = cases()
    assert c["block_8bit_field"][42 + 2] >> 4 == 6 and c["block_16bit_field"][42 + 2] >> 4 == 7 and c["block192"][42 + 2] >> 4 == 1
    assert c["variable_blocks"][42 + 1] == 0xF9 and c["stereo_mid_side"][42 + 3] >> 4 == 10
    assert c["rate_code13"][42 + 2] & 15 == 13 and c["bps4_size_code0"][42 + 3] & 0x0E == 0
    with pytest.raises(R.FlacError):
        bad = bytearray(c["fixed2"])
        bad[60] ^= 0x10
        R.decode(bytes(bad))


# -------------------------------------------------------------------------------------------------------------- container
def test_parse_flac_fields():
    import flac_lite

    info = flac_lite.parse_flac(R.FIXTURE_A, "A")
    assert info == (44100, 2, 16, 1, 4096, 4096, bytes.fromhex("3e84b41807dc690307586a3dad1a2e0f"), 42)
    assert info.sample_rate == 44100 and info.first_frame == 42 and info.total_samples == 1
    m = flac_lite.parse_flac(cases()["metadata_blocks"], "m")
    assert m.first_frame == 42 + 4 + 40 + 4 + 60 and m.channels == 1
    big = flac_lite.parse_flac(R.stream_file(b"", 655350, 8, 24, (1 << 36) - 1, 16, 65535), "big")
    assert big[:6] == (655350, 8, 24, (1 << 36) - 1, 16, 65535)


def test_parse_flac_refusals():
    import flac_lite

    a = R.FIXTURE_A

    def refuse(buf, reason):
        with pytest.raises(ValueError, match=reason) as e:
            flac_lite.parse_flac(buf, "some/file.flac")
        assert "some/file.flac" in str(e.value)

    refuse(b"ID3\x04\x00\x00\x00\x00\x00\x0a" + bytes(10) + a, "ID3v2")
    refuse(b"OggS\x00\x02" + bytes(40) + a, "Ogg")
    refuse(b"RIFF" + bytes(40), "not a FLAC file")
    refuse(R.stream_file(b"", 44100, 2, 25, 0, 16, 16), "25 bits per sample")
    refuse(R.stream_file(b"", 44100, 2, 32, 0, 16, 16), "32 bits per sample")
    refuse(R.stream_file(b"", 44100, 2, 3, 0, 16, 16), "3 bits per sample")
    refuse(b"fLaC" + bytes([0x84]) + (8).to_bytes(3, "big") + bytes(8) + a[42:], "no STREAMINFO")
    refuse(a[:30], "truncated")
    refuse(a[:5], "truncated")
    refuse(b"fLaC" + a[4:42].replace(b"\x80\x00\x00\x22", b"\x00\x00\x00\x22"), "truncated")  # "not last", and nothing follows


# ----------------------------------------------------------------------------------------------------------------- SPHERE
def sphere(data, sr, fmt="01", coding=None, width=2, extra=""):
    n, nch = data.shape
    head = "NIST_1A\n   1024\n"
    head += "database_id -s5 TIMIT\nsample_count -i %d\nsample_n_bytes -i %d\nchannel_count -i %d\n" % (n, width, nch)
    head += "sample_byte_format -s%d %s\nsample_rate -i %d\nsample_sig_bits -i %d\n" % (len(fmt), fmt, sr, 8 * width)
    if coding:
        head += "sample_coding -s%d %s\n" % (len(coding), coding)
    head += extra + "end_head\n"
    dt = "i1" if width == 1 else ("<i2" if fmt == "01" else ">i2")
    return head.encode().ljust(1024, b" ") + data.astype(dt).tobytes()


def test_read_sphere(F, tmp_path):
    rng = np.random.default_rng(3)
    data = rng.integers(-32768, 32768, size=(500, 1))
    data[:2, 0] = (-32768, 32767)
    for fmt in ("01", "10"):
        p = tmp_path / ("SA1_%s.WAV" % fmt)
        p.write_bytes(sphere(data, 16000, fmt, coding="pcm" if fmt == "10" else None))
        y, sr = F.read_sphere(p)
        assert sr == 16000 and y.dtype == np.float32 and np.array_equal(y, (data[:, 0] / 32768.0).astype(np.float32))
    two = rng.integers(-32768, 32768, size=(300, 2))
    p = tmp_path / "two.sph"
    p.write_bytes(sphere(two, 8000, "10"))
    x = two.astype(np.float32) / 32768.0
    assert np.array_equal(F.read_sphere(p)[0], x.mean(axis=1, dtype=np.float32))
    assert np.array_equal(F.read_sphere(p, channel=1)[0], x[:, 1])
    with pytest.raises(ValueError, match="no channel 2"):
        F.read_sphere(p, channel=2)
    # the same samples in a WAV file: the same waveform bit for bit
    _write_wav(tmp_path / "two.wav", two, 8000, 2)
    assert np.array_equal(F.read_wav(tmp_path / "two.wav")[0], F.read_sphere(p)[0])
    one = rng.integers(-128, 128, size=(50, 1))
    p1 = tmp_path / "one.sph"
    p1.write_bytes(sphere(one, 8000, "1", width=1))
    assert np.array_equal(F.read_sphere(p1)[0], (one[:, 0] / 128.0).astype(np.float32))
    for coding in ("pcm,embedded-shorten-v2.00", "ulaw", "alaw", "pcm,embedded-wavpack-v1.0"):
        q = tmp_path / "coded.sph"
        q.write_bytes(sphere(data, 16000, "01", coding=coding, width=1 if "law" in coding else 2))
        with pytest.raises(ValueError, match=coding.split(",")[-1].split("-v")[0]) as e:
            F.read_sphere(q)
        assert "coded.sph" in str(e.value)
    q = tmp_path / "cut.sph"
    q.write_bytes(sphere(data, 16000)[:-10])
    with pytest.raises(ValueError, match="truncated"):
        F.read_sphere(q)
    q.write_bytes(sphere(data, 16000, "0123"))
    with pytest.raises(ValueError, match="sample_byte_format"):
        F.read_sphere(q)


def test_read_audio_dispatch(F, tmp_path):
    rng = np.random.default_rng(4)
    data = rng.integers(-32768, 32768, size=(400, 2))
    _write_wav(tmp_path / "a.bin", data, 16000, 2)  # the name says nothing: the first bytes decide
    (tmp_path / "b.bin").write_bytes(sphere(data, 16000, "10"))
    ya, yb = F.read_audio(tmp_path / "a.bin"), F.read_audio(tmp_path / "b.bin", channel=0)
    assert ya[1] == yb[1] == 16000 and np.array_equal(ya[0], F.read_wav(tmp_path / "a.bin")[0])
    assert np.array_equal(yb[0], (data[:, 0] / 32768.0).astype(np.float32))
    both = F.read_audio_batch([tmp_path / "b.bin", tmp_path / "a.bin"], channel=1)
    assert np.array_equal(both[0][0], both[1][0])
    (tmp_path / "c.mp3").write_bytes(b"\xff\xfb\x90\x00" + bytes(100))
    with pytest.raises(ValueError, match="c.mp3") as e:
        F.read_audio(tmp_path / "c.mp3")
    assert all(k in str(e.value) for k in ("RIFF", "fLaC", "NIST_1A"))
    (tmp_path / "d.flac").write_bytes(b"ID3\x03" + bytes(60))
    with pytest.raises(ValueError, match="ID3v2"):
        F.read_audio(tmp_path / "d.flac")
    # pcm_to_float is read_wav's arithmetic
    for width in (1, 2, 3):
        bits = 8 * width
        d = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(200, 2))
        _write_wav(tmp_path / "w.wav", d + 128 if width == 1 else d, 8000, width)
        assert np.array_equal(F.pcm_to_float(d, bits), F.read_wav(tmp_path / "w.wav")[0])


# ------------------------------------------------------------------------------------------------------------------ tools
def test_preprocess_librispeech(tmp_path, capsys):
    import preprocess_librispeech as PL

    raw = tmp_path / "LibriSpeech"
    files = {"train-clean-100": ["103/1240/103-1240-0001", "103/1240/103-1240-0000", "26/495/26-495-0003"], "dev-clean": ["84/121123/84-121123-0001"],
             "dev-other": ["116/288045/116-288045-0000"], "test-clean": ["61/70968/61-70968-0002"], "test-other": ["367/130732/367-130732-0000"],
             "train-clean-360": ["100/121669/100-121669-0000"]}
    for subset, names in files.items():
        for n in names:
            (raw / subset / n).parent.mkdir(parents=True, exist_ok=True)
            (raw / subset / (n + ".flac")).write_bytes(b"fLaC")
            (raw / subset / (n + ".trans.txt")).write_text("x")
    assert PL.main([str(raw), str(tmp_path / "out"), "--data-format", "kaldi"]) == 0

    def scp(name):
        return [line.split(" ", 1) for line in (tmp_path / "out" / name / "wav.scp").read_text().splitlines()]

    train = scp("train")
    assert [u for u, _ in train] == ["103-1240-0000", "103-1240-0001", "26-495-0003"]
    assert all(p == str(raw / "train-clean-100" / u.split("-")[0] / u.split("-")[1] / (u + ".flac")) for u, p in train)  # the .flac itself
    assert [u for u, _ in scp("dev")] == ["116-288045-0000", "84-121123-0001"]
    assert [u for u, _ in scp("test")] == ["367-130732-0000", "61-70968-0002"]
    assert PL.process_librispeech(raw, tmp_path / "o2", train_list=["train-clean-360", "train-clean-100", "nothing"])[0] == tmp_path / "o2" / "train" / "wav.scp"
    lines = (tmp_path / "o2" / "train" / "wav.scp").read_text().splitlines()
    assert [ln.split()[0] for ln in lines] == ["100-121669-0000", "103-1240-0000", "103-1240-0001", "26-495-0003"]
    assert [ln.split()[0] for ln in (tmp_path / "o2" / "test" / "wav.scp").read_text().splitlines()] == ["367-130732-0000", "61-70968-0002"]


def timit_tree(raw):
    data = np.arange(-200, 200)[:, None] * 50
    for part, dr, spk, utts in (("TRAIN", "DR1", "FCJF0", ["SA1", "SI1027"]), ("TRAIN", "DR2", "MDAB0", ["SX139"]), ("TEST", "DR1", "FAKS0", ["SA2", "SA1"]),
                                ("TEST", "DR3", "MJMP0", ["SX95"]), ("TEST", "DR4", "FELC0", ["SI756"])):
        d = raw / part / dr / spk
        d.mkdir(parents=True)
        for u in utts:
            (d / (u + ".WAV")).write_bytes(sphere(data, 16000))
            (d / (u + ".PHN")).write_text("0 1 h#\n")
    return data


def test_preprocess_timit(F, tmp_path):
    import preprocess_timit as PT

    raw = tmp_path / "timit"
    data = timit_tree(raw)
    (tmp_path / "dev.list").write_text("FAKS0\nmjmp0\n")
    (tmp_path / "test.list").write_text("felc0\n")
    assert PT.main([str(raw), str(tmp_path / "out"), "--dev_spk", str(tmp_path / "dev.list"), "--test_spk", str(tmp_path / "test.list")]) == 0

    def scp(name):
        return [line.split(" ", 1) for line in (tmp_path / "out" / name / "wav.scp").read_text().splitlines()]

    assert [u for u, _ in scp("train")] == ["fcjf0_SA1", "fcjf0_SI1027", "mdab0_SX139"]
    assert [u for u, _ in scp("dev")] == ["faks0_SA1", "faks0_SA2", "mjmp0_SX95"]
    assert scp("test") == [["felc0_SI756", str(raw / "TEST" / "DR4" / "FELC0" / "SI756.WAV")]]
    assert not (tmp_path / "out" / "wav").exists()  # nothing converted: the SPHERE files are listed in place, and readable
    y, sr = F.read_audio(scp("dev")[0][1])
    assert sr == 16000 and np.array_equal(y, (data[:, 0] / 32768.0).astype(np.float32))
    with pytest.raises(SystemExit):
        PT.main([str(raw), str(tmp_path / "out")])  # the speaker lists are required
    (tmp_path / "test.list").write_text("felc0\nfaks0\n")
    with pytest.raises(ValueError, match="faks0"):
        PT.process_timit(raw, tmp_path / "out", tmp_path / "dev.list", tmp_path / "test.list")


def test_preprocess_data_command_line(tmp_path, monkeypatch):
    """The reference's command line, the directory name, what reaches the prepare functions and the paths_dict that comes back
    (the prepare functions themselves need the GPU: tests/test_flac_gpu.py runs them on FLAC)."""
    import prepare_kaldi_data
    import prepare_numpy_data
    import preprocess_data as PD

    assert str(PD.output_dir_name("timit", "numpy", "spec")) == "timit_np_spec" and str(PD.output_dir_name("librispeech", "kaldi", "spec")) == "librispeech_kd_fbank"
    a = PD.build_parser().parse_args(["timit", "raw"])
    assert (a.data_format, a.feat_type, a.hop_size, a.win_size, a.mels, a.sample_rate, a.fbank_conf) == ("numpy", "fbank", 0.010, 0.025, 80, None, "./misc/fbank.conf")
    with pytest.raises(SystemExit):
        PD.build_parser().parse_args(["timit", "raw", "--kaldi-root", "k"])
    raw = tmp_path / "timit"
    timit_tree(raw)
    (tmp_path / "dev.list").write_text("faks0\n")
    (tmp_path / "test.list").write_text("felc0\n")
    monkeypatch.chdir(tmp_path)
    seen = []

    def fake_numpy(dataset, set_name, dataset_dir, output_dir=None, ftype="fbank", sample_rate=None, win_t=0.025, hop_t=0.010, n_mels=80, **kw):
        seen.append((dataset, set_name, str(dataset_dir), ftype, sample_rate, n_mels, kw))
        return 2, ("w_" + set_name, "f_" + set_name, "l_" + set_name)

    def fake_kaldi(dataset_dir, set_name, fbank_conf, **kw):
        seen.append((str(dataset_dir), set_name, fbank_conf, kw))
        return 1, ("d", "a_" + set_name, "f_" + set_name, "l_" + set_name)

    monkeypatch.setattr(prepare_numpy_data, "prepare_numpy", fake_numpy)
    monkeypatch.setattr(prepare_kaldi_data, "prepare_kaldi", fake_kaldi)
    assert PD.main(["timit", str(raw)]) == 1  # no speaker lists
    args = PD.build_parser().parse_args(["timit", str(raw), "--dev-spk", "dev.list", "--test-spk", "test.list", "--feat-type", "spec", "--sample-rate", "8000", "--mels", "40"])
    paths = PD.preprocess_data(args)
    assert paths == {s: {"wav_pth": "w_" + s, "feat_pth": "f_" + s, "len_pth": "l_" + s} for s in ("train", "dev", "test")}
    assert [s[1] for s in seen] == ["train", "dev", "test"] and seen[0][:6] == ("timit", "train", "timit_np_spec", "spec", 8000, 40)
    assert seen[0][6] == {"resample": True, "verify_md5": False}
    assert len((tmp_path / "timit_np_spec" / "dev" / "wav.scp").read_text().splitlines()) == 2
    del seen[:]
    lib = tmp_path / "Libri"
    (lib / "dev-clean" / "1" / "2").mkdir(parents=True)
    (lib / "dev-clean" / "1" / "2" / "1-2-0000.flac").write_bytes(b"fLaC")
    args = PD.build_parser().parse_args(["librispeech", str(lib), "--data-format", "kaldi", "--fbank-conf", os.path.join(GOLDEN, "kaldi_fbank.conf"), "--verify-md5"])
    paths = PD.preprocess_data(args)
    assert paths["dev"] == {"wav_pth": "d", "feat_ark": "a_dev", "feat_pth": "f_dev", "len_pth": "l_dev"}
    assert seen[1][0] == "librispeech_kd_fbank" and seen[1][3] == {"resample": False, "verify_md5": True}
    assert (tmp_path / "librispeech_kd_fbank" / "dev" / "wav.scp").read_text() == "1-2-0000 %s\n" % (lib / "dev-clean" / "1" / "2" / "1-2-0000.flac")
