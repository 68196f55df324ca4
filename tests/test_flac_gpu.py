"""FLAC decoding on a MI355X (csrc/flac.hip through features.decode_flac) against the scalar oracle of tests/flac_ref.py, as
integers and exactly: the two RFC 9639 bitstreams, the case list of tests/test_flac_cpu.py (every subframe type, predictor
order, Rice form, stereo mode, sample size, channel count and block-size code), batches, a false frame start inside audio
data, broken files, and prepare_numpy_data.py / prepare_kaldi_data.py on a corpus stored as FLAC against the same as WAV."""
import os

import numpy as np
import pytest
import torch

import flac_ref as R
from test_feats_cpu import _write_wav
from test_flac_cpu import cases, signal

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


@pytest.fixture(scope="module")
def F():
    import features

    return features


@pytest.fixture(scope="module")
def oracle():
    """name -> (samples int64 (n, channels), rate, bps) by the scalar decoder, computed once."""
    return {name: R.decode(blob)[:3] for name, blob in cases().items()}


def same(got, want):
    return got[0].dtype == np.int32 and got[0].shape == want[0].shape and np.array_equal(got[0], want[0]) and got[1:] == want[1:]


def test_every_case_alone(hb, F, oracle):
    bad = []
    for name, blob in cases().items():
        got = F.decode_flac([blob], [name], verify_md5=True)[0]
        if not same(got, oracle[name]):
            bad.append(name)
    assert not bad, bad
    a = F.decode_flac([cases()["fixture_A"]])[0]
    assert a[0].tolist() == [[25588, 10416]] and a[1:] == (44100, 16)
    b = F.decode_flac([cases()["fixture_B"]])[0]
    assert b[0][:, 0].tolist() == R.B_LEFT and b[0][:, 1].tolist() == R.B_RIGHT


def test_batches(hb, F, oracle):
    """Five files of different rates, lengths and channel counts in one call; every case in one call; and the same cut into
    many small batches."""
    five = ["ch1", "ch8", "rice5_24bit", "frames_130", "fixture_A"]
    got = F.decode_flac([cases()[n] for n in five], five, verify_md5=True)
    assert {(g[1], g[0].shape[1], g[0].shape[0]) for g in got} == {(22050, 1, 70), (22050, 8, 70), (48000, 2, 120), (16000, 1, 2085), (44100, 2, 1)}
    assert all(same(g, oracle[n]) for g, n in zip(got, five))
    names = list(cases())
    blobs = [cases()[n] for n in names]
    for kw in ({}, {"max_samples": 700}):
        got = F.decode_flac(blobs, names, verify_md5=True, **kw)
        assert [n for g, n in zip(got, names) if not same(g, oracle[n])] == []
    assert F.decode_flac([]) == []
    empty = R.stream_file(b"", 16000, 2, 16, 0, 4096, 4096)
    got = F.decode_flac([empty, cases()["ch2"], empty])
    assert got[0][0].shape == (0, 2) and got[2][0].shape == (0, 2) and same(got[1], oracle["ch2"])


def test_false_start_is_off_the_chain(hb, F, oracle):
    """The hidden frame is a candidate and parses with a good CRC-16, and the decode still follows the chain."""
    import flac_lite

    blob = cases()["false_start"]
    first = flac_lite.parse_flac(blob).first_frame
    buf = torch.from_numpy(np.frombuffer(blob, np.uint8)[first:].copy()).cuda()
    desc = np.zeros(1, hb.FLAC_DESC)
    desc["byte_end"], desc["rate"], desc["channels"], desc["bps"], desc["min_block"] = buf.numel(), 16000, 1, 16, 1
    desc_d = torch.from_numpy(desc.view(np.uint8)).cuda()
    info = torch.empty(buf.numel(), dtype=torch.int32, device="cuda")
    hb.flac_scan(buf, desc_d, info)
    cand = torch.nonzero(info).flatten()
    n = cand.numel()
    assert n == 4  # three frames and the hidden one
    st, end, spos = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
    hb.flac_decode(buf, desc_d, cand, st, end, spos)
    pos, st, end, spos = cand.cpu().tolist(), st.cpu().tolist(), end.cpu().tolist(), spos.cpu().tolist()
    words = info[cand].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert st == [0, 0, 0, 0] and pos[0] == 0 and end[0] == pos[2] and end[2] == pos[3] and end[3] == buf.numel()
    assert pos[0] < pos[1] and end[1] < pos[2] and spos[1] == 1  # the hidden frame lies inside the first and calls itself frame 1
    assert ((words[1] >> 8) & 0x1FFFF) == 16 and (words[1] & 0xFF) == 7 and words[1] >> 31 == 1
    assert same(F.decode_flac([blob], verify_md5=True)[0], oracle["false_start"])


def test_broken_files_are_refused_and_leave_nothing_behind(hb, F, oracle):
    import flac_lite

    name = "stereo_mid_side"
    blob = cases()[name]
    first = flac_lite.parse_flac(blob).first_frame

    def still_exact():
        assert same(F.decode_flac([blob], verify_md5=True)[0], oracle[name])

    # every byte of a frame is under its CRC-16 (or is it): one flipped bit anywhere in the frames is an error
    for at in range(first, len(blob), 5):
        bad = bytearray(blob)
        bad[at] ^= 1 << (at % 8)
        with pytest.raises(ValueError, match="corpus/broken.flac.*byte offset"):
            F.decode_flac([cases()["ch1"], bytes(bad)], ["corpus/fine.flac", "corpus/broken.flac"])
    still_exact()
    for cut in (1, 2, 3, 40, len(blob) - first - 7):
        with pytest.raises(ValueError, match="cut.flac.*byte offset"):
            F.decode_flac([blob[:len(blob) - cut]], ["cut.flac"])
    still_exact()
    with pytest.raises(ValueError, match="cut.flac.*STREAMINFO announces"):  # cut between two frames: no frame is broken
        F.decode_flac([blob[:first + _first_frame_len(hb, blob, first)]], ["cut.flac"])
    wrong = bytearray(blob)
    wrong[26 + 5] ^= 0x40  # a byte of STREAMINFO's MD5
    assert same(F.decode_flac([bytes(wrong)])[0], oracle[name])  # (not asked for: not checked)
    with pytest.raises(ValueError, match="sums.flac.*MD5"):
        F.decode_flac([bytes(wrong)], ["sums.flac"], verify_md5=True)
    still_exact()
    swapped = cases()["frames_130"]
    f130 = flac_lite.parse_flac(swapped).first_frame
    fl = _first_frame_len(hb, swapped, f130)
    with pytest.raises(ValueError, match="order.flac.*starts at sample 16, the frames before it end at 0"):
        F.decode_flac([swapped[:f130] + swapped[f130 + fl:]], ["order.flac"])  # the first frame is missing
    still_exact()


def _first_frame_len(hb, blob, first):
    x = np.frombuffer(blob, np.uint8)[first:].copy()
    info = __import__("flac_lite").parse_flac(blob)
    desc = np.zeros(1, hb.FLAC_DESC)
    desc["byte_end"], desc["rate"], desc["channels"], desc["bps"], desc["min_block"] = len(x), info.sample_rate, info.channels, info.bps, info.min_block
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    st, end, spos = torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty_like(z), torch.empty_like(z)
    hb.flac_decode(torch.from_numpy(x).cuda(), torch.from_numpy(desc.view(np.uint8)).cuda(), z, st, end, spos)
    assert int(st.item()) == 0
    return int(end.item())


def test_decode_stays_inside_its_output_range(hb, F):
    """A frame whose samples do not fit the range its descriptor gives it is refused with a status and writes nothing."""
    import flac_lite

    blob = cases()["ch2"]  # two frames of 35 samples, 2 channels
    first = flac_lite.parse_flac(blob).first_frame
    x = np.frombuffer(blob, np.uint8)[first:].copy()
    buf = torch.from_numpy(x).cuda()
    fl = _first_frame_len(hb, blob, first)
    cand = torch.tensor([0, fl], dtype=torch.int64, device="cuda")
    st, end, spos = torch.empty(2, dtype=torch.int32, device="cuda"), torch.empty_like(cand), torch.empty_like(cand)
    for n_samples, out_off, n_out, want in ((70, 0, 140, [0, 0]), (69, 0, 140, [0, 9]), (34, 0, 140, [9, 9]), (70, 2, 140, [9, 9]), (70, 0, 139, [9, 9])):
        desc = np.zeros(1, hb.FLAC_DESC)
        desc["byte_end"], desc["rate"], desc["channels"], desc["bps"], desc["min_block"] = len(x), 22050, 2, 16, 35
        desc["n_samples"], desc["out_off"] = n_samples, out_off
        out = torch.full((160,), 12345, dtype=torch.int32, device="cuda")
        hb.flac_decode(buf, torch.from_numpy(desc.view(np.uint8)).cuda(), cand, st, end, spos, out[:n_out])
        assert st.cpu().tolist() == want, (n_samples, out_off, n_out)
        o = out.cpu().numpy()
        written = np.flatnonzero(o != 12345).size  # (a sample may be 12345 itself)
        expect = 70 * want.count(0)
        assert expect - 2 <= written <= expect and np.all(o[140:] == 12345)
    t = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hb.flac_scan(t, t, torch.zeros(4, dtype=torch.int32))


def test_flac_and_wav_of_the_same_samples_read_the_same(hb, F, tmp_path):
    rng = np.random.default_rng(8)
    for bps, width in ((16, 2), (24, 3), (8, 1)):
        pcm = signal(rng, 3000, 2, bps, amp=0.9)
        (tmp_path / "x.flac").write_bytes(R.encode_stream(pcm, bps, 16000, block=1152, stereo="mid_side"))
        _write_wav(tmp_path / "x.wav", pcm + 128 if width == 1 else pcm, 16000, width)
        for ch in (None, 0, 1):
            a, b = F.read_audio(tmp_path / "x.flac", channel=ch), F.read_wav(tmp_path / "x.wav", channel=ch)
            assert a[1] == b[1] == 16000 and a[0].dtype == np.float32 and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    both = F.read_audio_batch([tmp_path / "x.wav", tmp_path / "x.flac"], verify_md5=True)
    assert np.array_equal(both[0][0], both[1][0])


def _corpus(tmp_path, rng):
    """Three utterances, each as FLAC under flac/train and as WAV under wav/train, with a wav.scp each."""
    sr = 16000
    for kind in ("flac", "wav"):
        (tmp_path / kind / "train").mkdir(parents=True)
    lines = {"flac": [], "wav": []}
    for j, n in enumerate((9000, 16000, 12345)):
        pcm = signal(rng, n, 1 if j != 1 else 2, 16, amp=0.5)
        key = "spk%d_u%d" % (j % 2, j)
        block = 4096 if j else 1152
        blob = R.encode_stream(pcm, 16, sr, block=block, stereo="indep" if j != 1 else "left_side",  # (the short last frame: one partition)
                               subs=lambda fi, ch: R.Sub("lpc", coefs=[1800, -900, 80], precision=12, shift=10, part_order=2 if fi < n // block else 0))
        (tmp_path / "flac" / "train" / (key + ".flac")).write_bytes(blob)
        _write_wav(tmp_path / "wav" / "train" / (key + ".wav"), pcm, sr, 2)
        for kind in lines:
            lines[kind].append("%s %s\n" % (key, tmp_path / kind / "train" / (key + "." + kind)))
    for kind in lines:
        (tmp_path / kind / "train" / "wav.scp").write_text("".join(lines[kind]))
    return [ln.split()[0] for ln in lines["wav"]]


def test_prepare_numpy_data_on_flac_equals_wav(hb, tmp_path, capsys):
    import prepare_numpy_data as PN

    keys = _corpus(tmp_path, np.random.default_rng(21))
    for kind in ("flac", "wav"):
        assert PN.main([str(tmp_path / kind), "--set_name", "train"] + (["--verify-md5"] if kind == "flac" else [])) == 0
    capsys.readouterr()
    assert (tmp_path / "flac" / "train" / "len.scp").read_text() == (tmp_path / "wav" / "train" / "len.scp").read_text()
    for k in keys:
        a, b = np.load(tmp_path / "flac" / "train" / (k + ".npy")), np.load(tmp_path / "wav" / "train" / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == b.shape and a.shape[1] == 80 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), k


def test_prepare_kaldi_data_on_flac_equals_wav(hb, tmp_path, capsys):
    import kaldi_io_lite as K
    import prepare_kaldi_data as PK

    keys = _corpus(tmp_path, np.random.default_rng(22))
    conf = tmp_path / "fbank.conf"
    conf.write_text(open(CONF).read().replace("--dither=1", "--dither=0"))
    assert "--dither=0" in conf.read_text()
    for kind in ("flac", "wav"):
        assert PK.main([str(tmp_path / kind), "--fbank_conf", str(conf), "--set_name", "train"]) == 0
    capsys.readouterr()
    assert (tmp_path / "flac" / "train" / "len.scp").read_text() == (tmp_path / "wav" / "train" / "len.scp").read_text()
    fa, fb = (tmp_path / "flac" / "train" / "feats.scp").read_text().splitlines(), (tmp_path / "wav" / "train" / "feats.scp").read_text().splitlines()
    assert [ln.split()[0] for ln in fa] == [ln.split()[0] for ln in fb] == keys
    for a, b in zip(fa, fb):
        ma, mb = K.load_mat(a.split(None, 1)[1]), K.load_mat(b.split(None, 1)[1])
        assert ma.shape == mb.shape and ma.shape[1] == 80 and np.array_equal(ma.view(np.uint32), mb.view(np.uint32))
