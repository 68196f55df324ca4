"""Energy VAD on a MI355X (csrc/vad.hip, include/fhvae_vad.h) against the float64 oracle of tests/vad_ref.py.

Energies: |got - want| <= 2^-23 |want| (one float32 rounding of a float64 value, doubled: the kernel's float64 sum is in another
order than numpy's, 1e-16 relative).  Decisions, ranks, selections, batch invariance: equality, no frame excluded; every
decision test first asserts on the oracle's side that no frame is closer to its threshold than 1e-6 relative (RMS) or 1e-5
absolute (log energy), about ten float32 roundings of a stored energy."""
import os

import numpy as np
import pytest
import torch

import vad_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "tests", "golden", "kaldi_fbank.conf")
RMS_MARGIN, LOGE_MARGIN = 1e-6, 1e-5
N, S = 400, 160  # Kaldi's 25 ms / 10 ms at 16 kHz
KALDI_DEFAULT = (5.0, 0.5, 0, 0.6)
KALDI_RECIPE = (5.5, 0.5, 2, 0.12)


@pytest.fixture(scope="module")
def V():
    import build_ext

    build_ext.build(verbose=False)
    import vad

    vad.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return vad


@pytest.fixture(scope="module")
def F(V):
    import features

    return features


def ptr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_energy(V, waves, L, hop, mode, flags=0):
    """waves: float32 arrays on the scale the mode wants -> (list of float32 energies, status)."""
    lens = np.array([len(w) for w in waves])
    frames = [R.rms_frames(n, L, hop) if mode == V.VAD_RMS_CENTER else R.snip_frames(n, L, hop) for n in lens]
    fp = ptr(frames)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    e = V.energy(dev(np.concatenate(waves)), dev(ptr(lens)), dev(fp), int(fp[-1]), L, hop, mode, flags, status)
    e = e.cpu().numpy()
    return [e[fp[j]:fp[j + 1]] for j in range(len(waves))], int(status.item())


def device_decide(V, energies, params):
    """-> (list of bool decisions, rank (n + 1,), status)."""
    fp = ptr([len(e) for e in energies])
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    vad, rank = V.decide(dev(np.concatenate(energies).astype(np.float32)), dev(fp), *params, status)
    v = vad.cpu().numpy()
    return [v[fp[j]:fp[j + 1]].astype(bool) for j in range(len(energies))], rank.cpu().numpy(), int(status.item())


def close(got, want64):
    """|got - want| <= 2^-23 |want| for the float32 `got` against the unrounded float64 oracle."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want64.shape
    err = np.abs(got.astype(np.float64) - want64)
    assert np.all(err <= 2.0 ** -23 * np.abs(want64)), (err.max(), np.abs(want64).min())


# ------------------------------------------------------------------------------------------------------------ energies
@pytest.mark.parametrize("sr", [16000, 8000, 22050])
def test_rms_energy_against_the_oracle(V, F, sr):
    L, hop = F.frame_sizes(sr)  # (400, 160), (200, 80), (551, 220): the odd frame length
    lengths = [L // 2 + 1, L, 19200, 9001, 30011, L // 2 + 1, L]
    waves = [R.signal(sr, n, seed=j) for j, n in enumerate(lengths)]
    got, status = device_energy(V, waves, L, hop, V.VAD_RMS_CENTER)
    assert status == 0
    for w, g in zip(waves, got):
        assert len(g) == F.num_frames(len(w), L, hop)
        close(g, R.rms_energy64(w, L, hop))


@pytest.mark.parametrize("remove_dc", [False, True])
def test_log_energy_against_the_oracle(V, F, remove_dc):
    lengths = [N, N + S - 1, N + S, 19200]
    waves = [(R.signal(16000, n, seed=10 + j) + np.float32(0.01 * j)) * np.float32(32768.0) for j, n in enumerate(lengths)]
    got, status = device_energy(V, waves, N, S, V.VAD_LOGE_SNIP, V.VAD_REMOVE_DC if remove_dc else 0)
    assert status == 0
    assert [len(g) for g in got] == [1, 1, 2, 118] == [F.kaldi_num_frames(n, N, S) for n in lengths]
    for w, g in zip(waves, got):
        close(g, R.log_energy64(w, N, S, remove_dc))
    # silence: the floor, ln(FLT_EPSILON), with and without the mean removed
    got, status = device_energy(V, [np.zeros(N + S, np.float32), np.full(N, 3.0, np.float32)], N, S, V.VAD_LOGE_SNIP,
                                V.VAD_REMOVE_DC if remove_dc else 0)
    floor = np.float32(np.log(R.FLT_EPSILON))
    assert status == 0 and np.all(got[0] == floor) and (got[1][0] == floor if remove_dc else got[1][0] == np.float32(np.log(3600.0)))


def test_energy_does_not_depend_on_the_wave_alignment(V):
    """The 16-byte loads start where wave + offset is aligned: utterances at every offset mod 4 give the energies of the
    utterance alone."""
    w = R.signal(16000, 3001, seed=3)
    alone, _ = device_energy(V, [w], 400, 160, V.VAD_RMS_CENTER)
    for pad in (201, 202, 203, 204):
        got, status = device_energy(V, [R.signal(16000, pad, seed=pad), w, R.signal(16000, 777, seed=5)], 400, 160, V.VAD_RMS_CENTER)
        assert status == 0 and np.array_equal(got[1], alone[0])


# ------------------------------------------------------------------------------------------------------------ decisions
@pytest.mark.parametrize("sr,n", [(16000, 19200), (8000, 9001), (22050, 30011)])
def test_reference_decisions_exact(F, sr, n):
    L, _ = F.frame_sizes(sr)
    waves = [R.signal(sr, n), R.signal(sr, L // 2 + 1, seed=1), np.zeros(n // 3, np.float32), R.signal(sr, n // 2, seed=2)]
    got = F.energy_vad(waves, sr)
    for j, (w, g) in enumerate(zip(waves, got)):
        want, margin, _ = R.reference_vad(w, sr)
        if j != 2:
            assert margin.min() >= RMS_MARGIN
        assert g.dtype == bool and np.array_equal(g, want), j
    # (the shortest utterance the centred framing takes, win_length // 2 + 1 samples, has 2 frames at these sizes)
    assert not got[2].any() and len(got[1]) == 2 and got[0].any() and not got[0].all()
    other = F.energy_vad(waves[:1], sr, th_ratio=1.5)[0]
    want, margin, _ = R.reference_vad(waves[0], sr, th_ratio=1.5)
    assert margin.min() >= RMS_MARGIN and np.array_equal(other, want) and not np.array_equal(other, got[0])


@pytest.mark.parametrize("params", [KALDI_DEFAULT, KALDI_RECIPE])
@pytest.mark.parametrize("remove_dc", [True, False])
def test_kaldi_decisions_exact(F, params, remove_dc):
    waves = [R.signal(16000, 19200), R.signal(16000, N, seed=1), np.zeros(5000, np.float32), R.signal(16000, 9001, seed=2),
             R.signal(16000, N + 3 * S, seed=3)]
    names = ("vad-energy-threshold", "vad-energy-mean-scale", "vad-frames-context", "vad-proportion-threshold")
    got = F.kaldi_energy_vad(waves, {"remove-dc-offset": remove_dc}, dict(zip(names, params)))
    for j, (w, g) in enumerate(zip(waves, got)):
        want, margin, _ = R.kaldi_vad(w, N, S, remove_dc, *params)
        assert margin.min() >= LOGE_MARGIN
        assert np.array_equal(g, want), j
    assert not got[2].any() and len(got[1]) == 1 and len(got[4]) == 4 and got[0].any()
    if params[2]:  # the context window is cut at both edges: the decisions differ from the plain comparison somewhere
        plain, _, _ = R.kaldi_vad(waves[0], N, S, remove_dc, params[0], params[1], 0, params[3])
        assert not np.array_equal(got[0], plain)


def random_energies(rng, lengths):
    """Log-energy-like values with runs of 7 loud and 14 quiet frames."""
    return [(np.where((np.arange(n) // 7) % 3 == 0, 24.0, 10.0) + rng.normal(0.0, 1.0, n)).astype(np.float32) for n in lengths]


@pytest.mark.parametrize("params", [KALDI_DEFAULT, KALDI_RECIPE, (0.0, 0.9, 0, 1.0)])
def test_decide_across_tiles_and_chunks(V, params):
    """More frames than twice the scan's tile with utterance boundaries off the tile boundaries; one utterance longer than two
    of the mean's chunks; utterances that end exactly on a chunk boundary; rank against numpy.cumsum."""
    assert V.VAD_TILE == V.VAD_CHUNK == 1024
    lengths = [700, 1, 1500, 333, 2500, 1024, 2048, 5, 1023]
    energies = random_energies(np.random.default_rng(7), lengths)
    energies[3][:] = energies[3][0]  # an all-equal utterance in the middle
    got, rank, status = device_decide(V, energies, params)
    assert status == 0
    want = []
    for j, e in enumerate(energies):
        w, margin = R.decide(e, *params, relative=False)
        assert margin.min() >= LOGE_MARGIN
        assert np.array_equal(got[j], w), j
        want.append(w)
    flat = np.concatenate(want)
    assert rank.dtype == np.int64 and np.array_equal(rank, np.concatenate([[0], np.cumsum(flat)]))
    fp = ptr(lengths)
    assert np.array_equal(np.diff(rank[fp]), [w.sum() for w in want])


def test_vad_decide_wrapper_and_all_equal_utterance(F):
    energies = random_energies(np.random.default_rng(8), [50, 9, 1])
    energies[1][:] = np.float32(-15.942385)
    got = F.vad_decide(energies, 0.0, 1.0, 2, 0.12)
    for e, g in zip(energies, got):
        assert np.array_equal(g, R.decide(e, 0.0, 1.0, 2, 0.12, relative=False)[0])
    assert not got[1].any() and not got[2].any()  # e > mean(e) is false for equal frames, and for a single one


def test_batch_invariance_bitwise(V):
    w = R.signal(16000, 30011, seed=4)
    others = [R.signal(16000, n, seed=20 + n % 7) for n in (1203, 19200, 401, 9001)]
    for mode, L, hop, scale, params in ((V.VAD_RMS_CENTER, 400, 160, 1.0, (0.0, 1.04 / 2, 0, 1.0)),
                                        (V.VAD_LOGE_SNIP, N, S, 32768.0, KALDI_RECIPE)):
        flags = V.VAD_REMOVE_DC if mode == V.VAD_LOGE_SNIP else 0
        sc = np.float32(scale)
        alone, st0 = device_energy(V, [w * sc], L, hop, mode, flags)
        batch, st1 = device_energy(V, [o * sc for o in others[:2]] + [w * sc] + [o * sc for o in others[2:]], L, hop, mode, flags)
        assert st0 == st1 == 0 and np.array_equal(alone[0].view(np.uint32), batch[2].view(np.uint32))
        d0, _, _ = device_decide(V, alone, params)
        d1, _, _ = device_decide(V, batch, params)
        assert np.array_equal(d0[0], d1[2])
    # a long utterance (more than two chunks of the mean) alone and behind utterances that shift it off the chunk grid
    rng = np.random.default_rng(9)
    long = random_energies(rng, [3000])[0]
    d0, _, _ = device_decide(V, [long], KALDI_DEFAULT)
    d1, _, _ = device_decide(V, random_energies(rng, [77, 1500]) + [long] + random_energies(rng, [13]), KALDI_DEFAULT)
    assert np.array_equal(d0[0], d1[2])


# ------------------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("n_feat", [80, 23])
def test_selection_is_the_masked_rows_bitwise(V, n_feat):
    rng = np.random.default_rng(11)
    lengths = [300, 40, 1500, 1, 900]
    energies = random_energies(rng, lengths)
    energies[1][:] = 3.0  # no voiced frame in the middle of the batch
    fp = ptr(lengths)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    vad, rank = V.decide(dev(np.concatenate(energies)), dev(fp), 0.0, 1.0, 0, 1.0, status)
    rows = rng.standard_normal((int(fp[-1]), n_feat)).astype(np.float32)
    rows[5, 3] = np.float32("nan")  # a copy: NaN payloads and signed zeros come through
    rows[6, 0] = -0.0
    n_out = int(rank[-1].item())
    out = V.select(dev(rows), vad, rank, n_out, status)
    mask = vad.cpu().numpy().astype(bool)
    assert int(status.item()) == 0 and 0 < n_out < len(mask) and not mask[fp[1]:fp[2]].any()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), rows[mask].view(np.uint32))
    # a vad that rank is not the prefix count of (its first voiced frame cleared): that row is zeros, the status bit is set
    bad = vad.clone()
    bad[int(mask.argmax())] = 0
    out = V.select(dev(rows), bad, rank, n_out, status).cpu().numpy()
    assert int(status.item()) == V.VAD_BAD_RANK and not out[0].any()
    assert np.array_equal(out[1:].view(np.uint32), rows[mask][1:].view(np.uint32))


def test_compute_features_with_vad(F):
    sr = 16000
    waves = [R.signal(sr, 19200), np.zeros(4000, np.float32), R.signal(sr, 9001, seed=2)]
    plain = F.compute_features(waves, sr)
    marked, vads = F.compute_features(waves, sr, vad={})
    kept, vads2 = F.compute_features(waves, sr, vad={"drop": True})
    for j, w in enumerate(waves):
        want = R.reference_vad(w, sr)[0]
        assert np.array_equal(vads[j], want) and np.array_equal(vads2[j], want)
        assert np.array_equal(marked[j], plain[j]) and np.array_equal(kept[j], plain[j][want])
    assert kept[1].shape == (0, 80)
    # with rates: the decisions come from the waveform as resampled on the device
    y8 = R.signal(8000, 9001, seed=5)
    y16 = F.resample([y8], 8000, sr)[0]
    want, margin, _ = R.reference_vad(y16, sr)
    assert margin.min() >= RMS_MARGIN
    both = F.compute_features([waves[0], y8], sr, rates=[sr, 8000])
    kept, vads = F.compute_features([waves[0], y8], sr, rates=[sr, 8000], vad={"drop": True})
    assert np.array_equal(vads[1], want) and np.array_equal(kept[1], both[1][want])
    assert np.array_equal(vads[0], vads2[0]) and np.array_equal(kept[0], plain[0][vads2[0]])


# ------------------------------------------------------------------------------------------------------------ status
def test_bad_frame_ptr_sets_the_status_and_writes_nothing(V):
    e = dev(random_energies(np.random.default_rng(12), [100])[0])
    for fp in ([0, 60, 40, 100], [0, 50, 50, 100], [1, 50, 100], [0, 50, 99]):  # decreasing, empty utterance, wrong ends
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        import hip_binding as hb

        ws = torch.zeros(64, dtype=torch.int64, device="cuda")
        vad = torch.full((100,), 7, dtype=torch.uint8, device="cuda")
        rank = torch.full((101,), -1, dtype=torch.int64, device="cuda")
        hb._call("fhvae_vad_decide", hb._p(e), hb._p(dev(np.array(fp, dtype=np.int64))), len(fp) - 1, 100, 5.0, 0.5, 1, 0.6, hb._p(ws),
                 ws.numel() * 8, hb._p(vad), hb._p(rank), hb._p(status))
        assert int(status.item()) == V.VAD_BAD_PTR, fp
        assert bool((vad == 7).all()) and bool((rank == -1).all())
    # the energy kernel: a frame count that is not the utterance's, a decreasing wave_ptr, an utterance that is too short
    w = dev(R.signal(16000, 4000))
    for wp, fp in (([0, 2000, 4000], [0, 13, 27]), ([0, 3000, 2000, 4000], [0, 19, 20, 26]), ([0, 100, 4000], [0, 1, 26])):
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        import hip_binding as hb

        out = torch.full((fp[-1],), 123.0, device="cuda")
        hb._call("fhvae_vad_energy", hb._p(w), 4000, hb._p(dev(np.array(wp, dtype=np.int64))), hb._p(dev(np.array(fp, dtype=np.int64))),
                 len(wp) - 1, fp[-1], 400, 160, V.VAD_RMS_CENTER, 0, hb._p(out), hb._p(status))
        assert int(status.item()) == V.VAD_BAD_PTR, (wp, fp)
        assert bool((out == 123.0).all())


# ------------------------------------------------------------------------------------------------------------ the reference's call
def test_audio_utils_energy_vad(F):
    from utils import AudioUtils

    for sr, n in ((16000, 19200), (22050, 30011)):
        y = R.signal(sr, n)
        got = AudioUtils.energy_vad(y, sr)
        want, margin, _ = R.reference_vad(y, sr)
        assert margin.min() >= RMS_MARGIN
        assert got.shape == (1, len(want)) and got.dtype.kind == "i" and np.array_equal(got[0], want.astype(int))
    got = AudioUtils.energy_vad(y, sr, hop_t=0.005, win_t=0.032, th_ratio=0.8)
    want, margin, _ = R.reference_vad(y, sr, 0.032, 0.005, 0.8)
    assert margin.min() >= RMS_MARGIN and np.array_equal(got[0], want.astype(int))


# ------------------------------------------------------------------------------------------------------------ the CLIs
@pytest.fixture(scope="module")
def corpus(tmp_path_factory, F):
    """Three files, the one in the middle silent: <dir>/train/wav.scp -> (dir, keys, the waveforms as the CLIs read them)."""
    d = tmp_path_factory.mktemp("vad_corpus")
    (d / "train").mkdir()
    keys = ["spk1-a", "spk1-silent", "spk2-b"]
    for key, y in zip(keys, (R.signal(16000, 19200), np.zeros(8000, np.float32), R.signal(16000, 9001, seed=2))):
        F.write_wav(d / ("%s.wav" % key), y, 16000)
    (d / "train" / "wav.scp").write_text("".join("%s %s\n" % (k, d / ("%s.wav" % k)) for k in keys))
    return d, keys, [F.read_wav(d / ("%s.wav" % k))[0] for k in keys]


def scp(path):
    return [ln.split(None, 1) for ln in open(path).read().splitlines()]


def test_prepare_numpy_cli(F, corpus, tmp_path, capsys):
    import prepare_numpy_data as PN

    d, keys, waves = corpus
    want = []
    for j, w in enumerate(waves):
        v, margin, _ = R.reference_vad(w, 16000)
        assert j == 1 or margin.min() >= RMS_MARGIN
        want.append(v)
    out = tmp_path / "np"
    base = [str(d), "--np_dir", str(out), "--set_name", "train"]
    assert PN.main(base) == 0
    files = ["feats.scp", "len.scp"] + ["%s.npy" % k for k in keys]
    plain = {f: open(out / "train" / f, "rb").read() for f in files}
    assert not os.path.exists(out / "train" / "vad.scp")
    feats = [np.load(out / "train" / ("%s.npy" % k)) for k in keys]

    assert PN.main(base + ["--vad", "mark"]) == 0
    assert {f: open(out / "train" / f, "rb").read() for f in files} == plain
    marks = scp(out / "train" / "vad.scp")
    assert [k for k, _ in marks] == keys
    for (_, path), v in zip(marks, want):
        got = np.load(path)
        assert got.dtype == np.uint8 and np.array_equal(got, v.astype(np.uint8))

    capsys.readouterr()
    drop = tmp_path / "np_drop"
    assert PN.main([str(d), "--np_dir", str(drop), "--set_name", "train", "--vad", "drop"]) == 0
    io = capsys.readouterr()
    assert "spk1-silent" in io.err and "no voiced frame" in io.err and "spk1-a" not in io.err
    total, kept = sum(len(v) for v in want), sum(int(v.sum()) for v in want)
    assert "Skipped 1 of 3 sequences" in io.out and "dropped %d of %d frames" % (total - kept, total) in io.out
    assert scp(drop / "train" / "len.scp") == [[keys[j], str(int(want[j].sum()))] for j in (0, 2)]
    assert [k for k, _ in scp(drop / "train" / "feats.scp")] == [keys[0], keys[2]]
    assert not os.path.exists(drop / "train" / "spk1-silent.npy")
    for j in (0, 2):
        assert np.array_equal(np.load(drop / "train" / ("%s.npy" % keys[j])), feats[j][want[j]])
    for (_, path), v in zip(scp(drop / "train" / "vad.scp"), want):  # over the ORIGINAL frames, the skipped file included
        assert np.array_equal(np.load(path), v.astype(np.uint8))
    other = tmp_path / "np_ratio"
    assert PN.main([str(d), "--np_dir", str(other), "--set_name", "train", "--vad", "mark", "--vad_th_ratio", "1.5"]) == 0
    v15, margin, _ = R.reference_vad(waves[0], 16000, th_ratio=1.5)
    assert margin.min() >= RMS_MARGIN and np.array_equal(np.load(other / "train" / "spk1-a.vad.npy"), v15.astype(np.uint8))


def test_prepare_kaldi_cli(F, corpus, tmp_path, capsys):
    import shutil

    import kaldi_io_lite as K
    import prepare_kaldi_data as PK

    _, keys, waves = corpus
    conf = tmp_path / "vad.conf"
    conf.write_text("--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n--vad-frames-context=2\n--vad-proportion-threshold=0.12\n")
    want = []
    for w in waves:
        v, margin, _ = R.kaldi_vad(w, N, S, True, *KALDI_RECIPE)
        assert margin.min() >= LOGE_MARGIN
        want.append(v)
    assert not want[1].any() and want[0].any() and want[2].any()

    def run(name, *extra):
        d = tmp_path / name
        shutil.copytree(corpus[0] / "train", d / "train")
        assert PK.main([str(d), "--fbank_conf", CONF, "--set_name", "train"] + list(extra)) == 0
        return d / "train"

    files = ["feats.ark", "feats.scp", "len.scp"]
    mark = run("mark")
    plain = {f: open(mark / f, "rb").read() for f in files}
    assert not os.path.exists(mark / "vad.ark")
    feats = [m for _, m in K.read_ark(str(mark / "feats.ark"))]
    assert PK.main([str(tmp_path / "mark"), "--fbank_conf", CONF, "--set_name", "train", "--vad", "mark", "--vad_conf", str(conf)]) == 0
    assert {f: open(mark / f, "rb").read() for f in files} == plain
    got = list(K.read_vec_ark(str(mark / "vad.ark")))
    assert [k for k, _ in got] == keys == [k for k, _ in scp(mark / "vad.scp")]
    for (_, g), v in zip(got, want):
        assert g.dtype == np.float32 and np.array_equal(g, v.astype(np.float32))
    for (_, spec), v in zip(scp(mark / "vad.scp"), want):
        assert np.array_equal(K.load_vec(spec), v.astype(np.float32))
    # Kaldi's own defaults without --vad_conf
    assert PK.main([str(tmp_path / "mark"), "--fbank_conf", CONF, "--set_name", "train", "--vad", "mark"]) == 0
    for (_, g), w in zip(K.read_vec_ark(str(mark / "vad.ark")), waves):
        v, margin, _ = R.kaldi_vad(w, N, S, True, *KALDI_DEFAULT)
        assert margin.min() >= LOGE_MARGIN and np.array_equal(g, v.astype(np.float32))

    capsys.readouterr()
    drop = run("drop", "--vad", "drop", "--vad_conf", str(conf))
    io = capsys.readouterr()
    assert "spk1-silent" in io.err and "no voiced frame" in io.err and "spk1-a" not in io.err
    total, kept = sum(len(v) for v in want), sum(int(v.sum()) for v in want)
    assert "Skipped 1 of 3 utterances" in io.out and "dropped %d of %d frames" % (total - kept, total) in io.out
    assert scp(drop / "len.scp") == [[keys[j], str(int(want[j].sum()))] for j in (0, 2)]
    got = list(K.read_ark(str(drop / "feats.ark")))
    assert [k for k, _ in got] == [keys[0], keys[2]] == [k for k, _ in scp(drop / "feats.scp")]
    for (_, g), j in zip(got, (0, 2)):
        assert np.array_equal(g, feats[j][want[j]])
    assert [k for k, _ in K.read_vec_ark(str(drop / "vad.ark"))] == keys

    # --compress: only the kept rows are coded.  The codec's step: a value is coded on at most 63 .. 128 levels between two of
    # its column's percentiles, which lie within the matrix' range, so it decodes within range / 63 of itself
    comp = run("comp", "--vad", "drop", "--vad_conf", str(conf), "--compress")
    assert scp(comp / "len.scp") == scp(drop / "len.scp")
    for (key, spec), j in zip(scp(comp / "feats.scp"), (0, 2)):
        assert key == keys[j] and K.read_raw(spec)[0] == "CM"
        ref = feats[j][want[j]]
        dec = K.load_mat(spec)
        assert dec.shape == ref.shape and np.abs(dec - ref).max() <= (ref.max() - ref.min()) / 63.0
