"""The frame-level layer without a GPU: the host geometry of frames.py against brute-force enumeration, chunk_plan's properties,
the two exported entry points' argument errors (they return before any launch), the oracle's own identities, the
CLI's argument errors and an archive round trip through its writer."""
import ctypes
import os

import numpy as np
import pytest

import frames_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import frames

    return frames.load_library()


def test_covering_against_enumeration():
    import frames as FR

    for T in range(1, 25):
        assert FR.left(T) == T // 2 and FR.max_overlap_shift(T) == T - T // 2
        for s in range(1, T + 3):
            for n in range(1, 70):
                assert FR.num_windows(n, s) == R.n_windows(n, s)
                for f in range(n):
                    ks = R.brute_covering(f, n, T, s)
                    k0, k1 = FR.covering(f, n, T, s)
                    assert list(range(k0, k1 + 1)) == ks, (T, s, n, f)
                    if s <= T - T // 2:  # the coverage claim: every frame of every utterance has a window
                        assert ks, (T, s, n, f)


def test_coverage_bound_is_needed():
    # one step above T - T // 2 some frame of some utterance is uncovered: the bound of overlap_mean is not loose
    for T in range(1, 25):
        s = T - T // 2 + 1
        assert any(not R.brute_covering(f, n, T, s) for n in range(1, 70) for f in range(n)), T


LENGTHS = [1, 2, 19, 45, 400]


@pytest.mark.parametrize("s", [1, 3, 10])
@pytest.mark.parametrize("max_windows", [40, 64])
def test_chunk_plan_properties(s, max_windows):
    import frames as FR

    T = 20
    utt = np.concatenate([[0], np.cumsum(LENGTHS)])
    win = np.concatenate([[0], np.cumsum([R.n_windows(n, s) for n in LENGTHS])])
    halo = -(-T // s) - 1
    # overlap=False: the window ranges tile [0, total windows)
    flat = FR.chunk_plan(LENGTHS, T, s, max_windows, overlap=False)
    assert [c[0] for c in flat] == list(np.cumsum([0] + [c[1] for c in flat])[:-1]) and sum(c[1] for c in flat) == win[-1]
    assert all(1 <= c[1] <= max_windows for c in flat)
    plan = FR.chunk_plan(LENGTHS, T, s, max_windows, overlap=True)
    assert len(plan) >= -(-int(win[-1]) // max_windows)
    if s < 10:  # the long utterance is split several times (at shift 10 the whole corpus is 49 windows)
        assert sum(utt[4] < c[2] < utt[5] for c in plan) >= 2
    g = 0
    for w0, B, g0, G in plan:
        assert g0 == g and G >= 1 and 1 <= B <= max_windows and 0 <= w0 and w0 + B <= win[-1]  # tiling, bound
        g += G
        halo_left = halo_right = 0
        seen = set()
        for fr in range(g0, g0 + G):
            u = int(np.searchsorted(utt, fr, side="right")) - 1
            for k in R.brute_covering(fr - utt[u], LENGTHS[u], T, s):
                assert w0 <= win[u] + k < w0 + B  # every covering window inside
                seen.add(int(win[u] + k))
        assert seen == set(range(w0, w0 + B))  # and no window that covers none of the chunk's frames
        for w in range(w0, w0 + B):  # the halo: windows centred on a frame outside the chunk's frame range
            u = int(np.searchsorted(win, w, side="right")) - 1
            centre = utt[u] + (w - win[u]) * s
            halo_left += centre < g0
            halo_right += centre >= g0 + G
        assert halo_left <= halo and halo_right <= halo, (w0, B, g0, G)
    assert g == utt[-1]


def test_chunk_plan_refuses_what_does_not_fit():
    import frames as FR

    # T = 20, shift 1: splitting needs 19 windows of halo on both sides and one window between them
    with pytest.raises(ValueError, match="max_windows = 20 is too small"):
        FR.chunk_plan(LENGTHS, 20, 1, 20, overlap=True)
    assert len(FR.chunk_plan(LENGTHS, 20, 1, 20, overlap=False)) == -(-sum(LENGTHS) // 20)
    # utterances that fit are not split when splitting is not allowed
    assert FR.chunk_plan([5, 19], 20, 1, 20, overlap=True) == [(0, 5, 0, 5), (5, 19, 5, 19)]
    with pytest.raises(ValueError, match="shift = 11"):
        FR.chunk_plan(LENGTHS, 20, 11, 64, overlap=True)
    with pytest.raises(ValueError, match="at least one frame"):
        FR.chunk_plan([3, 0], 20, 1, 64, overlap=False)


def test_symbols_exported_and_errors_before_any_launch(lib):
    import frames as FR
    import hip_binding as hb

    for name in FR.FRAMES_SIGNATURES:
        assert hasattr(lib, name) and name not in hb.SIGNATURES
    assert lib.fhvae_abi_version() == 12
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    g, o = lib.fhvae_frames_gather, lib.fhvae_frames_overlap_mean
    #        pool n  utt win U  w0 B  T  F  s  mean inv btf tbf status stream
    good = [p, 8, p, p, 1, 0, 2, 4, 2, 1, None, None, p, None, p, None]
    for i in (0, 2, 3, 14):  # pool, utt_ptr, win_ptr, status
        assert g(*[None if j == i else a for j, a in enumerate(good)]) == -1
    assert g(*[None if j in (12, 13) else a for j, a in enumerate(good)]) == -1  # neither output
    assert g(*[p if j == 10 else a for j, a in enumerate(good)]) == -1  # mean without inv_std
    for i in (1, 4, 7, 8, 9):  # pool_frames, U, T, F, shift
        for bad in (0, -3):
            assert g(*[bad if j == i else a for j, a in enumerate(good)]) == -2
    assert g(*[-1 if j == 6 else a for j, a in enumerate(good)]) == -2 and g(*[-1 if j == 5 else a for j, a in enumerate(good)]) == -2
    assert g(*[0 if j == 6 else a for j, a in enumerate(good)]) == 0  # B == 0: nothing to do, nothing launched
    #        seg w0 B  utt win U  g0 G  T  F  s  mean std out status stream
    good = [p, 0, 2, p, p, 1, 0, 2, 4, 2, 1, None, None, p, p, None]
    for i in (0, 3, 4, 13, 14):  # seg, utt_ptr, win_ptr, out, status
        assert o(*[None if j == i else a for j, a in enumerate(good)]) == -1
    assert o(*[p if j == 12 else a for j, a in enumerate(good)]) == -1  # std without mean
    for i in (2, 5, 8, 9, 10):  # B, U, T, F, shift
        for bad in (0, -3):
            assert o(*[bad if j == i else a for j, a in enumerate(good)]) == -2
    assert o(*[-1 if j == 7 else a for j, a in enumerate(good)]) == -2
    assert o(*[0 if j == 7 else a for j, a in enumerate(good)]) == 0  # G == 0
    # shift above T - T / 2 leaves frames uncovered: refused for every T, at the first shift that is too large
    for T in (1, 4, 5, 20, 21):
        ok = [T if j == 8 else (T - T // 2 + 1) if j == 10 else a for j, a in enumerate(good)]
        assert o(*ok) == -2, T
        assert o(*[0 if j == 7 else a for j, a in enumerate([T if j == 8 else (T - T // 2) if j == 10 else a for j, a in enumerate(good)])]) == 0


def _short(a):
    """float32 values cut to 19 significant bits (the low 5 bits of the significand cleared)."""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFFFFE0)).view(np.float32)


def test_oracle_identities():
    """The overlap mean of the windows of x at shift 1 and without MVN is x again, bit for bit: a frame is then the mean of
    c <= T <= 24 copies of itself.  That mean is exact when c * v is: the running sums j * v, j <= 24 < 2^5, are representable
    when v has at most 24 - 5 = 19 significant bits, and the quotient c * v / c is then v.  For values that use all 24 bits
    the statement is false however the c copies are added in f32: already 2 v + v rounds, and fl(3 v) / 3 rounds to a
    neighbour of v for 1 398 101 of the 2^23 significands (for 6 829 156 of them at c = 24); both halves are asserted here."""
    rng = np.random.default_rng(0)
    lengths = [1, 2, 19, 45]
    for T in (24, 20, 5, 1):
        feats = [_short(rng.standard_normal((n, 3)) * 10 ** rng.uniform(-3, 3, (n, 3))) for n in lengths]
        x = np.concatenate(feats)
        got = R.overlap_mean(R.windows(feats, T, 1), lengths, T, 1)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), x.view(np.uint32))
    # every 19-bit significand (binade [1, 2); a power of two changes nothing for normal numbers), the running sum rounded at
    # every step as the kernel and the oracle round it
    vals = ((np.arange(1 << 18, dtype=np.uint32) << np.uint32(5)) | np.uint32(0x3F800000)).view(np.float32)
    acc = vals.copy()
    for c in range(2, 25):
        acc = acc + vals
        assert acc.dtype == np.float32 and np.array_equal(acc / np.float32(c), vals), c
    # all 24 bits: not an identity (the counts of the docstring)
    full = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3F800000)).view(np.float32)
    assert int((((full + full) + full) / np.float32(3) != full).sum()) == 1398101
    # windows: shape, the centre frame, the replicated edges
    w = R.windows(feats, 5, 3)
    assert w.shape == (sum(R.n_windows(n, 3) for n in lengths), 5, 3)
    assert np.array_equal(w[0], np.repeat(feats[0], 5, axis=0))  # the 1-frame utterance: its frame five times
    k = 1 + 1  # the first window of the 19-frame utterance; its window 2 is centred on frame 6
    assert np.array_equal(w[k + 2], feats[2][4:9]) and np.array_equal(w[k][:3], np.repeat(feats[2][:1], 3, axis=0))


@pytest.mark.parametrize("out_format,compress", [("kaldi", False), ("kaldi", True), ("numpy", False)])
def test_archive_round_trip(tmp_path, out_format, compress):
    import extract_latents as EL
    import kaldi_io_lite as K
    from datasets import KaldiDataset, NumpyDataset

    rng = np.random.default_rng(1)
    keys = ["spk1-a", "spk1-b", "spk2-a", "one"]
    mats = [rng.standard_normal((n, 7)).astype(np.float32) for n in (30, 9, 12, 1)]
    d = tmp_path / "z1"
    assert EL.write_archive(str(d), keys, mats, out_format, compress=compress) == 4
    Dataset = KaldiDataset if out_format == "kaldi" else NumpyDataset
    ds = Dataset(str(d / "feats.scp"), str(d / "len.scp"), 0, None, 20, 8, False)
    assert ds.seq_keys == keys and ds.seq_lens == [30, 9, 12, 1]  # every key, in order, the 1-row one included
    for i, m in enumerate(mats):
        got = ds.load_seq(i)
        if compress:
            tok, payload = K.compress_mat(m, "auto")
            want = K.CompressedMatrix(tok, K.header_bytes(m), payload).decode()
        else:
            want = m
        assert got.dtype == np.float32 and np.array_equal(got, want)


def test_pool_refuses_an_entry_without_rows(tmp_path, lib):
    # (raised from the lengths, before anything is uploaded: no GPU needed)
    import frames as FR
    from datasets import NumpyDataset

    with open(tmp_path / "feats.scp", "w") as fs, open(tmp_path / "len.scp", "w") as ls:
        for k, n in (("a", 3), ("empty-one", 0), ("b", 2)):
            np.save(tmp_path / (k + ".npy"), np.zeros((n, 4), np.float32))
            fs.write("%s %s\n" % (k, tmp_path / (k + ".npy")))
            ls.write("%s %d\n" % (k, n))
    ds = NumpyDataset(str(tmp_path / "feats.scp"), str(tmp_path / "len.scp"), 0, None, 20, 1, False)
    assert ds.seq_keys == ["a", "empty-one", "b"]
    with pytest.raises(ValueError, match="utterance empty-one has no frames"):
        FR.FramePool(ds, 20, 1, device="cpu")
    with pytest.raises(ValueError, match="utterance 1 has no frames"):
        FR.FramePool([np.zeros((3, 4), np.float32), np.zeros((0, 4), np.float32)], 20, 1, device="cpu")


def _checkpoint(tmp_path):
    import torch

    import utils
    from fhvae import FHVAE

    torch.manual_seed(0)
    m = FHVAE(20 * 4, [8, 8], [8, 8], 4, 4, [8, 8], seg_len=20)
    utils.save_checkpoint(m, None, [], {}, "t", 1, 1, 0.0, 0.0, str(tmp_path))
    return str(tmp_path / "fhvae_t_e1.tar")


def test_cli_argument_errors(tmp_path, capsys, lib):
    import extract_latents as EL

    ck = _checkpoint(tmp_path)
    base = ["--checkpoint", ck, "--feat-scp", "x.scp", "--len-scp", "y.scp", "--out", str(tmp_path / "o")]
    for extra, words in ((["--what", "recon", "--shift", "11"], ("--shift 11", "T - T // 2 = 10", "T = 20")),
                         (["--what", "z1", "convert", "--shift", "12", "--convert-to", "a"], ("--shift 12", "= 10")),
                         (["--what", "convert"], ("--convert-to",)),
                         (["--what", "z1", "--out-format", "numpy", "--compress"], ("--compress",)),
                         (["--what", "z1", "--shift", "0"], ("--shift 0",))):
        with pytest.raises(SystemExit) as e:
            EL.main(base + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), err
