"""Every row-tile height of the audio kernels on a MI355X (csrc/feats.hip, synth.hip, kaldi_fbank.hip, resample.hip,
melinv.hip) against their float64 oracles: the cases of tests/audio_cases.py, compared by tests/audio_compare.py (per
element, bounds derived in that module's docstring; the worst and mean error in units next to a float32 sequential
emulation's, within 2 x of it), bitwise equality of the batch with each utterance alone at every height, and sentinels
behind every output buffer.  The batches put utterance boundaries inside tiles and leave the last tile part empty."""
import numpy as np
import pytest
import torch

import audio_cases as C
import audio_compare as AC

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GUARD = 64  # rows (or samples) behind the logical end of an output buffer


@pytest.fixture(scope="module")
def F():
    import build_ext

    build_ext.build(verbose=False)
    import features
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return features


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(shape):
    """A sentinel-filled buffer with GUARD more rows than `shape` -> (the whole buffer, the logical view the kernel gets)."""
    whole = torch.full((shape[0] + GUARD,) + tuple(shape[1:]), SENTINEL, device="cuda")
    return whole, whole[:shape[0]]


def take(whole, n):
    """The logical part on the host; asserts the guard untouched and everything before it written."""
    a = whole.cpu().numpy()
    assert np.all(a[n:] == SENTINEL), "the kernel wrote behind the end of its output"
    assert not np.any(a[:n] == SENTINEL), "the kernel left output elements unwritten"
    return a[:n]


def split(a, ptr):
    return [a[ptr[j]:ptr[j + 1]] for j in range(len(ptr) - 1)]


# ------------------------------------------------------------------------------------------------------------ feats
def run_feats(F, c, waves, bases):
    import hip_binding as hb

    n_fft, hop, n_mels, ftype = c["n_fft"], c["hop"], c["n_mels"], c["ftype"]
    lens = np.array([len(w) for w in waves], dtype=np.int64)
    fp = C_ptr(F.num_frames(lens, n_fft, hop))
    whole, out = guarded((int(fp[-1]), n_mels if ftype == "fbank" else n_fft // 2 + 1))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    hb.feats_fwd(dev(np.concatenate(waves)), dev(C_ptr(lens)), dev(fp), bases[0], bases[1], n_fft, hop, n_mels, ftype, out, status)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return split(take(whole, int(fp[-1])), fp)


def C_ptr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


@pytest.mark.parametrize("c", C.runnable(C.FEATS), ids=C.case_id)
def test_feats(F, c):
    import hip_binding as hb

    assert hb.load_library().fhvae_feats_tile_rows(c["n_fft"], hb.FEATS_TYPES[c["ftype"]]) == c["rows"]
    waves, oracles = C.feats_waves(c), C.feats_oracles(c)
    bases = (dev(F.dft_basis(c["n_fft"])), dev(F.mel_basis(c["sr"], c["n_fft"], c["n_mels"])) if c["ftype"] == "fbank" else None)
    got = run_feats(F, c, waves, bases)
    assert [len(g) for g in got][:4] == C.frame_counts(c["rows"]) and [len(g) for g in got] == [len(o.A) for o in oracles]
    for j, w in enumerate(waves):  # the fixed-order claim of audio_tile.h, at this height: batch == alone, bitwise
        assert np.array_equal(run_feats(F, c, [w], bases)[0], got[j]), j
    units = np.concatenate([o.units(g) for o, g in zip(oracles, got)])
    emu = np.concatenate([o.units(o.emulate_f32(), enforce=False) for o in oracles])
    assert len(units) == len(emu)
    if len(units):  # (n_fft = 2 fbank: every mel filter is empty, every element is the floor, compared for equality)
        AC.stat_line("feats " + C.case_id(c), units, emu)
    else:
        print("feats %-28s every element is the floor" % C.case_id(c))


# ------------------------------------------------------------------------------------------------------------ resample
@pytest.mark.parametrize("sr_in,sr_out", C.RESAMPLE_NEW)
def test_resample(F, sr_in, sr_out):
    """The pair that reaches the 16-row tile.  Rows per utterance 15, 16, 17, 35 (an output row is P * L samples), a single
    sample, digital silence, and first the short utterance the statistical bound is measured on."""
    import hip_binding as hb
    import resample_ref as R

    b = F.resample_bank(sr_in, sr_out)
    tile = hb.load_library().fhvae_resample_tile_rows(b.KP)
    assert tile == dict(C.RESAMPLE_PAIRS)[(sr_in, sr_out)]
    row_in = b.P * b.M
    waves = [C.speechlike(sr_in, sr_in // 50, sr_in)]
    waves += [C.speechlike(sr_in, (r - 1) * row_in + row_in // 2, sr_in + r) for r in C.frame_counts(tile)]
    waves += [np.array([0.25], np.float32), np.zeros(2 * b.M + 5, np.float32)]
    lens = np.array([len(w) for w in waves], dtype=np.int64)
    olens = F.resampled_length(lens, sr_in, sr_out)
    rows = -(-olens // (b.P * b.L))
    assert list(rows[1:5]) == C.frame_counts(tile)
    rd = F._ResampleDev(b, "cuda")

    def run(idx):
        ptrs = [C_ptr(v[idx]) for v in (lens, olens, rows)]
        whole, out = guarded((int(ptrs[1][-1]),))
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        exc = dev(b.exceptions(int(-(-olens[idx].max() // b.L))).copy()) if rd.alt is not None else None
        hb.resample_fwd(dev(np.concatenate([waves[j] for j in idx])), dev(ptrs[0]), dev(ptrs[1]), dev(ptrs[2]), int(ptrs[2][-1]),
                        rd.bank, rd.chunks, b.L, b.M, b.P, b.WL, b.ratio, exc, rd.alt if exc is not None else None, b.alt_wl, out,
                        status)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        return split(take(whole, int(ptrs[1][-1])), ptrs[1])

    got = run(list(range(len(waves))))
    for j in range(len(waves)):
        assert np.array_equal(run([j])[0], got[j]), j
    for j, (g, y) in enumerate(zip(got, waves)):
        want, cond, _ = R.resample(y, sr_in, sr_out)
        units = AC.dense_units(g, want, AC.EPS * cond, b.terms(len(g)), what="resample %d -> %d utterance %d" % (sr_in, sr_out, j))
        assert not g[R.lengths(len(y), sr_in, sr_out)[0]:].any()
        if not np.any(y):
            assert not g.any()
        if j == 0:
            emu = R.resample_f32_sequential(y, sr_in, sr_out)
            m = cond > 0
            AC.stat_line("resample %d -> %d" % (sr_in, sr_out), units, (np.abs(emu.astype(np.float64) - want) / (AC.EPS * cond))[m])


# ------------------------------------------------------------------------------------------------------------ melinv
@pytest.mark.parametrize("c", C.MELINV_NEW, ids=lambda c: "tf%d" % c["rows"])
def test_melinv(F, c):
    """TF = 16 and TF = 8 through test_melinv_gpu's trajectory criterion (1 and 3 iterations: at most 4 x the drift of the
    oracle's float32 emulation, floor 8 * 2^-24, no frame excluded) and its bitwise batch invariance."""
    import feats_ref
    import hip_binding as hb
    import melinv_ref as R

    sr, win_t, n_mels, tf = c["sr"], c["win_t"], c["n_mels"], c["rows"]
    n_fft, hop = feats_ref.sizes(sr, win_t)
    n_bins = n_fft // 2 + 1
    assert hb.load_library().fhvae_mel_invert_tile_rows(n_mels, n_bins) == tf
    frames = C.frame_counts(tf) + [2, 30]  # (30 frames of test_signal hold a stretch of digital silence)
    lms = []
    for j, f in enumerate(frames):
        y = R.test_signal(sr, hop * (f - 1) + n_fft % 2, 30 + j)
        lm = feats_ref.features(y, sr, "fbank", win_t=win_t, n_mels=n_mels).astype(np.float32)
        assert lm.shape == (f, n_mels)
        lms.append(lm)
    lm_all = np.concatenate(lms)
    fp = C_ptr(frames)
    M, A = np.exp(lm_all.astype(np.float64)), R.bank(sr, n_mels, win_t)
    iters = (1, 3)
    _, k64 = R.fista(M, A, 3, keep=iters)
    _, k32 = R.fista(M, A, 3, np.float32, keep=iters)

    def run(lm, it):
        md = F._MelInvDev(sr, n_fft, n_mels, it, "cuda")
        whole, out = guarded((lm.shape[0], n_bins))
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        hb.mel_invert(dev(lm), md.bin_filt, md.bin_w, md.filt_first, md.filt_off, md.filt_w, md.inv_l, md.beta, out, st, in_log=True,
                      out_log=False)
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        return take(whole, lm.shape[0])

    bad = []
    for it in iters:
        x = run(lm_all, it)
        assert np.all(np.isfinite(x))
        for j, lm in enumerate(lms):
            assert np.array_equal(run(lm, it), x[fp[j]:fp[j + 1]]), (it, j)
        got, emu = R.drift(x, k64[it]), R.drift(k32[it], k64[it])
        bound = max(4.0 * emu, 8.0 * 2.0 ** -24)
        print("melinv TF %d, %d iterations: drift kernel %.3g, float32 emulation %.3g, bound %.3g" % (tf, it, got, emu, bound))
        if got > bound:
            bad.append((it, got, bound))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ synth
def _units(got, want, u):
    m = u > 0
    return (np.abs(got.astype(np.float64) - want) / np.where(m, u, 1.0))[m]


@pytest.mark.parametrize("c", C.runnable(C.SYNTH), ids=C.case_id)
def test_synth(F, c):
    """istft (the workspace of the inverse DFT and the overlap-added waveform), project without tprev, with tprev and with
    momentum 0, at every height: hard bounds on every element, the yardstick on the first two utterances."""
    import hip_binding as hb

    n_fft, hop = c["n_fft"], c["hop"]
    n_bins, KP = n_fft // 2 + 1, (n_fft + 15) // 16 * 16
    assert hb.load_library().fhvae_synth_tile_rows(n_fft) == c["rows"]
    o = C.synth_oracles(c)
    frames = np.array(o["frames"], dtype=np.int64)
    fp, wp = C_ptr(frames), C_ptr(hop * (frames - 1))
    dft, syn, wsq = dev(F.dft_basis(n_fft)), dev(F.synth_basis(n_fft)), dev(F.window_sq(n_fft))
    assert (o["S"] == 0).all(axis=1).any()  # silent frames

    def istft(X, idx):
        f, w = C_ptr(frames[idx]), C_ptr(hop * (frames[idx] - 1))
        rows = np.concatenate([np.arange(fp[j], fp[j + 1]) for j in idx])
        ws_whole, ws = guarded((int(f[-1]), KP))
        y_whole, y = guarded((int(w[-1]),))
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        hb.synth_istft(dev(AC.pack32(X[rows])), dev(w), dev(f), syn, wsq, n_fft, hop, ws, y, st)
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        return take(ws_whole, int(f[-1])), take(y_whole, int(w[-1]))

    def project(y, tprev, coef, idx):
        f, w = C_ptr(frames[idx]), C_ptr(hop * (frames[idx] - 1))
        rows = np.concatenate([np.arange(fp[j], fp[j + 1]) for j in idx])
        smp = np.concatenate([np.arange(wp[j], wp[j + 1]) for j in idx])
        r_whole, reb = guarded((int(f[-1]), n_bins, 2))
        n_whole, nxt = guarded((int(f[-1]), n_bins, 2))
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        hb.synth_project(dev(y[smp]), dev(w), dev(f), dft, dev(o["S"][rows].astype(np.float32)),
                         None if tprev is None else dev(AC.pack32(tprev[rows])), coef, n_fft, hop, reb, nxt, st)
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        return take(r_whole, int(f[-1])), take(n_whole, int(f[-1]))

    everything, what = list(range(len(frames))), "synth " + C.case_id(c)
    r2 = int(fp[2])
    n2 = int(wp[2])
    ist = o["ist"]
    ws, y = istft(o["X0"], everything)
    for j in everything:
        ws1, y1 = istft(o["X0"], [j])
        assert np.array_equal(ws1, ws[fp[j]:fp[j + 1]]) and np.array_equal(y1, y[wp[j]:wp[j + 1]]), j
    assert not ws[:, n_fft:].any()  # the padded samples of a workspace row are written as zeros
    AC.dense_units(ws[:, :n_fft], ist.ws, ist.uws, ist.terms, what=what + " workspace")
    AC.dense_units(y, ist.y, ist.uy, 0, c=0, extra=ist.Ey, what=what + " istft")
    ws_e, y_e = ist.emulate_f32(2)
    AC.stat_line(what + " idft", _units(ws[:r2, :n_fft], ist.ws[:r2], ist.uws[:r2]), _units(ws_e, ist.ws[:r2], ist.uws[:r2]))
    AC.stat_line(what + " ola", _units(y[:n2], ist.y[:n2], ist.uy[:n2]), _units(y_e, ist.y[:n2], ist.uy[:n2]))
    for name, yk, tprev, coef, stat in (("p1", "y1", None, o["coef"], True), ("p2", "y2", o["tprev"], o["coef"], True),
                                        ("p0", "y2", o["tprev"], 0.0, False)):
        p = o[name]
        reb, nxt = project(o[yk], tprev, coef, everything)
        for j in everything:
            reb1, nxt1 = project(o[yk], tprev, coef, [j])
            assert np.array_equal(reb1, reb[fp[j]:fp[j + 1]]) and np.array_equal(nxt1, nxt[fp[j]:fp[j + 1]]), (name, j)
        p.check(reb, nxt, "%s %s" % (what, name))
        if stat:
            reb_e, nxt_e = p.emulate_f32(r2)
            AC.stat_line("%s %s rebuilt" % (what, name), p.rebuilt_units(reb[:r2]), p.rebuilt_units(reb_e))
            AC.stat_line("%s %s next" % (what, name), p.next_units(nxt[:r2]), p.next_units(nxt_e))


# ------------------------------------------------------------------------------------------------------------ kaldi fbank
@pytest.mark.parametrize("c", C.runnable(C.KALDI), ids=C.case_id)
def test_kaldi_fbank(F, c):
    """Dither 0 against the oracle at every height (48 rows, TM = 3, among them); with dither only that a launch repeats
    bitwise and that an utterance alone equals itself in the batch (the noise is a function of seed, stream and frame)."""
    import hip_binding as hb

    N, S, P, n_mels = c["N"], c["S"], c["P"], c["n_mels"]
    assert hb.load_library().fhvae_kaldi_fbank_tile_rows(N, P, n_mels) == c["rows"]
    waves, oracles = C.kaldi_waves(c), C.kaldi_oracles(c)
    dft, mel = dev(F.kaldi_dft_basis(N, P)), dev(F.kaldi_mel_basis(c["sr"], P, n_mels))
    flags = hb.KALDI_REMOVE_DC | hb.KALDI_USE_LOG | hb.KALDI_USE_POWER
    ids = np.arange(len(waves), dtype=np.int64) * 7919 + 11

    def run(idx, dither, flags=flags):
        lens = np.array([len(waves[j]) for j in idx], dtype=np.int64)
        fp = C_ptr(F.kaldi_num_frames(lens, N, S))
        whole, out = guarded((int(fp[-1]), n_mels))
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        hb.kaldi_fbank_fwd(dev(np.concatenate([waves[j] for j in idx])), dev(C_ptr(lens)), dev(fp), dev(ids[idx]) if dither else None,
                           dft, mel, N, S, P, n_mels, 0.97, dither, 5, flags, out, st)
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        return split(take(whole, int(fp[-1])), fp)

    everything = list(range(len(waves)))
    got = run(everything, 0.0)
    assert [len(g) for g in got] == C.frame_counts(c["rows"]) + [1, len(oracles[-1].A)]
    for j in everything:
        assert np.array_equal(run([j], 0.0)[0], got[j]), j
    for o, g in zip(oracles, got):
        o.units(g)  # the logarithms: the hard bound
    linear = run(everything, 0.0, flags & ~hb.KALDI_USE_LOG)  # the yardstick: on the mel energies (audio_compare's docstring)
    units = np.concatenate([o.units_linear(e) for o, e in zip(oracles, linear)])
    emu = np.concatenate([o.units_linear(o.emulate_f32(log=False), enforce=False) for o in oracles])
    AC.stat_line("kaldi " + C.case_id(c), units, emu)
    noisy, again = run(everything, 1.0), run(everything, 1.0)
    for j in everything:
        assert np.array_equal(noisy[j], again[j]) and np.array_equal(run([j], 1.0)[0], noisy[j]), j
    assert not np.array_equal(noisy[0], got[0])
