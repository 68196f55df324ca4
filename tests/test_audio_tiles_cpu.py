"""What tests/test_audio_tiles_gpu.py rests on, checked without a GPU: the case tables of tests/audio_cases.py reach every
row-tile height the five audio files compile (read from the sources' TmSet<...> lists and melinv's launches, confirmed by the
library's *_tile_rows queries), the share of elements the log comparison leaves out stays within 1 % on the oracle alone,
and the comparator of tests/audio_compare.py rejects perturbed outputs of the kind a wrong tile height would produce."""
import os
import re

import numpy as np
import pytest

import audio_cases as C
import audio_compare as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-scalablefhvae_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    return hip_binding.load_library()  # loads without a GPU; the queries are host code


def compiled_heights(name):
    """16 * TM for the TMs of the file's `using ... = TmSet<...>;`."""
    src = open(os.path.join(CSRC, name)).read()
    sets = re.findall(r"using \w+ = TmSet<([0-9, ]+)>;", src)
    assert len(sets) == 1, (name, sets)
    return {16 * int(t) for t in sets[0].split(",")}


def queried(lib, kernel, c):
    import hip_binding as hb

    if kernel == "feats":
        return lib.fhvae_feats_tile_rows(c["n_fft"], hb.FEATS_TYPES[c["ftype"]])
    if kernel == "synth":
        return lib.fhvae_synth_tile_rows(c["n_fft"])
    return lib.fhvae_kaldi_fbank_tile_rows(c["N"], c["P"], c["n_mels"])


@pytest.mark.parametrize("kernel,source,table", [("feats", "feats.hip", C.FEATS), ("synth", "synth.hip", C.SYNTH),
                                                 ("kaldi", "kaldi_fbank.hip", C.KALDI)])
def test_every_compiled_height_has_a_case(lib, kernel, source, table):
    for c in table:
        assert queried(lib, kernel, c) == c["rows"], c
    heights = compiled_heights(source)
    groups = {"fbank": [c for c in table if c["ftype"] == "fbank"], "spec": [c for c in table if c["ftype"] == "spec"]} \
        if kernel == "feats" else {kernel: table}  # (kaldi: every dither-free case runs with dither as well)
    for what, rows in groups.items():
        assert {c["rows"] for c in C.runnable(rows)} == heights, (what, heights)
        # the last size of a height and the first of the next are both rows: sizes one apart with different heights
        size = "N" if kernel == "kaldi" else "n_fft"
        by_size = {(c.get("P"), c[size]): c["rows"] for c in rows}
        steps = {(a, by_size[(p, n + 1)]) for (p, n), a in by_size.items() if (p, n + 1) in by_size and by_size[(p, n + 1)] != a}
        if kernel == "kaldi":  # (48 -> 32 and 16 -> 16 cross a change of P: 512 | 513 and 1024 | 1025 are rows as well)
            assert {(64, 48), (32, 16), (16, 0)} <= steps and by_size[(512, 512)] == 48 and by_size[(1024, 513)] == 32, steps
        else:
            assert steps == {(64, 32), (32, 16), (16, 0)}, (what, steps)


def test_resample_heights(lib):
    import features as F
    from test_resample_cpu import PAIRS

    assert [p for p, _ in C.RESAMPLE_PAIRS[:len(PAIRS)]] == PAIRS
    for (sr_in, sr_out), rows in C.RESAMPLE_PAIRS:
        assert lib.fhvae_resample_tile_rows(F.resample_bank(sr_in, sr_out).KP) == rows, (sr_in, sr_out)
    for kp, rows in C.RESAMPLE_KP:
        assert lib.fhvae_resample_tile_rows(kp) == rows, kp
    assert {r for _, r in C.RESAMPLE_PAIRS} == compiled_heights("resample.hip")
    assert [r for _, r in C.RESAMPLE_KP] == [64, 32, 32, 16, 16, 0] and all(b - a == 16 for (a, _), (b, _) in zip(C.RESAMPLE_KP[::2], C.RESAMPLE_KP[1::2]))
    run_here = {dict(C.RESAMPLE_PAIRS)[p] for p in C.RESAMPLE_NEW}
    assert run_here | {r for p, r in C.RESAMPLE_PAIRS if p in PAIRS} == compiled_heights("resample.hip")


def test_melinv_heights(lib):
    import melinv_ref

    src = open(os.path.join(CSRC, "melinv.hip")).read()
    compiled = {(int(a), int(b)) for a, b in re.findall(r"melinv_launch<(\d+), (\d+)>\(", src)}
    assert compiled == set(C.MELINV_THREADS.items())
    assert [(c["sr"], c["n_mels"]) for c in C.MELINV[:4]] == melinv_ref.CONFIGS
    for c in C.MELINV:
        n_bins = int(c["sr"] * c["win_t"]) // 2 + 1
        assert lib.fhvae_mel_invert_tile_rows(c["n_mels"], n_bins) == c["rows"], c
    for n_mels, n_bins, rows in C.MELINV_EDGES:
        assert lib.fhvae_mel_invert_tile_rows(n_mels, n_bins) == rows, (n_mels, n_bins)
    assert {c["rows"] for c in C.MELINV} == {tf for tf, _ in compiled}
    assert {c["rows"] for c in C.MELINV_NEW} == {16, 8}  # what test_melinv_gpu.py's configurations do not reach


# ------------------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("c", C.runnable(C.FEATS), ids=C.case_id)
def test_feats_inputs_keep_the_excluded_share(c):
    """A condition on the inputs: on the oracle alone, at most 1 % of a case's elements lie inside 2 E, no element below the
    floor lies within E of it (so "must equal the floor" is implied by the bound), and the batch holds silent frames.  The
    float32 emulation's figures (the yardstick of the GPU test) are printed."""
    oracles = C.feats_oracles(c)
    excluded = sum(o.excluded_share()[0] for o in oracles)
    total = sum(o.lin.size for o in oracles)
    assert excluded <= AC.MAX_EXCLUDED * total, (excluded, total)
    for o in oracles:
        low = o.lin < np.exp(o.floor)
        assert np.all((o.lin + o.E)[low] < np.exp(o.floor))
    assert sum(int(o.silent.sum()) for o in oracles) >= 2
    units = np.concatenate([o.units(o.emulate_f32(), enforce=False) for o in oracles])
    print("%s: excluded %d of %d (%.4f %%), emulation max %.3f mean %.4f units over %d elements"
          % (C.case_id(c), excluded, total, 100.0 * excluded / total, units.max() if len(units) else 0.0,
             units.mean() if len(units) else 0.0, len(units)))


@pytest.mark.parametrize("c", C.runnable(C.SYNTH), ids=C.case_id)
def test_synth_inputs_keep_the_excluded_share(c):
    """On the oracle alone: the bins of fhvae_synth_project whose direction is not compared (|a| inside 2 Ea, S > 0) are at
    most 1 % of each of the three projections of a case; the batch holds silent frames."""
    o = C.synth_oracles(c)
    assert (o["S"] == 0).all(axis=1).any()
    for name in ("p1", "p2", "p0"):
        excluded, total = o[name].excluded()
        print("synth %s %s: excluded %d of %d (%.4f %%)" % (C.case_id(c), name, excluded, total, 100.0 * excluded / total))
        assert excluded <= AC.MAX_EXCLUDED * total, (name, excluded, total)


@pytest.mark.parametrize("c", C.runnable(C.KALDI), ids=C.case_id)
def test_kaldi_inputs_keep_the_excluded_share(c):
    """As test_feats_inputs_keep_the_excluded_share, for the Kaldi cases; the oracle of audio_compare.py agrees with
    tests/kaldi_fbank_ref.py where the sizes are those of a sample rate."""
    import kaldi_fbank_ref as R

    oracles = C.kaldi_oracles(c)
    excluded, total = sum(o.excluded_share()[0] for o in oracles), sum(o.lin.size for o in oracles)
    assert excluded <= AC.MAX_EXCLUDED * total, (excluded, total)
    for o in oracles:
        low = o.lin < np.exp(o.floor)
        assert np.all((o.lin + o.E)[low] < np.exp(o.floor))
    assert sum(int(o.silent.sum()) for o in oracles) >= 2
    if c["how"] == "real":
        assert R.sizes(c["sr"]) == (c["N"], c["S"], c["P"])
        want = R.fbank(C.kaldi_waves(c)[0], sr=c["sr"], n_mels=c["n_mels"])
        assert np.abs(want - np.log(np.maximum(oracles[0].lin, R.FLT_EPSILON))).max() < 1e-12
    units = np.concatenate([o.units_linear(o.emulate_f32(log=False), enforce=False) for o in oracles])
    print("kaldi %s: excluded %d of %d, emulation max %.3f mean %.4f units" % (C.case_id(c), excluded, total, units.max(), units.mean()))


# ------------------------------------------------------------------------------------------------------------ bite
def old_feats_check(got, want_log):
    """test_feats_gpu.check_against_oracle's tolerance -> whether it accepts."""
    err = np.abs(got.astype(np.float64) - want_log)
    ok = err <= 5e-4
    ok |= np.abs(np.exp(got.astype(np.float64)) - np.exp(want_log)) <= 1e-6 * np.exp(want_log).max(axis=1, keepdims=True)
    return bool(ok.all())


def _rejects(o, logs):
    try:
        o.units(logs.astype(np.float32))
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("ftype,n_mels", [("fbank", 81), ("spec", 80)])
def test_comparator_rejects_what_a_wrong_tile_would_compute(ftype, n_mels):
    """Three perturbed oracle outputs at a 32-row height (n_fft = 416 fbank / 625 spec), the utterance of 2 * 32 + 3 frames:
      1. the second 16-row tile of a workgroup reads the first tile's fragment (t = 1 gets t = 0's rows),
      2. one 16-sample chunk of the DFT chain is dropped,
      3. (fbank) a zero-padded mel row replaces the last real one, n_mels = 81.
    The new comparator rejects all of them (2 with the chunk at the window's edge, its smallest share, and in the middle).
    What the old 5e-4 / 1e-6-of-the-row's-largest check makes of each is printed: at these sizes it rejects them too.  What
    it cannot see is an error of a few hundred units in a weak bin; the yardstick of the GPU test (2 x the emulation) does."""
    c = dict(ftype=ftype, n_fft=416 if ftype == "fbank" else 625, hop=160, n_mels=n_mels, sr=16000, rows=32, how="direct")
    o = C.feats_oracles(c)[3]
    assert len(o.A) == 2 * 32 + 3

    def logs(c_, s_):
        with np.errstate(divide="ignore"):
            return np.maximum(np.log(o.finish(c_, s_)), o.floor)

    clean = logs(o.c, o.s)
    assert not _rejects(o, clean) and old_feats_check(clean.astype(np.float32), clean)
    seen = {}
    p1 = clean.copy()
    p1[16:32] = clean[0:16]
    seen["tile 1 reads tile 0"] = p1
    A = o.A.copy()
    A[:, 0:16] = 0.0  # the first chunk: under the Hamming window's edge, the smallest share of the sum
    seen["first chunk dropped"] = logs(A @ o.C64.T, A @ o.S64.T)
    A = o.A.copy()
    A[:, 192:208] = 0.0
    seen["middle chunk dropped"] = logs(A @ o.C64.T, A @ o.S64.T)
    if ftype == "fbank":
        p3 = clean.copy()
        p3[:, n_mels - 1] = o.floor
        seen["padded mel row in the last real one"] = p3
    old = {}
    for what, x in seen.items():
        assert _rejects(o, x), what
        old[what] = not old_feats_check(x.astype(np.float32), clean)
        print("%s %-36s new comparator rejects, old check %s" % (ftype, what, "rejects" if old[what] else "ACCEPTS"))
    assert all(old.values())
