"""The sizes at which the audio kernels are run against their oracles, chosen so that every compiled row-tile height of every
file is selected by at least one case (tests/test_audio_tiles_cpu.py asserts that against the sources' TmSet<...> lists and
the library's *_tile_rows queries; tests/test_audio_tiles_gpu.py runs them).  A plain module, as tests/trellis_cases.py.

A row gives the sizes, the tile height `rows` the host must pick for them (0: the library refuses the size: the first size
past the last one that fits; such a row is only queried, never run) and how the size is reached: "real" rows are what the
command-line options give (16 kHz with --win-t 0.025 / 0.05 / 0.064 / 0.104 / 0.128, Kaldi's 25 ms frames at 8 to 44.1 kHz,
pairs of sample rates), "direct" rows call the C ABI through hip_binding with sizes no option produces.  For each height the
last size that fits and the first that does not are both rows.

Heights that no legal size reaches: none.  Every TmSet height of feats (fbank and spec), synth, kaldi_fbank and resample and
all four (TF, NT) of melinv have a row.  melinv's TF = 8 is legal at exactly one size, 1025 bins with 256 mels
(n_fft = 2048, --n-mels 256).  feats fbank stops at n_fft = 1664 (FHVAE_FEATS_MAX_NFFT_FBANK): 2048 is spec only.
"""
import numpy as np


def _row(rows, how="direct", **kw):
    return dict(kw, rows=rows, how=how)


def _feats(ftype, n_fft, rows, hop=160, n_mels=80, how="direct", sr=16000):
    return _row(rows, how, ftype=ftype, n_fft=n_fft, hop=hop, n_mels=n_mels, sr=sr)


FEATS = (
    # 16 kHz at --win-t 0.025, 0.05, 0.064, 0.104 (the largest fbank window), 0.128 (the largest window: spec only)
    [_feats("fbank", n, r, how="real") for n, r in ((400, 64), (800, 32), (1024, 16), (1664, 16))]
    + [_feats("spec", n, r, how="real") for n, r in ((400, 64), (800, 32), (1024, 32), (1664, 16), (2048, 16))]
    # the last size of each height and the first of the next (odd sizes among them)
    + [_feats("fbank", n, r) for n, r in ((415, 64), (416, 32), (831, 32), (832, 16), (1665, 0))]
    + [_feats("spec", n, r) for n, r in ((624, 64), (625, 32), (1248, 32), (1249, 16), (2049, 0))]
    # tiny windows: G = 1 (three waves idle in the DFT), NC = 1 (the prefetch branch of tile_product never fires) and 2, odd
    + [_feats(t, n, 64, hop=h) for t in ("fbank", "spec") for n, h in ((2, 1), (16, 5), (17, 6), (33, 11))]
    # mel counts below, across and just over a 16-group: the j < n_out tail and the zero-padded basis rows
    + [_feats("fbank", 400, 64, n_mels=m) for m in (1, 23, 40, 81)]
    # hop > n_fft: frames leave gaps
    + [_feats(t, 64, 64, hop=100) for t in ("fbank", "spec")]
)


def _synth(n_fft, rows, hop=160, how="direct"):
    return _row(rows, how, n_fft=n_fft, hop=hop)


SYNTH = (
    [_synth(n, r, how="real") for n, r in ((400, 64), (800, 32), (1024, 32), (1664, 16), (2048, 16))]
    # last / first sizes; 623, 1247 and 2047 are the odd n_fft of each height (one sample past the symmetric padding)
    + [_synth(n, r) for n, r in ((623, 64), (624, 32), (1247, 32), (1248, 16), (2047, 16), (2049, 0))]
    # hop == n_fft: one covering frame per sample; hop = 1: n_fft covering frames
    + [_synth(64, 64, hop=64), _synth(16, 64, hop=1), _synth(33, 64, hop=7)]
)


def _kaldi(N, S, P, rows, sr=16000, how="direct", n_mels=23):
    return _row(rows, how, N=N, S=S, P=P, sr=sr, n_mels=n_mels)


KALDI = (
    # 25 ms / 10 ms at 8, 16, 22.05, 32 and 44.1 kHz
    [_kaldi(200, 80, 256, 64, 8000, "real"), _kaldi(400, 160, 512, 48, 16000, "real"), _kaldi(551, 220, 1024, 32, 22050, "real"),
     _kaldi(800, 320, 1024, 16, 32000, "real"), _kaldi(1102, 441, 2048, 16, 44100, "real")]
    + [_kaldi(N, 160, P, r) for N, P, r in ((368, 512, 64), (369, 512, 48), (512, 512, 48), (513, 1024, 32), (736, 1024, 32),
                                            (737, 1024, 16), (1025, 2048, 16), (1504, 2048, 16), (1505, 2048, 0))]
    + [_kaldi(400, 160, 512, 48, n_mels=m) for m in (1, 40, 81)]
)

# resample: KP is a function of the pair of rates.  The first six are test_resample_cpu.PAIRS (run by test_resample_gpu.py);
# 48 -> 8 kHz is the pair that reaches 16 rows.  The KP rows are the last / first sizes, queried only.
RESAMPLE_PAIRS = [((44100, 16000), 32), ((22050, 16000), 32), ((48000, 16000), 32), ((8000, 16000), 64), ((16000, 22050), 64),
                  ((11025, 16000), 64), ((48000, 8000), 16)]
RESAMPLE_KP = [(608, 64), (624, 32), (1248, 32), (1264, 16), (2496, 16), (2512, 0)]
RESAMPLE_NEW = [(48000, 8000)]  # pairs test_audio_tiles_gpu.py runs itself

# melinv: (sr, win_t, n_mels) -> TF.  The first four are melinv_ref.CONFIGS at 25 ms (run by test_melinv_gpu.py).
MELINV = [_row(64, "real", sr=16000, win_t=0.025, n_mels=80), _row(64, "real", sr=16000, win_t=0.025, n_mels=40),
          _row(64, "real", sr=8000, win_t=0.025, n_mels=40), _row(32, "real", sr=22050, win_t=0.025, n_mels=80),
          _row(16, "real", sr=16000, win_t=0.128, n_mels=80), _row(8, "real", sr=16000, win_t=0.128, n_mels=256)]
MELINV_NEW = MELINV[4:]
MELINV_THREADS = {64: 512, 32: 256, 16: 256, 8: 256}
# (n_mels, n_bins) -> TF: last / first sizes, queried only
MELINV_EDGES = [(80, 240, 64), (80, 241, 32), (80, 560, 32), (80, 561, 16), (80, 1025, 16), (256, 1024, 16), (256, 1025, 8),
                (256, 1026, 0)]


def runnable(table):
    return [c for c in table if c["rows"]]


def case_id(c):
    return "-".join("%s%s" % (k[0] if k not in ("ftype", "how") else "", c[k]) for k in c if k not in ("rows", "how")) + "-r%d" % c["rows"]


# ------------------------------------------------------------------------------------------------------------ the batches
def speechlike(sr, n, seed):
    """n samples of test_feats_cpu.speechlike, float32."""
    from test_feats_cpu import speechlike as gen

    y = gen(sr, n / sr + 0.01, seed)[:n]
    assert len(y) == n and y.dtype == np.float32
    return y


def frame_counts(tile):
    """Utterance boundaries inside tiles and a part-empty last tile, at every height."""
    return [tile - 1, tile, tile + 1, 2 * tile + 3]


def feats_waves(c):
    """Six utterances: frame counts tile - 1, tile, tile + 1, 2 tile + 3, the shortest legal one (n_fft // 2 + 1 samples) and one
    with a block of exact zeros long enough for whole silent frames."""
    sr, n_fft, hop, tile = c["sr"], c["n_fft"], c["hop"], c["rows"]
    pad = n_fft // 2
    waves = []
    for j, nfr in enumerate(frame_counts(tile)):
        L = (nfr - 1) * hop + n_fft % 2 + hop // 2
        assert L >= pad + 1 and 1 + (L + 2 * pad - n_fft) // hop == nfr
        waves.append(speechlike(sr, L, 7 * n_fft + j))
    waves.append(speechlike(sr, pad + 1, 7 * n_fft + 5))
    lead, zeros = pad + 2 * hop, n_fft + 3 * hop  # (at least two frames lie wholly inside the zeros, pre-emphasis included)
    y = speechlike(sr, lead + zeros + 2 * hop + 1, 7 * n_fft + 6).copy()
    y[lead:lead + zeros] = 0.0
    waves.append(y)
    return waves


def synth_frames(c):
    """Frames per utterance: the four tile counts, the shortest legal utterance (2 frames) and one long enough to hold frames
    that lie wholly inside a block of n_fft + 2 hop exact zeros starting at sample hop."""
    return frame_counts(c["rows"]) + [2, -(-c["n_fft"] // c["hop"]) + 5]


def kaldi_waves(c):
    """As feats_waves on the int16 scale (integer-valued, with a DC offset); the shortest utterance is one frame."""
    N, S, tile = c["N"], c["S"], c["rows"]
    waves = []
    for j, nfr in enumerate(frame_counts(tile) + [1]):
        L = N + (nfr - 1) * S + (S // 2 if nfr > 1 else 0)
        waves.append(np.round(speechlike(c["sr"], L, 3 * N + j).astype(np.float64) * 20000.0 + 300.0).astype(np.float32))
    y = np.round(speechlike(c["sr"], 5 * N, 3 * N + 6).astype(np.float64) * 20000.0).astype(np.float32)
    y[N:4 * N] = 0.0
    waves.append(y)
    return waves


# ------------------------------------------------------------------------------------------------------------ the oracles
_ORACLES = {}


def feats_oracles(c):
    """One audio_compare.FeatsOracle per utterance of feats_waves(c), computed once per process."""
    import audio_compare as AC
    import features as F
    import feats_ref

    key = case_id(c)
    if key not in _ORACLES:
        n_fft, n_mels, fbank = c["n_fft"], c["n_mels"], c["ftype"] == "fbank"
        basis = F.dft_basis(n_fft)
        mel32 = F.mel_basis(c["sr"], n_fft, n_mels) if fbank else None
        mel64 = feats_ref.mel_bank(c["sr"], 2 * (n_fft // 2), n_mels) if fbank else None
        _ORACLES[key] = [AC.FeatsOracle(y, c["sr"], n_fft, c["hop"], n_mels, c["ftype"], basis, mel32, mel64) for y in feats_waves(c)]
    return _ORACLES[key]


def synth_oracles(c, sr=16000):
    """The inputs and audio_compare oracles of one synth case, computed once per process: the inverse STFT of S * random
    phases, one projection without tprev on that waveform (rounded to f32, so both sides start from the same numbers), the
    next round's projection with tprev = the first round's rebuilt, and the same with momentum 0."""
    import audio_compare as AC
    import features as F
    import synth_ref as R

    key = "synth-" + case_id(c)
    if key not in _ORACLES:
        n_fft, hop, frames = c["n_fft"], c["hop"], synth_frames(c)
        # (white noise at a tenth of the peak fills the weak bins: the direction of a bin inside 2 E is not compared, and the
        # bound grows with n_fft; with it the excluded share stays below the cap, test_audio_tiles_cpu.py)
        rng = np.random.default_rng(n_fft)
        ys = [(speechlike(sr, hop * (f - 1), 5 * n_fft + j) + 0.05 * rng.standard_normal(hop * (f - 1))).astype(np.float32)
              for j, f in enumerate(frames)]
        ys[-1][hop:hop + n_fft + 2 * hop] = 0.0
        dft, syn = F.dft_basis(n_fft), F.synth_basis(n_fft)
        S = np.abs(np.concatenate([R.stft(y, n_fft, hop, f) for y, f in zip(ys, frames)])).astype(np.float32).astype(np.float64)
        X0 = AC.unpack64(AC.pack32(S * R.unit_phases(n_fft, S.shape)))
        ist = AC.IstftOracle(X0, frames, n_fft, hop, syn)
        y1 = ist.y.astype(np.float32)
        coef = 0.99 / 1.99
        p1 = AC.ProjectOracle(y1, frames, n_fft, hop, S, None, coef, dft)
        tprev = AC.unpack64(AC.pack32(p1.re + 1j * p1.im))
        ist2 = AC.IstftOracle(AC.unpack64(AC.pack32(p1.next)), frames, n_fft, hop, syn)
        y2 = ist2.y.astype(np.float32)
        p2 = AC.ProjectOracle(y2, frames, n_fft, hop, S, tprev, coef, dft)
        p0 = AC.ProjectOracle(y2, frames, n_fft, hop, S, tprev, 0.0, dft)
        _ORACLES[key] = dict(frames=frames, S=S, X0=X0, ist=ist, y1=y1, y2=y2, tprev=tprev, coef=coef, p1=p1, p2=p2, p0=p0)
    return _ORACLES[key]


def kaldi_oracles(c):
    """One audio_compare.KaldiOracle per utterance of kaldi_waves(c) (dither 0, Kaldi's default options otherwise)."""
    import audio_compare as AC
    import features as F
    import kaldi_fbank_ref as R

    key = "kaldi-" + case_id(c)
    if key not in _ORACLES:
        N, S, P, sr, n_mels = c["N"], c["S"], c["P"], c["sr"], c["n_mels"]
        basis, mel32 = F.kaldi_dft_basis(N, P), F.kaldi_mel_basis(sr, P, n_mels)
        mel64, w = R.mel_bank(sr, P, n_mels), R.window(N, "povey")
        _ORACLES[key] = [AC.KaldiOracle(y, sr, N, S, P, n_mels, basis, mel32, mel64, w) for y in kaldi_waves(c)]
    return _ORACLES[key]
