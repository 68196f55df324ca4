"""float64 numpy oracle of include/fhvae_vad.h, written from the published semantics (librosa.feature.rms with centre padding by
reflection; Kaldi's snip-edges raw log energy; ComputeVadEnergy's threshold and context vote): np.pad, explicit frames, plain
sums.  It mirrors the header's storage rule: an energy is rounded once to float32, everything behind it is float64 again.
Besides the decisions it returns every frame's margin to its threshold, so that a test can show that no decision hangs on
the last bits of an energy."""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)


def signal(sr, n, seed=0):
    """Gaussian noise whose amplitude alternates between 0.3 and 0.003 every 0.1 s, float32."""
    rng = np.random.default_rng(seed)
    amp = np.where((np.arange(n) // int(0.1 * sr)) % 2 == 0, 0.3, 0.003)
    return (rng.standard_normal(n) * amp).astype(np.float32)


def rms_frames(n, L, hop):
    return 1 + (n + 2 * (L // 2) - L) // hop


def snip_frames(n, N, S):
    return 0 if n < N else 1 + (n - N) // S


def rms_energy64(y, L, hop):
    """librosa.feature.rms(y, frame_length=L, hop_length=hop, center=True, pad_mode="reflect") in float64, not yet rounded."""
    y = np.asarray(y, dtype=np.float64)
    assert len(y) >= L // 2 + 1
    p = np.pad(y, L // 2, mode="reflect")
    T = rms_frames(len(y), L, hop)
    return np.array([np.sqrt(np.mean(p[f * hop:f * hop + L] ** 2)) for f in range(T)])


def log_energy64(y, N, S, remove_dc):
    """Kaldi's raw log energy of the snip-edges frames of y (already on the int16 scale) in float64, not yet rounded."""
    y = np.asarray(y, dtype=np.float64)
    out = []
    for f in range(snip_frames(len(y), N, S)):
        x = y[f * S:f * S + N]
        if remove_dc:
            x = x - x.mean()
        out.append(np.log(max(np.sum(x * x), FLT_EPSILON)))
    return np.array(out)


def decide(e, thr_abs, mean_scale, ctx, proportion, relative):
    """One utterance: e (T,) energies as stored (they are rounded to float32 here) -> (vad bool (T,), margin (T,)): the
    margin of frame t is |e - th| / th (relative) or |e - th|."""
    e = np.asarray(e, dtype=np.float32).astype(np.float64)
    T = len(e)
    th = thr_abs + mean_scale * (e.sum() / T)
    a = e > th
    vad = np.zeros(T, dtype=bool)
    for t in range(T):
        lo, hi = max(t - ctx, 0), min(t + ctx, T - 1)
        num, den = int(a[lo:hi + 1].sum()), hi - lo + 1
        vad[t] = np.float32(num) >= np.float32(den) * np.float32(proportion)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.abs(e - th) / th if relative else np.abs(e - th)
    return vad, margin


def reference_vad(y, sr, win_t=0.025, hop_t=0.010, th_ratio=1.04 / 2):
    """AudioUtils.energy_vad of the reference (utils.py:275-300) -> (vad, relative margins, float32 energies)."""
    L, hop = int(sr * win_t), int(sr * hop_t)
    e = rms_energy64(y, L, hop).astype(np.float32)
    return decide(e, 0.0, th_ratio, 0, 1.0, relative=True) + (e,)


def kaldi_vad(y, N=400, S=160, remove_dc=True, thr_abs=5.0, mean_scale=0.5, ctx=0, proportion=0.6):
    """compute-vad-decision on the raw log energy of y (float32 at full scale 1.0) -> (vad, absolute margins, float32 energies)."""
    e = log_energy64(np.asarray(y, dtype=np.float32).astype(np.float64) * 32768.0, N, S, remove_dc).astype(np.float32)
    return decide(e, thr_abs, mean_scale, ctx, proportion, relative=False) + (e,)
