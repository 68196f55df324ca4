"""kaldi_post.py -- the binding of include/fhvae_kaldi_post.h (csrc/kaldi_post.hip) and what stands on it: MFCC features,
delta features and sliding-window CMVN on the device, as Kaldi's compute-mfcc-feats, add-deltas and apply-cmvn-sliding
define them.  Nothing here runs a Kaldi binary; the definitions are the header's.

  kaldi_mfcc_options   the option set of compute-mfcc-feats from a config file or a dict
  dct_matrix, lifter_coeffs, delta_scales, cmvn_window
                       the host-side constants and the window rule (pure Python / numpy float64, rounded once)
  cepstra, add_deltas, cmvn_sliding
                       the three entry points on device tensors: (n, D) rows plus frame_ptr in, (n, D') out; they only
                       enqueue, so they chain without a download
  compute_kaldi_mfcc   waveforms in, MFCC matrices out (fhvae_kaldi_fbank_fwd with the conf's bank, then cepstra)
  compute_kaldi_feats  fbank or MFCC with deltas, sliding CMVN, VAD selection and compression behind them on the device
  post_process         deltas and / or CMVN of matrices that come from anywhere (an archive of z1, say)
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

import hip_ext

#: the bit of the int32 device status word and the limits (include/fhvae_kaldi_post.h, FHVAE_KPOST_*)
KPOST_BAD_PTR = 1
KPOST_MAX_BINS, KPOST_MAX_WINDOW, KPOST_MAX_COLS, KPOST_CHUNK = 128, 8, 1024, 256

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry points of include/fhvae_kaldi_post.h: name -> (restype, argtypes).  They are exported from libfhvae_hip.so but are
#: not part of include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
KPOST_SIGNATURES = {
    "fhvae_kaldi_cepstra": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, C.c_float, _vp, _vp]),
    "fhvae_kaldi_add_deltas": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "fhvae_kaldi_post_ws_bytes": (_i64, [_i64, _i64, _i64]),
    "fhvae_kaldi_cmvn_sliding": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, C.c_int, C.c_int, _vp, _i64, _vp, _vp, _vp]),
}

KPOST_WHAT = "fhvae_kaldi_add_deltas / fhvae_kaldi_cmvn_sliding: status %s (inconsistent frame_ptr)"


def load_library():
    """hip_binding.load_library() with the entry points above bound (argtypes from KPOST_SIGNATURES)."""
    return hip_ext.load(KPOST_SIGNATURES)


# ------------------------------------------------------------------------------------------------------------ host side
#: compute-mfcc-feats: the options it has on top of the frame and mel-bank options, with Kaldi's defaults
MFCC_DEFAULTS = {"num-ceps": 13, "cepstral-lifter": 22.0, "use-energy": True, "energy-floor": 0.0, "raw-energy": True,
                 "htk-compat": False}
#: options of compute-fbank-feats that compute-mfcc-feats does not have
MFCC_NOT_OPTIONS = ("use-log-fbank", "use-power")


def _read_conf(path):
    import features as F

    given = {}
    try:
        fh = open(path)
    except OSError as e:
        raise ValueError("%s: cannot read the Kaldi MFCC configuration (%s); expected a text file with %s"
                         % (path, e.strerror or e, F.KALDI_SYNTAX.replace("--num-mel-bins=80", "--num-ceps=13"))) from None
    with fh:
        for ln, raw in enumerate(fh, 1):
            line = raw.split("#", 1)[0].strip()
            if not line:
                continue
            if not line.startswith("--"):
                raise ValueError("%s:%d: %r is not an option; expected %s" % (path, ln, line, F.KALDI_SYNTAX))
            name, _, value = line[2:].partition("=")
            given[name.strip()] = value.strip()
    return given


def kaldi_mfcc_options(source=None):
    """The option set of Kaldi's compute-mfcc-feats from a config file (path) or a dict of option names (dashes, as Kaldi
    spells them) -> dict: every frame and mel-bank option of features.kaldi_fbank_options (which parses and checks them) plus
    num-ceps (13), cepstral-lifter (22), use-energy (true), energy-floor (0) and raw-energy (true); num-mel-bins defaults to
    23.  htk-compat=true, raw-energy=false, num-ceps above num-mel-bins and every option the fbank parser refuses raise
    ValueError naming the option and the file."""
    import features as F

    where = "options"
    if source is None:
        given = {}
    elif isinstance(source, dict):
        given = {str(k).lstrip("-").replace("_", "-"): v for k, v in source.items()}
    else:
        where = str(source)
        given = _read_conf(where)
    opts = dict(MFCC_DEFAULTS)
    bank = {}
    for name, value in given.items():
        if name in MFCC_NOT_OPTIONS:
            raise ValueError("%s: unknown option --%s (compute-mfcc-feats has none of that name)" % (where, name))
        if name not in MFCC_DEFAULTS:
            bank[name] = value
            continue
        kind = type(MFCC_DEFAULTS[name])
        try:
            if kind is bool:
                opts[name] = value if isinstance(value, bool) else F._kaldi_bool(value)
            elif kind is int:
                if not isinstance(value, str) and int(value) != value:
                    raise ValueError
                opts[name] = int(value)
            else:
                opts[name] = float(value)
        except (TypeError, ValueError):
            raise ValueError("%s: option --%s has the value %r, not a %s" % (where, name, value, kind.__name__)) from None
    try:
        fb = F.kaldi_fbank_options(bank)
    except ValueError as e:
        text = str(e)
        raise ValueError(where + text[len("options"):] if text.startswith("options") else text) from None
    if opts["htk-compat"]:
        raise ValueError("%s: option --htk-compat=true is not supported (only false is implemented)" % where)
    if not opts["raw-energy"]:
        raise ValueError("%s: option --raw-energy=false is not supported (only true is implemented)" % where)
    if not 1 <= opts["num-ceps"] <= fb["num-mel-bins"]:
        raise ValueError("%s: option --num-ceps=%d is outside [1, num-mel-bins = %d]" % (where, opts["num-ceps"], fb["num-mel-bins"]))
    if fb["num-mel-bins"] > KPOST_MAX_BINS:
        raise ValueError("%s: option --num-mel-bins=%d is above %d, the most the cepstra take" % (where, fb["num-mel-bins"], KPOST_MAX_BINS))
    if not (math.isfinite(opts["cepstral-lifter"]) and math.isfinite(opts["energy-floor"])):
        raise ValueError("%s: --cepstral-lifter and --energy-floor must be finite" % where)
    fb.update(opts)
    for name in MFCC_NOT_OPTIONS:  # (the result holds compute-mfcc-feats's options only: it can be given back to this function)
        del fb[name]
    return fb


def fbank_part(opts):
    """The options of kaldi_mfcc_options that features.compute_kaldi_fbank takes (the mel bank in front of the cepstra)."""
    import features as F

    fb = {k: v for k, v in opts.items() if k in F.KALDI_DEFAULTS}
    fb.update({"use-energy": False, "energy-floor": 0.0, "raw-energy": True, "htk-compat": False, "use-log-fbank": True, "use-power": True})
    return fb


def dct_matrix(num_ceps, num_bins):
    """Kaldi's ComputeDctMatrix, the first num_ceps rows: (num_ceps, num_bins) float32, computed in float64 and rounded once.
    Row 0 is sqrt(1 / B), row k is sqrt(2 / B) cos(pi / B (j + 0.5) k)."""
    B = int(num_bins)
    k = np.arange(int(num_ceps), dtype=np.float64)[:, None]
    j = np.arange(B, dtype=np.float64)[None, :]
    m = math.sqrt(2.0 / B) * np.cos(math.pi / B * (j + 0.5) * k)
    m[0, :] = math.sqrt(1.0 / B)
    return m.astype(np.float32)


def lifter_coeffs(num_ceps, Q):
    """Kaldi's ComputeLifterCoeffs: (num_ceps,) float32, 1 + 0.5 Q sin(pi k / Q), computed in float64 and rounded once."""
    k = np.arange(int(num_ceps), dtype=np.float64)
    return (1.0 + 0.5 * float(Q) * np.sin(math.pi * k / float(Q))).astype(np.float32)


def delta_scales(order, window):
    """The scale vectors of Kaldi's DeltaFeatures: [scales_0, .., scales_order], scales_i (2 i window + 1,) float32;
    scales_0 = [1], scales_i = (1 / sum j^2) * the full convolution of scales_{i-1} with [-window .. window]; float64,
    rounded once."""
    order, window = int(order), int(window)
    if order < 0 or window < 1:
        raise ValueError("delta order %d / window %d: the order must be >= 0 and the window >= 1" % (order, window))
    out = [np.ones(1, dtype=np.float64)]
    norm = float(sum(j * j for j in range(-window, window + 1)))
    for _ in range(order):
        prev = out[-1]
        cur = np.zeros(len(prev) + 2 * window, dtype=np.float64)
        for j in range(-window, window + 1):
            for k in range(len(prev)):
                cur[j + window + k] += j * prev[k]
        out.append(cur * (1.0 / norm))
    return [s.astype(np.float32) for s in out]


def cmvn_window(t, T, cmn_window=600, min_window=100, center=False):
    """The window [b, e) of frame t of an utterance of T frames under Kaldi's SlidingWindowCmn (include/fhvae_kaldi_post.h)."""
    if center:
        b = t - cmn_window // 2
        e = b + cmn_window
    else:
        b = t - cmn_window
        e = t + 1
    if b < 0:
        e -= b
        b = 0
    if not center and e > t:
        e = max(t + 1, min_window)
    if e > T:
        b -= e - T
        e = T
        b = max(b, 0)
    return b, e


def check_deltas(order, window, D=None):
    if order not in (1, 2):
        raise ValueError("--delta-order %r is not 1 or 2" % (order,))
    if not 1 <= window <= KPOST_MAX_WINDOW:
        raise ValueError("--delta-window %r is outside [1, %d]" % (window, KPOST_MAX_WINDOW))
    if D is not None and (order + 1) * D > KPOST_MAX_COLS:
        raise ValueError("%d columns with deltas of order %d are more than %d" % (D, order, KPOST_MAX_COLS))


def check_cmvn(cmn_window, min_window, D=None):
    if not 1 <= cmn_window < 1 << 31:
        raise ValueError("--cmn-window %r is outside [1, 2^31)" % (cmn_window,))
    if not 1 <= min_window < 1 << 31:
        raise ValueError("--cmn-min-window %r is outside [1, 2^31)" % (min_window,))
    if D is not None and D > KPOST_MAX_COLS:
        raise ValueError("%d columns are more than %d" % (D, KPOST_MAX_COLS))


def deltas_spec(order=2, window=2):
    check_deltas(order, window)
    return {"order": int(order), "window": int(window)}


def cmvn_spec(cmn_window=300, min_window=100, center=True, norm_vars=False):
    check_cmvn(cmn_window, min_window)
    return {"cmn_window": int(cmn_window), "min_window": int(min_window), "center": bool(center), "norm_vars": bool(norm_vars)}


# ------------------------------------------------------------------------------------------------------ device batches
def _check_status(status):
    """(KPOST_WHAT is the wording of features._download's status errors, which the batches below also raise through)"""
    st = int(status.cpu().item())
    if st:
        raise RuntimeError(KPOST_WHAT % st)


def cepstra(logmel, dct, lifter=None, energy=None, log_energy_floor=-math.inf):
    """fhvae_kaldi_cepstra: logmel (n, B) f32 (rows may be strided), dct (C, B), lifter (C,) or None, energy (n,) or None, all
    on the device -> (n, C) f32."""
    import torch

    import hip_binding as hb

    load_library()
    hb._need_gpu(logmel, dct, lifter, energy)
    op = "kaldi_cepstra"
    if logmel.dim() != 2 or logmel.dtype != torch.float32 or (logmel.shape[0] > 1 and logmel.stride(1) != 1) or (
            logmel.shape[0] > 1 and logmel.stride(0) < logmel.shape[1]):
        raise RuntimeError("%s: logmel must be a 2-D torch.float32 tensor with unit column stride (got %s %s, strides %s)"
                           % (op, logmel.dtype, tuple(logmel.shape), logmel.stride()))
    n, B = int(logmel.shape[0]), int(logmel.shape[1])
    ld = int(logmel.stride(0)) if n > 1 else B
    if n == 1 and not logmel.is_contiguous():
        logmel = logmel.contiguous()
    hb._want(op, "dct", dct, torch.float32, shape=(None, B))
    Cn = int(dct.shape[0])
    hb._want(op, "lifter", lifter, torch.float32, shape=(Cn,), optional=True)
    hb._want(op, "energy", energy, torch.float32, shape=(n,), optional=True)
    out = torch.empty((n, Cn), dtype=torch.float32, device=logmel.device)
    hb._call("fhvae_kaldi_cepstra", hb._p(logmel), ld, n, B, hb._p(dct), Cn, hb._p(lifter), hb._p(energy), float(log_energy_floor),
             hb._p(out))
    return out


_scales_cache = {}


def _scales_dev(order, window, device):
    import torch

    key = (order, window, str(device))
    if key not in _scales_cache:
        _scales_cache[key] = torch.from_numpy(np.concatenate(delta_scales(order, window))).to(device)
    return _scales_cache[key]


def add_deltas(x, frame_ptr, order=2, window=2, status=None):
    """fhvae_kaldi_add_deltas: x (n, D) f32 and frame_ptr (U + 1,) int64 on the device -> (n, (order + 1) D) f32.  `status`:
    the (1,) int32 device word the caller checks later; None: one is made and checked here (which synchronises)."""
    import torch

    import hip_binding as hb

    load_library()
    own = status is None
    status = hip_ext.status_word(x.device) if own else status
    hb._need_gpu(x, frame_ptr, status)
    op = "kaldi_add_deltas"
    hb._want(op, "x", x, torch.float32, ndim=2)
    hb._want(op, "frame_ptr", frame_ptr, torch.int64, ndim=1)
    hb._want(op, "status", status, torch.int32, numel=1, contiguous=False)
    n, D = int(x.shape[0]), int(x.shape[1])
    check_deltas(order, window, D)
    out = torch.empty((n, (order + 1) * D), dtype=torch.float32, device=x.device)
    hb._call("fhvae_kaldi_add_deltas", hb._p(x), hb._p(frame_ptr), int(frame_ptr.shape[0]) - 1, n, D, int(order), int(window),
             hb._p(_scales_dev(int(order), int(window), x.device)), hb._p(out), hb._p(status))
    if own:
        _check_status(status)
    return out


def cmvn_sliding(x, frame_ptr, cmn_window=600, min_window=100, center=False, norm_vars=False, status=None):
    """fhvae_kaldi_cmvn_sliding: x (n, D) f32 and frame_ptr (U + 1,) int64 on the device -> (n, D) f32.  The defaults are
    apply-cmvn-sliding's.  The workspace is allocated here.  `status` as in add_deltas."""
    import torch

    import hip_binding as hb

    lib = load_library()
    own = status is None
    status = hip_ext.status_word(x.device) if own else status
    hb._need_gpu(x, frame_ptr, status)
    op = "kaldi_cmvn_sliding"
    hb._want(op, "x", x, torch.float32, ndim=2)
    hb._want(op, "frame_ptr", frame_ptr, torch.int64, ndim=1)
    hb._want(op, "status", status, torch.int32, numel=1, contiguous=False)
    n, D, U = int(x.shape[0]), int(x.shape[1]), int(frame_ptr.shape[0]) - 1
    check_cmvn(cmn_window, min_window, D)
    nbytes = int(lib.fhvae_kaldi_post_ws_bytes(n, U, D))
    if nbytes < 0:
        raise ValueError("fhvae_kaldi_post_ws_bytes(%d, %d, %d) = %d" % (n, U, D, nbytes))
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=x.device)
    out = torch.empty((n, D), dtype=torch.float32, device=x.device)
    hb._call("fhvae_kaldi_cmvn_sliding", hb._p(x), hb._p(frame_ptr), U, n, D, int(cmn_window), int(min_window), int(bool(center)),
             int(bool(norm_vars)), hb._p(ws), nbytes, hb._p(out), hb._p(status))
    if own:
        _check_status(status)
    return out


def apply_post(x, frame_ptr, deltas=None, cmvn=None, status=None):
    """Kaldi's recipe order on the device: add_deltas (`deltas`, a deltas_spec) then cmvn_sliding (`cmvn`, a cmvn_spec)."""
    if deltas is not None:
        x = add_deltas(x, frame_ptr, deltas["order"], deltas["window"], status)
    if cmvn is not None:
        x = cmvn_sliding(x, frame_ptr, cmvn["cmn_window"], cmvn["min_window"], cmvn["center"], cmvn["norm_vars"], status)
    return x


class _MfccConsts:
    """Device copies of the DCT matrix and the lifter for one option set."""

    def __init__(self, opts, device):
        import torch

        Cn, B, Q = opts["num-ceps"], opts["num-mel-bins"], opts["cepstral-lifter"]
        self.dct = torch.from_numpy(dct_matrix(Cn, B)).to(device)
        self.lifter = torch.from_numpy(lifter_coeffs(Cn, Q)).to(device) if Q != 0.0 else None
        self.floor = math.log(opts["energy-floor"]) if opts["energy-floor"] > 0.0 else -math.inf


def _feats_batch(hb, waves, ids, fb, mfcc, sizes, seed, bases, consts, device, compress, names, vad, deltas, cmvn):
    """One batch of compute_kaldi_feats: the log-mel rows (fhvae_kaldi_fbank_fwd), the cepstra (`mfcc`: the MFCC options or
    None), deltas, CMVN, then the VAD's row selection, the compression and the download, as features._kaldi_batch ends."""
    import torch

    import features as F
    import vad as V

    N, S, P = sizes
    n_mels = fb["num-mel-bins"]
    lens = np.array([len(w) for w in waves], dtype=np.int64)
    frame_ptr = F._ptr(F.kaldi_num_frames(lens, N, S))
    n = int(frame_ptr[-1])
    wave_d = F._upload(waves, device, scale=32768.0)
    ptrs_d = F._upload_ptrs([F._ptr(lens), frame_ptr], device)
    dither = float(fb["dither"])
    ids_d = torch.from_numpy(np.asarray(ids, dtype=np.uint64).view(np.int64).copy()).to(device) if dither != 0.0 else None
    x = torch.empty((n, n_mels), dtype=torch.float32, device=device)
    status, vstatus, kstatus = hip_ext.status_word(device), hip_ext.status_word(device), hip_ext.status_word(device)
    flags = (hb.KALDI_REMOVE_DC if fb["remove-dc-offset"] else 0) | hb.KALDI_USE_LOG | hb.KALDI_USE_POWER if mfcc is not None else (
        (hb.KALDI_REMOVE_DC if fb["remove-dc-offset"] else 0) | (hb.KALDI_USE_LOG if fb["use-log-fbank"] else 0)
        | (hb.KALDI_USE_POWER if fb["use-power"] else 0))
    hb.kaldi_fbank_fwd(wave_d, ptrs_d[0], ptrs_d[1], ids_d, bases.dft, bases.mel, N, S, P, n_mels, fb["preemphasis-coefficient"],
                       dither, seed, flags, x, status)
    if mfcc is not None:
        energy = None
        if mfcc["use-energy"]:  # the raw log energy of the frame as it is read: no dither, no pre-emphasis, no window
            energy = V.energy(wave_d, ptrs_d[0], ptrs_d[1], n, N, S, V.VAD_LOGE_SNIP, V.VAD_REMOVE_DC if fb["remove-dc-offset"] else 0,
                              vstatus)
        x = cepstra(x, consts.dct, consts.lifter, energy, consts.floor)
    x = apply_post(x, ptrs_d[1], deltas, cmvn, kstatus)
    statuses = (status, vstatus, kstatus)
    what = "fhvae_kaldi_fbank_fwd / fhvae_vad_energy / fhvae_kaldi_post: status %s (inconsistent wave_ptr / frame_ptr)"
    if vad is not None:
        return F._vad_finish(wave_d, ptrs_d, frame_ptr, x, vad, statuses, what, compress, names)
    if compress is None:
        return F._download(x, statuses, what, frame_ptr)
    st = tuple(int(s.cpu().item()) for s in statuses)
    if any(st):
        raise RuntimeError(what % (st,))
    return F.kaldi_compress(x, np.diff(frame_ptr), compress, names)


def compute_kaldi_feats(waves, opts=None, kind="mfcc", seed=0, stream_ids=None, names=None, device="cuda", max_samples=None,
                        rates=None, compress=None, vad=None, deltas=None, cmvn=None):
    """features.compute_kaldi_fbank with the steps of this module behind the mel bank, all on the device: `kind` "fbank"
    (`opts`: what features.kaldi_fbank_options takes) or "mfcc" (`opts`: what kaldi_mfcc_options takes; with use-energy C0 is
    the raw log energy of fhvae_vad_energy's FHVAE_VAD_LOGE_SNIP mode, remove-dc-offset as the conf says, no dither on the
    energy), then `deltas` (a deltas_spec), `cmvn` (a cmvn_spec), the VAD's row selection (`vad`, as compute_kaldi_fbank) and
    the compression (`compress`), in that order.  Every other argument and the result are compute_kaldi_fbank's."""
    import features as F

    if kind not in ("fbank", "mfcc"):
        raise ValueError("kind must be fbank or mfcc, got %r" % (kind,))
    if compress is not None:
        import kaldi_io_lite

        kaldi_io_lite.token_for(1, compress)
    mfcc = kaldi_mfcc_options(opts) if kind == "mfcc" else None
    fb = fbank_part(mfcc) if mfcc is not None else F.kaldi_fbank_options(opts)
    sizes = F.check_kaldi_options(fb)
    sr = fb["sample-frequency"]
    if sr != int(sr):
        raise ValueError("sample-frequency %r is not a whole number of Hz" % (sr,))
    F.kaldi_mel_filters(sr, sizes[2], fb["num-mel-bins"], fb["low-freq"], fb["high-freq"])  # (bad band edges fail here)
    D = mfcc["num-ceps"] if mfcc is not None else fb["num-mel-bins"]
    if deltas is not None:
        check_deltas(deltas["order"], deltas["window"], D)
        D *= deltas["order"] + 1
    if cmvn is not None:
        check_cmvn(cmvn["cmn_window"], cmvn["min_window"], D)
    max_samples = F.BATCH_SAMPLES if max_samples is None else max_samples
    waves = [np.ascontiguousarray(w, dtype=np.float32).reshape(-1) for w in waves]
    names = list(names) if names is not None else ["utterance %d" % j for j in range(len(waves))]
    ids = list(range(len(waves))) if stream_ids is None else [int(v) & 0xFFFFFFFFFFFFFFFF for v in stream_ids]
    if len(ids) != len(waves) or len(names) != len(waves):
        raise ValueError("stream_ids / names must have one entry per waveform (%d)" % len(waves))
    if rates is not None:
        groups = {r: idx for r, idx in F._rate_groups(rates, len(waves)).items() if r != int(sr)}
        for r in groups:
            F.resample_bank(r, int(sr))  # (an unsupported ratio fails before any work)
        for r, idx in groups.items():
            for j, y in zip(idx, F.resample([waves[j] for j in idx], r, int(sr), device, max_samples)):
                waves[j] = y
    for j, w in enumerate(waves):
        if len(w) < sizes[0]:
            raise ValueError("%s: %d samples%s; one frame needs %d (Kaldi would skip the utterance)"
                             % (names[j], len(w), " after resampling" if rates is not None else "", sizes[0]))
    spec = F._vad_spec_kaldi(vad, fb, sizes) if vad is not None else None
    if not waves:
        return [] if vad is None else ([], [])
    import hip_binding as hb

    bases = F._KaldiBases(fb, sizes[0], sizes[2], device)
    consts = _MfccConsts(mfcc, device) if mfcc is not None else None
    out, vads = [], []
    for a, b in F.batches([len(w) for w in waves], max_samples):
        got = _feats_batch(hb, waves[a:b], ids[a:b], fb, mfcc, sizes, int(seed), bases, consts, device, compress, names[a:b], spec,
                           deltas, cmvn)
        if vad is not None:
            vads.extend(got[1])
            got = got[0]
        out.extend(got)
    return out if vad is None else (out, vads)


def compute_kaldi_mfcc(waves, opts=None, seed=0, stream_ids=None, names=None, device="cuda", max_samples=None, rates=None,
                       deltas=None, cmvn=None):
    """compute-mfcc-feats for every waveform (float32 1-D arrays at full scale 1.0, at the sample-frequency of `opts`, what
    kaldi_mfcc_options takes) -> list of float32 (nframes, num-ceps), in input order: compute_kaldi_feats with kind "mfcc"."""
    return compute_kaldi_feats(waves, opts, "mfcc", seed, stream_ids, names, device, max_samples, rates, None, None, deltas, cmvn)


def post_process(mats, deltas=None, cmvn=None, device="cuda", max_frames=1 << 20, compress=None, names=None):
    """Deltas and / or sliding CMVN of matrices that come from anywhere (a list of (T_j, D) arrays with one D) -> a list of
    float32 (T_j, D') arrays, or with `compress` of kaldi_io_lite.CompressedMatrix; batches of at most `max_frames` rows."""
    import torch

    import features as F

    mats = [np.ascontiguousarray(m, dtype=np.float32) for m in mats]
    if not mats:
        return []
    D = mats[0].shape[1] if mats[0].ndim == 2 else -1
    for j, m in enumerate(mats):
        if m.ndim != 2 or m.shape[1] != D or m.shape[0] < 1:
            raise ValueError("%s: a matrix of shape %s; expected at least one row of %d columns"
                             % (names[j] if names is not None else "matrix %d" % j, m.shape, D))
    if deltas is not None:
        check_deltas(deltas["order"], deltas["window"], D)
    if cmvn is not None:
        check_cmvn(cmvn["cmn_window"], cmvn["min_window"], D * ((deltas["order"] + 1) if deltas is not None else 1))
    out = []
    for a, b in F.batches([len(m) for m in mats], max_frames):
        frame_ptr = F._ptr([len(m) for m in mats[a:b]])
        x = F._upload(mats[a:b], device)
        ptr_d = torch.from_numpy(frame_ptr).to(device)
        status = hip_ext.status_word(device)
        x = apply_post(x, ptr_d, deltas, cmvn, status)
        if compress is None:
            out.extend(F._download(x, (status,), KPOST_WHAT, frame_ptr))
        else:
            _check_status(status)
            out.extend(F.kaldi_compress(x, np.diff(frame_ptr), compress, names[a:b] if names is not None else None))
    return out
