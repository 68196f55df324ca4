"""features.py -- log-mel (fbank) and log-magnitude (spec) features from PCM WAV files on the MI355X.

The reference computes them per file on the CPU with librosa 0.8.0 (prepare_numpy_data.generate_feat, :14-46, on
AudioUtils.stft / rstft / to_melspec, utils.py:155-272).  Here the arithmetic runs in one launch per batch of utterances
(fhvae_feats_fwd, csrc/feats.hip); this module holds the host side:

  read_wav            RIFF WAV, integer PCM (8-bit unsigned, 16, 24, 32-bit) -> float32 mono, scaled like soundfile
                      (int16 / 2**15, int24 / 2**23, int32 / 2**31, (u8 - 128) / 128); channels averaged.  No resampling here.
  decode_flac         native FLAC files (bytes) -> int32 (n, channels) samples, decoded on the device (csrc/flac.hip: fhvae_flac_scan
                      finds the frame headers, fhvae_flac_decode parses and decodes the frames; the container is flac_lite.py)
  read_sphere         NIST SPHERE (TIMIT's .WAV), uncompressed PCM -> float32 mono like read_wav
  read_audio / read_audio_batch
                      any of the three by its first bytes (RIFF, fLaC, NIST_1A); the batch decodes all its FLAC files together
  frame_sizes         n_fft = win_length = int(sr * win_t), hop = int(sr * hop_t) (the reference's truncation)
  dft_basis           windowed cos / -sin columns (periodic Hamming), built in float64, rounded to f32, padded for the kernel
  mel_filters         librosa.filters.mel(sr, n_fft', n_mels, fmin=0, fmax=sr/2, htk=False, norm='slaney') in float64, with
                      n_fft' = 2 * (n_bins - 1): melspectrogram(S=...) recovers n_fft from S's row count (odd n_fft differs)
  compute_features    a list of waveforms -> a list of (nframes, n_out) float32 arrays, batched into bounded launches
  resample_filter / resample_bank / resampled_length / resample
                      librosa.load's sample-rate conversion (resampy kaiser_best): the filter and the polyphase bank of a
                      pair of rates on the host in float64, the conversion itself on the device (csrc/resample.hip);
                      compute_features(..., rates=...) converts on the way to the features

and the way back for "spec" features (csrc/synth.hip: fhvae_synth_istft / _project / _deemph):

  synth_basis         window * irfft weights per output sample, (re, im) interleaved along the bins, float64 -> f32, padded
  window_sq           the squared window the overlap-add is normalised with
  synthesize          a list of (nframes, n_fft // 2 + 1) log-magnitude spectrograms -> a list of float32 waveforms by
                      Griffin-Lim (librosa 0.8.0 griffinlim semantics) and de-emphasis, batched into bounded launches
  write_wav           float32 mono -> 16-bit PCM WAV (the inverse of read_wav)

and for "fbank" features the step in front of it (csrc/melinv.hip: fhvae_mel_invert):

  MelBand             the mel bank in band form (a bin in at most two adjacent filters, a filter one run of bins)
  nnls_constants      1 / L and the momentum table of FISTA on ||A x - m||^2, in float64
  mel_to_spec         a list of (nframes, n_mels) log-mel features -> a list of (nframes, n_fft // 2 + 1) log-magnitude
                      spectrograms: non-negative least squares against mel_filters, a fixed number of FISTA steps from zero
  synthesize_mel      mel_to_spec, then synthesize on the device buffer

and Kaldi's filterbank features (csrc/kaldi_fbank.hip: fhvae_kaldi_fbank_fwd), numerically a different feature from "fbank":

  kaldi_fbank_options a Kaldi config file ("--name=value" lines) or a dict -> the full option set, Kaldi's defaults filled in
  kaldi_frame_sizes / kaldi_num_frames
                      N = int(sr * 0.001 * frame-length), S likewise, P = the power of two >= N; snip-edges frame count
  kaldi_window / kaldi_mel_filters / kaldi_dft_basis / kaldi_mel_basis
                      the symmetric window, the HTK mel triangles over bins 0 .. P/2 - 1 and the kernel's padded bases
  compute_kaldi_fbank a list of waveforms -> a list of (nframes, num-mel-bins) float32 arrays (dither by Philox, reproducible)

and energy voice-activity detection (csrc/vad.hip, include/fhvae_vad.h; the binding is vad.py):

  energy_vad          the reference's AudioUtils.energy_vad (utils.py:275-300): centred RMS per frame, voiced above th_ratio times
                      the utterance's mean -> one bool array per waveform
  kaldi_vad_options   a Kaldi config file of the four --vad-* options or a dict -> the full option set
  kaldi_energy_vad    compute-vad-decision on Kaldi's raw log energy (snip-edges frames, no dither)
  vad_decide          the decision alone, on energies that come from anywhere
  compute_features / compute_kaldi_fbank (..., vad=...) return (features, decisions) from the waveform already on the device,
                      with drop=True only the voiced rows (selected on the device, in front of the download / the compression)

Utterances shorter than n_fft // 2 + 1 samples are an error (one reflection of the centre padding must suffice; numpy's
repeated reflection for shorter inputs is not reproduced).
"""
from __future__ import annotations

import wave as _wave

import numpy as np

FTYPES = ("fbank", "spec")
LOG_FLOOR = {"fbank": -20.0, "spec": -50.0}  # utils.py:233 / :199
MAX_NFFT = 2048  # FHVAE_FEATS_MAX_NFFT
MAX_NMELS = 256  # FHVAE_FEATS_MAX_NMELS
BATCH_SAMPLES = 1 << 24  # samples per launch (about 17 minutes at 16 kHz)
BATCH_FRAMES = 1 << 17  # frames per synthesis batch (about 22 minutes at a 10 ms hop; about 8 KB of device memory per frame)


# ---------------------------------------------------------------------------------------------------------- audio input
def read_wav(path, channel=None):
    """-> (samples float32 (n,), sample rate).  Integer PCM only; anything else raises ValueError naming the file.
    `channel`: take that channel of a multi-channel file instead of the channel mean (Kaldi reads channel 0)."""
    try:
        with _wave.open(str(path), "rb") as w:
            nch, width, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
            raw = w.readframes(n)
    except (_wave.Error, EOFError) as e:  # not RIFF, or a format the wave module does not read (float, extensible, ...)
        raise ValueError("%s: not a PCM WAV file (%s)" % (path, e)) from None
    if width not in (1, 2, 3, 4) or nch < 1:
        raise ValueError("%s: unsupported sample width %d bytes" % (path, width))
    n = len(raw) // (width * nch)
    b = np.frombuffer(raw, dtype=np.uint8, count=n * width * nch)
    if width == 1:
        x = (b.astype(np.float32) - 128.0) / 128.0
    elif width == 2:
        x = b.view("<i2").astype(np.float32) / 32768.0
    elif width == 3:
        t = b.reshape(-1, 3).astype(np.int32)
        v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) / float(1 << 23)
    else:
        x = b.view("<i4").astype(np.float32) / float(1 << 31)
    x = x.reshape(n, nch)
    if channel is not None and not 0 <= channel < nch:
        raise ValueError("%s: no channel %d in a file of %d channel(s)" % (path, channel, nch))
    y = x[:, channel or 0] if nch == 1 or channel is not None else x.mean(axis=1, dtype=np.float32)
    return np.ascontiguousarray(y, dtype=np.float32), sr


def pcm_to_float(v, bps, channel=None, where="audio"):
    """The integer -> float32 mono step shared by the FLAC and SPHERE readers, in read_wav's expressions: `v` (n, channels)
    integers of `bps` bits -> v / 2**(bps - 1) in float32, then the float32 channel mean, or channel `channel`.  The same
    samples therefore give the same waveform bit for bit whichever container held them."""
    n, nch = v.shape
    x = v.astype(np.float32) / float(1 << (bps - 1))
    if channel is not None and not 0 <= channel < nch:
        raise ValueError("%s: no channel %d in a file of %d channel(s)" % (where, channel, nch))
    y = x[:, channel or 0] if nch == 1 or channel is not None else x.mean(axis=1, dtype=np.float32)
    return np.ascontiguousarray(y, dtype=np.float32)


SPHERE_MAGIC = b"NIST_1A\n"
AUDIO_MAGICS = "RIFF (WAV), fLaC (FLAC) or NIST_1A (SPHERE)"


def _sphere_samples(raw, path):
    """(int (n, channels) samples, sample rate, bits) of a SPHERE file's bytes."""
    try:
        size = int(raw[8:16].split()[0])
        lines = raw[16:size].decode("ascii", "replace").split("\n")
    except (ValueError, IndexError):
        raise ValueError("%s: malformed SPHERE header (no header size after NIST_1A)" % path) from None
    if size < 16 or size > len(raw):
        raise ValueError("%s: SPHERE header of %d bytes in a file of %d" % (path, size, len(raw)))
    fields, ended = {}, False
    for line in lines:
        line = line.strip()
        if line == "end_head":
            ended = True
            break
        parts = line.split(None, 2)
        if len(parts) == 3 and parts[1].startswith("-") and not line.startswith(";"):
            fields[parts[0]] = parts[2]
    if not ended:
        raise ValueError("%s: SPHERE header without end_head" % path)
    coding = fields.get("sample_coding", "pcm")
    if coding != "pcm":
        raise ValueError("%s: SPHERE sample_coding %s is not supported (only uncompressed pcm; decode shorten / wavpack / ulaw files "
                         "with sph2pipe first)" % (path, coding))
    try:
        sr, nch, width = int(fields["sample_rate"]), int(fields.get("channel_count", 1)), int(fields["sample_n_bytes"])
        n = int(fields["sample_count"])
    except KeyError as e:
        raise ValueError("%s: SPHERE header lacks %s" % (path, e.args[0])) from None
    order = fields.get("sample_byte_format", "1" if width == 1 else None)
    want = {1: ("1",), 2: ("01", "10")}.get(width)
    if want is None or nch < 1:
        raise ValueError("%s: unsupported SPHERE sample_n_bytes %d (1 or 2) or channel_count %d" % (path, width, nch))
    if order not in want:
        raise ValueError("%s: SPHERE sample_byte_format %r for %d-byte samples (expected %s)" % (path, order, width, " or ".join(want)))
    if size + n * nch * width > len(raw):
        raise ValueError("%s: truncated: %d samples of %d channel(s) need %d bytes behind the header, the file has %d"
                         % (path, n, nch, n * nch * width, len(raw) - size))
    dt = np.int8 if width == 1 else np.dtype("<i2" if order == "01" else ">i2")
    v = np.frombuffer(raw, dtype=dt, count=n * nch, offset=size).reshape(n, nch)
    return v, sr, 8 * width


def read_sphere(path, channel=None):
    """NIST SPHERE (what TIMIT's .WAV files are) -> (samples float32 (n,), sample rate), scaled and mixed like read_wav.
    Uncompressed PCM of 1 or 2 bytes in either byte order; shorten / wavpack compressed files and ulaw are refused by name."""
    with open(str(path), "rb") as fh:
        raw = fh.read()
    if raw[:8] != SPHERE_MAGIC:
        raise ValueError("%s: not a SPHERE file (no NIST_1A header)" % path)
    v, sr, bps = _sphere_samples(raw, path)
    return pcm_to_float(v, bps, channel, path), sr


def _flac_md5(x, bps):
    import hashlib

    width = (bps + 7) // 8
    if width == 3:
        raw = np.ascontiguousarray(x.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    else:
        raw = x.astype({1: "<i1", 2: "<i2", 4: "<i4"}[width]).tobytes()
    return hashlib.md5(raw).digest()


def _flac_batch(hb, blobs, infos, names, device, verify_md5):
    """decode_flac for files that fit one pair of buffers: scan, parse every candidate, walk the chains on the host, decode the
    chains' frames."""
    import torch

    U = len(blobs)
    lens = [len(b) - i.first_frame for b, i in zip(blobs, infos)]
    ptr = _ptr(lens)
    n_bytes = int(ptr[-1])
    desc = np.zeros(U, dtype=hb.FLAC_DESC)
    desc["byte_begin"], desc["byte_end"] = ptr[:-1], ptr[1:]
    desc["rate"], desc["channels"], desc["bps"] = [i.sample_rate for i in infos], [i.channels for i in infos], [i.bps for i in infos]
    desc["min_block"] = [i.min_block for i in infos]
    counts = [0] * U
    chain = []
    if n_bytes:
        host = torch.empty(n_bytes, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        for j, (b, i) in enumerate(zip(blobs, infos)):
            hv[ptr[j]:ptr[j + 1]] = np.frombuffer(b, dtype=np.uint8, offset=i.first_frame)
        buf = host.to(device, non_blocking=True)
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(device)
        info = torch.empty(n_bytes, dtype=torch.int32, device=device)
        hb.flac_scan(buf, desc_d, info)
        cand = torch.nonzero(info).flatten()
        nc = cand.numel()
        if nc:
            st, end, spos = (torch.empty(nc, dtype=dt, device=device) for dt in (torch.int32, torch.int64, torch.int64))
            hb.flac_decode(buf, desc_d, cand, st, end, spos)
            words = info[cand].cpu().numpy()
            pos_h, st_h, end_h, spos_h = (t.cpu().numpy() for t in (cand, st, end, spos))
            bs_l = ((words & 0x7FFFFFFF) >> 8).tolist()
            nxt = np.searchsorted(pos_h, end_h)  # the candidate that starts where this one ends, when there is one
            linked = (pos_h[np.minimum(nxt, nc - 1)] == end_h).tolist()
            nxt_l, st_l, end_l, spos_l = nxt.tolist(), st_h.tolist(), end_h.tolist(), spos_h.tolist()
            first = np.searchsorted(pos_h, ptr[:-1])
        # the chain of a file: the frame at its first byte, then the one that starts where it ends, to the end of the file
        for j in range(U):
            p, e, expect = int(ptr[j]), int(ptr[j + 1]), 0
            where = lambda q: infos[j].first_frame + q - int(ptr[j])  # noqa: E731
            if p < e:
                k = int(first[j]) if nc else 0
                ok = nc > 0 and k < nc and int(pos_h[k]) == p
                while True:
                    if not ok:
                        raise ValueError("%s: no valid frame header at byte offset %d, where the chain of frames leads (a broken or "
                                         "truncated FLAC stream)" % (names[j], where(p)))
                    if st_l[k] != 0:
                        raise ValueError("%s: the frame at byte offset %d is broken: %s" % (names[j], where(p), hb.FLAC_STATUS.get(st_l[k], st_l[k])))
                    if spos_l[k] != expect:
                        raise ValueError("%s: the frame at byte offset %d starts at sample %d, the frames before it end at %d"
                                         % (names[j], where(p), spos_l[k], expect))
                    chain.append(k)
                    expect += bs_l[k]
                    p = end_l[k]
                    if p >= e:
                        break
                    ok, k = linked[k], nxt_l[k]
            if infos[j].total_samples and expect != infos[j].total_samples:
                raise ValueError("%s: the frames up to byte offset %d hold %d samples, STREAMINFO announces %d"
                                 % (names[j], where(p), expect, infos[j].total_samples))
            counts[j] = expect
    elems = [c * i.channels for c, i in zip(counts, infos)]
    optr = _ptr(elems)
    res = np.zeros(0, dtype=np.int32)
    if chain:
        desc["out_off"], desc["n_samples"] = optr[:-1], counts
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(device)
        cpos = cand[torch.from_numpy(np.asarray(chain, dtype=np.int64)).to(device)]
        m = cpos.numel()
        st, end, spos = (torch.empty(m, dtype=dt, device=device) for dt in (torch.int32, torch.int64, torch.int64))
        out = torch.empty(int(optr[-1]), dtype=torch.int32, device=device)
        hb.flac_decode(buf, desc_d, cpos, st, end, spos, out)
        pinned = torch.empty(out.shape, dtype=torch.int32, pin_memory=True)
        pinned.copy_(out, non_blocking=True)
        bad = int((st != 0).sum().cpu().item())  # (synchronises: the copy is done too)
        if bad:
            raise RuntimeError("fhvae_flac_decode: %d frame(s) that parsed in the first pass failed in the second" % bad)
        res = pinned.numpy()
    out = []
    for j, i in enumerate(infos):
        x = res[optr[j]:optr[j + 1]].reshape(counts[j], i.channels).copy()
        if verify_md5 and i.md5 != bytes(16) and _flac_md5(x, i.bps) != i.md5:
            raise ValueError("%s: MD5 of the decoded audio %s differs from STREAMINFO's %s" % (names[j], _flac_md5(x, i.bps).hex(), i.md5.hex()))
        out.append((x, i.sample_rate, i.bps))
    return out


def decode_flac(blobs, names=None, device="cuda", verify_md5=False, max_samples=BATCH_SAMPLES):
    """Native FLAC files, each the bytes of a whole file -> list of (int32 (n, channels) samples, sample rate, bits per sample),
    decoded on the device in batches of about `max_samples` samples.  A stream that is broken anywhere -- a frame that does
    not parse, a CRC-16 mismatch, frames that do not follow each other, a sample count other than STREAMINFO's -- is a
    ValueError naming the file (`names`) and the byte offset.  `verify_md5`: also compare the MD5 of the decoded audio with
    STREAMINFO's (an all-zero one means "not set" and is skipped)."""
    import flac_lite

    names = list(names) if names is not None else ["FLAC file %d" % j for j in range(len(blobs))]
    if len(names) != len(blobs):
        raise ValueError("names must have one entry per file (%d)" % len(blobs))
    infos = [flac_lite.parse_flac(b, n) for b, n in zip(blobs, names)]
    if not blobs:
        return []
    import hip_binding as hb

    # a batch is bounded by its decoded size; a file of unknown length counts as 4 samples per byte, a compression speech does not reach
    sizes = [(i.total_samples or 4 * len(b)) * i.channels for b, i in zip(blobs, infos)]
    out = []
    for a, b in batches(sizes, max_samples):
        out.extend(_flac_batch(hb, blobs[a:b], infos[a:b], names[a:b], device, verify_md5))
    return out


def read_audio_batch(paths, channel=None, verify_md5=False, threads=8):
    """read_audio for many files -> list of (samples float32 (n,), sample rate) in input order.  Files are read by `threads`
    threads; WAV and SPHERE files are converted on the host as they are read, all FLAC files are decoded together on the device."""
    import concurrent.futures as cf

    def load(path):
        with open(str(path), "rb") as fh:
            head = fh.read(8)
            if head[:4] == b"fLaC" or head[:3] == b"ID3" or head[:4] == b"OggS":  # (the last two: flac_lite says why not)
                return head + fh.read()
        if head[:4] == b"RIFF":
            return read_wav(path, channel)
        if head == SPHERE_MAGIC:
            return read_sphere(path, channel)
        raise ValueError("%s: unknown audio format (the first bytes are %r); supported: %s" % (path, head, AUDIO_MAGICS))

    paths = list(paths)
    if threads > 1 and len(paths) > 1:
        with cf.ThreadPoolExecutor(max_workers=threads) as pool:
            got = list(pool.map(load, paths))
    else:
        got = [load(p) for p in paths]
    idx = [j for j, g in enumerate(got) if isinstance(g, bytes)]
    if idx:
        dec = decode_flac([got[j] for j in idx], [str(paths[j]) for j in idx], verify_md5=verify_md5)
        for j, (x, sr, bps) in zip(idx, dec):
            got[j] = (pcm_to_float(x, bps, channel, paths[j]), sr)
    return got


def read_audio(path, channel=None):
    """What read_wav returns, for a RIFF WAV, a native FLAC or a NIST SPHERE file, told apart by their first bytes."""
    return read_audio_batch([path], channel)[0]


# ---------------------------------------------------------------------------------------------------------- sizes, bases
def frame_sizes(sr, win_t=0.025, hop_t=0.010):
    """(n_fft, hop) by the reference's integer truncation (prepare_numpy_data.py:34, utils.py:182-183)."""
    return int(sr * win_t), int(sr * hop_t)


def num_frames(length, n_fft, hop):
    """Frames of a centred STFT of `length` samples: 1 + (length + 2 * (n_fft // 2) - n_fft) // hop."""
    return 1 + (length + 2 * (n_fft // 2) - n_fft) // hop


def hz_to_mel(f):
    """Slaney mel scale (librosa.hz_to_mel, htk=False): linear below 1 kHz, logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3)
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    lin = m * (200.0 / 3)
    log = 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0))
    return np.where(m >= 15.0, log, lin)


def mel_filters(sr, n_fft, n_mels):
    """(n_mels, n_fft // 2 + 1) float64 slaney-normalised triangles, as librosa.filters.mel(sr, n_fft, n_mels) (0.8.0)."""
    fft_freqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    return weights * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]


def _padded_sizes(n_fft):
    n_bins = n_fft // 2 + 1
    return (n_fft + 15) // 16 * 16, n_bins, (n_bins + 15) // 16


def hamming(n_fft):
    """Periodic Hamming window (scipy get_window("hamming", n_fft, fftbins=True)) in float64."""
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def _dft_layout(w, period, n_bins, n_cols):
    """The kernels' (32 * G, n_cols) f32 DFT basis for a window w of N <= n_cols samples: row 32g + i =
    w[n] cos(2 pi n b / period), row 32g + 16 + i = -w[n] sin(...), for bin b = 16g + i < n_bins and n < N (zero elsewhere).
    Built in float64 with the phase reduced exactly (n * b mod period), then rounded to f32."""
    N, G = len(w), (n_bins + 15) // 16
    ph = 2.0 * np.pi * ((np.arange(n_bins)[:, None] * np.arange(N)[None, :]) % period) / period
    c = np.zeros((16 * G, N))
    s = np.zeros((16 * G, N))
    c[:n_bins] = w * np.cos(ph)
    s[:n_bins] = -w * np.sin(ph)
    out = np.zeros((G, 2, 16, n_cols), dtype=np.float64)
    out[:, 0, :, :N] = c.reshape(G, 16, N)
    out[:, 1, :, :N] = s.reshape(G, 16, N)
    return out.reshape(32 * G, n_cols).astype(np.float32)


def _mel_layout(m):
    """A (n_mels, n_bins) mel bank zero-padded to the kernels' f32 (16 * ceil(n_mels / 16), 16 * ceil(n_bins / 16))."""
    out = np.zeros(((m.shape[0] + 15) // 16 * 16, (m.shape[1] + 15) // 16 * 16), dtype=np.float32)
    out[:m.shape[0], :m.shape[1]] = m
    return out


def dft_basis(n_fft):
    """The kernel's (32 * G, KP) f32 basis (_dft_layout) of the n_fft-point DFT under the periodic Hamming window, bins
    0 .. n_fft // 2, KP = n_fft rounded up to 16."""
    KP, n_bins, _ = _padded_sizes(n_fft)
    return _dft_layout(hamming(n_fft), n_fft, n_bins, KP)


def mel_basis(sr, n_fft, n_mels):
    """The kernel's (16 * ceil(n_mels / 16), 16 * G) f32 mel basis for an STFT of n_fft points (n_fft' = 2 * (n_bins - 1))."""
    return _mel_layout(mel_filters(sr, 2 * (n_fft // 2), n_mels))


# ---------------------------------------------------------------------------------------------------------- resampling
# librosa.load(path, sr) resamples with resampy 0.2.2's kaiser_best filter (librosa 0.8.0: resample(..., fix=True,
# scale=False)).  The filter is rebuilt from its published parameters; for a rational ratio L / M = sr_out / sr_in there
# are L distinct phases, so every weight is computed once here in float64 and the device runs a polyphase FIR
# (csrc/resample.hip).
RS_NUM_ZEROS = 64
RS_NUM_TABLE = 512  # precision 9: table entries per zero crossing
RS_ROLLOFF = 0.9475937167399596
RS_BETA = 14.769656459379492
RS_MAX_L = 4096  # FHVAE_RESAMPLE_MAX_L
RS_MAX_BANK = 1 << 24  # FHVAE_RESAMPLE_MAX_BANK (f32 elements: 64 MiB)
RS_LDS_FLOATS = 40128  # FHVAE_RESAMPLE_LDS_FLOATS: 16 window rows of KP + 4 floats must fit (a CU's 160 KiB less the row bookkeeping)
RS_BAD_PTR = 1

_RS_CACHE = {}


def resample_filter():
    """resampy's kaiser_best half filter, 32769 float64 entries: kaiser(2n + 1, beta)[n:] * rolloff * sinc(rolloff * x),
    x = linspace(0, 64, n + 1), n = 512 * 64.  The Kaiser window is i0(beta * sqrt(1 - (k / n)^2)) / i0(beta)."""
    if "filter" not in _RS_CACHE:
        n = RS_NUM_TABLE * RS_NUM_ZEROS
        k = np.arange(n + 1, dtype=np.float64)
        taper = np.i0(RS_BETA * np.sqrt(np.maximum(0.0, 1.0 - (k / n) ** 2))) / np.i0(RS_BETA)
        _RS_CACHE["filter"] = taper * RS_ROLLOFF * np.sinc(RS_ROLLOFF * np.linspace(0.0, RS_NUM_ZEROS, n + 1))
    return _RS_CACHE["filter"]


def resampled_length(n, sr_in, sr_out):
    """Samples librosa returns for n input samples: ceil(n * ratio) in float64 (resampy computes int(n * ratio) of them,
    the rest is zero padding).  Works on arrays."""
    ratio = float(sr_out) / sr_in
    return np.ceil(np.asarray(n, dtype=np.float64) * ratio).astype(np.int64) if np.ndim(n) else int(np.ceil(n * ratio))


def _computed_length(n, sr_in, sr_out):
    ratio = float(sr_out) / sr_in
    return (np.asarray(n, dtype=np.float64) * ratio).astype(np.int64)


class ResampleBank:
    """The polyphase form of one (sr_in, sr_out) pair.  An output row is P periods: P * L outputs computed from the window
    x[row * P * M - WL + k], k < KP.  bank (NCP, KP) float64 (f32 for the device in bank32): row c = p * L + r holds
    the weights of output c of a row over that window (zero outside its taps, zero rows past P * L).  chunks (NCP / 16, 2)
    int32: the 16-sample chunks [c0, c1) of the window that the 16 columns of a group use; the kernel multiplies only
    those.  alt (alt_taps,) / alt_wl: the weights of an output whose time register fell just below its integer time
    (see resample_exceptions), over x[p * M - 1 - alt_wl + k]."""

    def __init__(self, sr_in, sr_out):
        import math

        g = math.gcd(int(sr_in), int(sr_out))
        L, M = int(sr_out) // g, int(sr_in) // g
        self.sr_in, self.sr_out, self.L, self.M = int(sr_in), int(sr_out), L, M
        self.ratio = float(sr_out) / sr_in
        scale = min(1.0, self.ratio)
        self.scale = scale
        step = int(scale * RS_NUM_TABLE)
        if L > RS_MAX_L or step < 1:
            raise ValueError("resampling %d -> %d Hz is not supported: the reduced ratio %d / %d has more than %d phases"
                             % (sr_in, sr_out, L, M, RS_MAX_L))
        self.index_step = step
        table = resample_filter() * (scale if self.ratio < 1 else 1.0)
        delta = np.zeros_like(table)
        delta[:-1] = np.diff(table)
        nwin = len(table)
        wing = nwin // step  # the most taps a wing can have (offset 0)
        taps = 2 * wing
        P0 = max(-(-taps // M), -(-16 // L))
        P = min(range(P0, 2 * P0 + 1), key=lambda p: (-(-p * L // 16) * 16 / (p * L), p))
        WL = wing - 1
        KP = (WL + P * M + wing + 15) // 16 * 16
        NCP = (P * L + 15) // 16 * 16
        if 16 * (KP + 4) > RS_LDS_FLOATS or NCP * KP > RS_MAX_BANK:
            raise ValueError("resampling %d -> %d Hz is not supported: a window of %d samples (limit %d) or a bank of %d "
                             "weights (limit %d) is too large" % (sr_in, sr_out, KP, RS_LDS_FLOATS // 16 - 4, NCP * KP,
                                                                  RS_MAX_BANK))
        self.P, self.WL, self.KP, self.NCP, self.wing = P, WL, KP, NCP, wing
        bank = np.zeros((NCP, KP), dtype=np.float64)
        for c in range(P * L):
            n, k = divmod(c * M, L)
            self._wings(bank[c], n + WL, scale * (k / L), table, delta)
        self.bank = bank
        self.bank32 = bank.astype(np.float32)
        nz = (self.bank32.reshape(NCP // 16, 16, KP // 16, 16) != 0).any(axis=(1, 3))
        ch = np.zeros((NCP // 16, 2), dtype=np.int32)
        for gi in range(NCP // 16):
            w = np.flatnonzero(nz[gi])
            if len(w):
                ch[gi] = (w[0], w[-1] + 1)
        self.chunks = ch
        # the phase just below an integer time: n = p * M - 1, frac -> scale from below
        alt = np.zeros(2 * wing + 1, dtype=np.float64)
        self._wings(alt, wing - 1, scale * (1.0 - 2.0 ** -40), table, delta)
        w = np.flatnonzero(alt)
        self.alt_wl = (wing - 1) - int(w[0])
        self.alt = alt[w[0]:w[-1] + 1].copy()
        self.alt32 = self.alt.astype(np.float32)
        # whether an integer time is a discontinuity of resampy's filter: only when index_step was truncated
        self.discontinuous = step != scale * RS_NUM_TABLE
        self._exc = np.zeros(0, dtype=np.uint8)
        self._exc_time = 0.0

    def _wings(self, row, centre, frac, table, delta):
        """Adds resampy's weights for an output at input sample `centre` (index into row) + frac / scale."""
        step, nwin = self.index_step, len(table)
        f = frac * RS_NUM_TABLE
        off = int(f)
        eta = f - off
        i = np.arange((nwin - off) // step)
        row[centre - i] = table[off + i * step] + eta * delta[off + i * step]
        f = (self.scale - frac) * RS_NUM_TABLE
        off = int(f)
        eta = f - off
        k = np.arange((nwin - off) // step)
        row[centre + 1 + k] = table[off + k * step] + eta * delta[off + k * step]

    def terms(self, n_out):
        """Products the kernel accumulates for output samples 0 .. n_out - 1 of an utterance (zero padding included)."""
        per_col = np.repeat(16 * (self.chunks[:, 1] - self.chunks[:, 0]), 16)[:self.P * self.L]
        t = per_col[np.arange(n_out) % (self.P * self.L)].astype(np.int64)
        e = self.exceptions(-(-n_out // self.L))
        idx = np.flatnonzero(e) * self.L
        t[idx[idx < n_out]] = 64 * -(-len(self.alt) // 64)
        return t

    def exceptions(self, n_periods):
        """uint8 (n_periods,): 1 where resampy's time register, advanced by repeated float64 addition of 1 / ratio, sits
        just below the integer time p * M of output sample p * L, so that resampy takes n = p * M - 1 and the phase at
        the end of the interval.  Where the filter is continuous there (index_step not truncated, every upsampling) the
        two readings agree and no exception is reported."""
        if not self.discontinuous:
            return np.zeros(n_periods, dtype=np.uint8)
        have = len(self._exc)
        if have < n_periods:
            inc = 1.0 / self.ratio
            new = np.zeros(n_periods - have, dtype=np.uint8)
            blk = max(1, (1 << 22) // self.L)  # periods per block of the running sum
            t = self._exc_time
            for a in range(0, len(new), blk):
                b = min(a + blk, len(new))
                acc = np.empty((b - a) * self.L + 1)
                acc[0] = t
                acc[1:] = inc
                acc = np.cumsum(acc)  # sequential float64 additions, as the time register
                at = acc[:-1:self.L]
                new[a:b] = at.astype(np.int64) < (np.arange(have + a, have + b, dtype=np.int64) * self.M)
                t = acc[-1]
            self._exc = np.concatenate([self._exc, new])
            self._exc_time = t
        return self._exc[:n_periods]


def resample_bank(sr_in, sr_out):
    """The cached ResampleBank of a pair of rates; ValueError naming both rates and the limit for a ratio whose reduced
    L / M has too many phases or too wide a window."""
    key = (int(sr_in), int(sr_out))
    if key[0] < 1 or key[1] < 1:
        raise ValueError("sample rates must be positive, got %r -> %r" % (sr_in, sr_out))
    if key not in _RS_CACHE:
        _RS_CACHE[key] = ResampleBank(*key)
    return _RS_CACHE[key]


def resample_host(y, sr_in, sr_out):
    """Float64 numpy model of the device computation (the bank applied row by row); for tests and small inputs."""
    b = resample_bank(sr_in, sr_out)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n_ret, n_calc = resampled_length(len(y), sr_in, sr_out), int(_computed_length(len(y), sr_in, sr_out))
    PL, PM = b.P * b.L, b.P * b.M
    rows = -(-n_ret // PL)
    x = np.concatenate([np.zeros(b.WL), y, np.zeros(rows * PM + b.KP)])
    out = np.concatenate([b.bank[:PL] @ x[r * PM:r * PM + b.KP] for r in range(rows)]) if rows else np.zeros(0)
    out = out[:n_ret].copy()
    xa = np.concatenate([np.zeros(b.alt_wl + 1), y, np.zeros(len(b.alt))])
    for p in np.flatnonzero(b.exceptions(-(-n_ret // b.L))):
        if p * b.L < n_calc:
            out[p * b.L] = b.alt @ xa[p * b.M:p * b.M + len(b.alt)]
    out[n_calc:] = 0.0
    return out


# ---------------------------------------------------------------------------------------------------------- the launch
def check_params(sr, ftype, win_t, hop_t, n_mels):
    if ftype not in FTYPES:
        raise ValueError("ftype must be one of %s, got %r" % (FTYPES, ftype))
    n_fft, hop = frame_sizes(sr, win_t, hop_t)
    if not 2 <= n_fft <= MAX_NFFT:
        raise ValueError("n_fft = int(sr * win_t) = %d is outside [2, %d]" % (n_fft, MAX_NFFT))
    if hop < 1:
        raise ValueError("hop = int(sr * hop_t) = %d must be at least 1" % hop)
    if ftype == "fbank" and not 1 <= n_mels <= MAX_NMELS:
        raise ValueError("n_mels = %d is outside [1, %d]" % (n_mels, MAX_NMELS))
    return n_fft, hop


class _Bases:
    """Device copies of the bases for one (sr, n_fft, n_mels, ftype), built once per compute_features call."""

    def __init__(self, sr, n_fft, n_mels, ftype, device):
        import torch

        self.dft = torch.from_numpy(dft_basis(n_fft)).to(device)
        self.mel = torch.from_numpy(mel_basis(sr, n_fft, n_mels)).to(device) if ftype == "fbank" else None


def _ptr(counts):
    """(len + 1,) int64: the running sum of `counts` behind a 0."""
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _upload(arrays, device, scale=None):
    """The float32 arrays concatenated (along axis 0) in a pinned buffer, times `scale`, -> their device copy."""
    import torch

    host = torch.empty((sum(len(a) for a in arrays),) + arrays[0].shape[1:], dtype=torch.float32, pin_memory=True)
    np.concatenate(arrays, out=host.numpy())
    if scale is not None:
        host.mul_(scale)
    return host.to(device, non_blocking=True)


def _upload_ptrs(ptrs, device):
    import torch

    return torch.from_numpy(np.stack(ptrs)).pin_memory().to(device, non_blocking=True)


def _download(out, statuses, what, ptr):
    """The end of a batch: `out` comes back through a pinned buffer, the status word(s) are read (which synchronises: the
    copy is done too), a set one raises RuntimeError(what % status), -> rows ptr[j] : ptr[j + 1] of the result, one array each."""
    import torch

    res = torch.empty(out.shape, dtype=torch.float32, pin_memory=True)
    res.copy_(out, non_blocking=True)
    st = tuple(int(s.cpu().item()) for s in statuses)
    if any(st):
        raise RuntimeError(what % (st[0] if len(st) == 1 else (st,)))
    r = res.numpy()
    return [r[ptr[j]:ptr[j + 1]].copy() for j in range(len(ptr) - 1)]


def _feats_batch(hb, wave_d, lens, n_fft, hop, n_mels, ftype, bases, device, what, statuses=(), vad=None):
    """fhvae_feats_fwd on the concatenated waveforms of `lens` samples on the device -> their features; `statuses`: the status
    words of what ran before it on the stream.  `vad` (a _vad_spec): -> (features, decisions), see _vad_finish."""
    import torch

    frame_ptr = _ptr(num_frames(lens, n_fft, hop))
    ptrs_d = _upload_ptrs([_ptr(lens), frame_ptr], device)
    out = torch.empty((int(frame_ptr[-1]), n_mels if ftype == "fbank" else n_fft // 2 + 1), dtype=torch.float32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    hb.feats_fwd(wave_d, ptrs_d[0], ptrs_d[1], bases.dft, bases.mel, n_fft, hop, n_mels, ftype, out, status)
    if vad is not None:
        return _vad_finish(wave_d, ptrs_d, frame_ptr, out, vad, tuple(statuses) + (status,), what)
    return _download(out, tuple(statuses) + (status,), what, frame_ptr)


def _run_batch(hb, waves, n_fft, hop, n_mels, ftype, bases, device, vad=None):
    return _feats_batch(hb, _upload(waves, device), np.array([len(w) for w in waves], dtype=np.int64), n_fft, hop, n_mels, ftype,
                        bases, device, "fhvae_feats_fwd: status %d (inconsistent wave_ptr / frame_ptr)", vad=vad)


def batches(lengths, max_samples=BATCH_SAMPLES):
    """Consecutive index ranges [a, b) whose total length stays within max_samples (a longer utterance goes alone)."""
    out, a, tot = [], 0, 0
    for j, n in enumerate(lengths):
        if j > a and tot + n > max_samples:
            out.append((a, j))
            a, tot = j, 0
        tot += n
    if a < len(lengths):
        out.append((a, len(lengths)))
    return out


class _ResampleDev:
    """Device copies of one ResampleBank."""

    def __init__(self, bank, device):
        import torch

        self.b = bank
        self.bank = torch.from_numpy(bank.bank32).to(device)
        self.chunks = torch.from_numpy(bank.chunks).to(device)
        self.alt = torch.from_numpy(bank.alt32).to(device) if bank.discontinuous else None


def _resample_batch(hb, waves, rd, device):
    """One launch: the waveforms (float32, one source rate) -> (device tensor of the concatenated results, their lengths)."""
    import torch

    b = rd.b
    lens = np.array([len(w) for w in waves], dtype=np.int64)
    olens = resampled_length(lens, b.sr_in, b.sr_out)
    PL = b.P * b.L
    rows = -(-olens // PL)
    ptrs = [_ptr(v) for v in (lens, olens, rows)]
    n_out, n_rows = int(ptrs[1][-1]), int(ptrs[2][-1])
    out = torch.zeros(n_out, dtype=torch.float32, device=device)
    if n_out == 0:
        return out, olens, torch.zeros(1, dtype=torch.int32, device=device)
    wave_d = _upload(waves, device)
    ptrs_d = _upload_ptrs(ptrs, device)
    exc = None
    if rd.alt is not None:
        exc = torch.from_numpy(b.exceptions(int(-(-olens.max() // b.L))).copy()).to(device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    hb.resample_fwd(wave_d, ptrs_d[0], ptrs_d[1], ptrs_d[2], n_rows, rd.bank, rd.chunks, b.L, b.M, b.P, b.WL, b.ratio, exc,
                    rd.alt if exc is not None else None, b.alt_wl, out, status)
    return out, olens, status


def resample(waves, sr_in, sr_out, device="cuda", max_samples=BATCH_SAMPLES):
    """Every waveform (float32 1-D arrays at rate sr_in) converted to sr_out as librosa.load does (resampy kaiser_best,
    ceil(n * sr_out / sr_in) samples) -> list of float32 arrays, in input order; batched into launches of at most
    `max_samples` input samples.  sr_in == sr_out returns the input unchanged."""
    if sr_in == sr_out:
        return list(waves)
    bank = resample_bank(sr_in, sr_out)
    waves = [np.ascontiguousarray(w, dtype=np.float32).reshape(-1) for w in waves]
    if not waves:
        return []
    import hip_binding as hb

    rd = _ResampleDev(bank, device)
    out = []
    for a, b in batches([len(w) for w in waves], max_samples):
        y, olens, status = _resample_batch(hb, waves[a:b], rd, device)
        out.extend(_download(y, (status,), "fhvae_resample_fwd: status %d (inconsistent in_ptr / out_ptr / row_ptr)", _ptr(olens)))
    return out


def _features_resampled(hb, waves, rd, n_fft, hop, n_mels, ftype, bases, device, names, vad=None):
    """One batch at a source rate: resampled on the device and handed to fhvae_feats_fwd there (no host round trip)."""
    y, olens, status = _resample_batch(hb, waves, rd, device)
    for j, n in enumerate(olens):
        if n < n_fft // 2 + 1:
            raise ValueError("%s: %d samples after resampling; at least n_fft // 2 + 1 = %d are needed" % (names[j], n, n_fft // 2 + 1))
    return _feats_batch(hb, y, olens, n_fft, hop, n_mels, ftype, bases, device,
                        "fhvae_resample_fwd / fhvae_feats_fwd: status %s (inconsistent pointers)", (status,), vad=vad)


def _rate_groups(rates, n):
    """{source rate: the indices of its waveforms, in order}; ValueError unless there is one rate per waveform."""
    if len(rates) != n:
        raise ValueError("rates has %d entries for %d waveforms" % (len(rates), n))
    groups = {}
    for j, r in enumerate(rates):
        groups.setdefault(int(r), []).append(j)
    return groups


def _compute_features_rates(waves, rates, sr, ftype, win_t, hop_t, n_mels, names, device, max_samples, vad=None):
    import hip_binding as hb

    n_fft, hop = check_params(sr, ftype, win_t, hop_t, n_mels)
    groups = _rate_groups(rates, len(waves))
    names = list(names) if names is not None else ["utterance %d" % j for j in range(len(waves))]
    banks = {r: resample_bank(r, sr) for r in groups if r != sr}  # (an unsupported ratio fails before any work)
    out = [None] * len(waves)
    bases = None
    spec = _vad_spec_reference(vad, n_fft, hop) if vad is not None else None
    for r, idx in groups.items():
        if r == sr:
            got = compute_features([waves[j] for j in idx], sr, ftype, win_t, hop_t, n_mels, [names[j] for j in idx], device,
                                   max_samples, vad=vad)
            if vad is not None:
                got = list(zip(*got))
        else:
            ws = [np.ascontiguousarray(waves[j], dtype=np.float32).reshape(-1) for j in idx]
            if bases is None:
                bases = _Bases(sr, n_fft, n_mels, ftype, device)
            rd = _ResampleDev(banks[r], device)
            got = []
            for a, b in batches([len(w) for w in ws], max_samples):
                g = _features_resampled(hb, ws[a:b], rd, n_fft, hop, n_mels, ftype, bases, device, [names[j] for j in idx[a:b]], spec)
                got.extend(g if vad is None else zip(*g))
        for j, g in zip(idx, got):
            out[j] = g
    if vad is not None:
        return [o[0] for o in out], [o[1] for o in out]
    return out


def compute_features(waves, sr, ftype="fbank", win_t=0.025, hop_t=0.010, n_mels=80, names=None, device="cuda",
                     max_samples=BATCH_SAMPLES, rates=None, vad=None):
    """Features of every waveform (float32 1-D arrays at rate `sr`) -> list of float32 (nframes, n_mels) for "fbank" or
    (nframes, n_fft // 2 + 1) for "spec", in input order.  Batched into launches of at most `max_samples` samples.
    `names` (optional) label the utterances in error messages.  `rates` (optional, one source rate per waveform): the
    waveforms whose rate is not `sr` are grouped by rate, resampled to `sr` on the device (see resample) and their features
    computed from the device copy; the others take the same path as without `rates`.  `vad` (optional, a dict with
    "th_ratio" (default 1.04 / 2) and "drop" (default False)): -> (features, decisions), the decisions of energy_vad computed
    from the waveform already on the device (after resampling), one bool array over the utterance's frames each; with drop
    only the voiced rows of every utterance are selected on the device and downloaded (an utterance may be left with none)."""
    if rates is not None:
        return _compute_features_rates(waves, rates, sr, ftype, win_t, hop_t, n_mels, names, device, max_samples, vad)
    import hip_binding as hb

    n_fft, hop = check_params(sr, ftype, win_t, hop_t, n_mels)
    waves = [np.ascontiguousarray(w, dtype=np.float32).reshape(-1) for w in waves]
    for j, w in enumerate(waves):
        if len(w) < n_fft // 2 + 1:
            name = names[j] if names is not None else "utterance %d" % j
            raise ValueError("%s: %d samples; at least n_fft // 2 + 1 = %d are needed" % (name, len(w), n_fft // 2 + 1))
    spec = _vad_spec_reference(vad, n_fft, hop) if vad is not None else None
    if not waves:
        return [] if vad is None else ([], [])
    bases = _Bases(sr, n_fft, n_mels, ftype, device)
    out, vads = [], []
    for a, b in batches([len(w) for w in waves], max_samples):
        got = _run_batch(hb, waves[a:b], n_fft, hop, n_mels, ftype, bases, device, spec)
        if vad is not None:
            vads.extend(got[1])
            got = got[0]
        out.extend(got)
    return out if vad is None else (out, vads)


# ---------------------------------------------------------------------------------------------------------- synthesis
def write_wav(path, y, sr):
    """Mono 16-bit PCM: samples clipped to [-1, 1) and scaled by 2**15 (read_wav gives them back within one step)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(y)):
        raise ValueError("%s: the waveform has non-finite samples" % path)
    q = np.clip(np.round(y * 32768.0), -32768, 32767).astype("<i2")
    with _wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sr))
        w.writeframes(q.tobytes())


def window_sq(n_fft):
    return (hamming(n_fft) ** 2).astype(np.float32)


def synth_basis(n_fft):
    """The kernel's (KP, K2P) f32 synthesis basis, KP = n_fft rounded up to 16, K2P = 2 * (n_fft // 2 + 1) rounded up to 16:
    row n . (re_0, im_0, re_1, im_1, ...) = window[n] * irfft(spectrum, n_fft)[n].  Column 2b holds
    w[n] c_b cos(2 pi b n / n_fft) / n_fft and column 2b + 1 holds -w[n] c_b sin(2 pi b n / n_fft) / n_fft, with c_b = 1 for
    bin 0 and (even n_fft) bin n_fft / 2 and 2 otherwise; the imaginary parts of those bins meet sin = 0, as irfft ignores
    them.  Built in float64 with the phase reduced exactly, then rounded to f32."""
    KP, n_bins, _ = _padded_sizes(n_fft)
    K2P = (2 * n_bins + 15) // 16 * 16
    n = np.arange(n_fft)
    b = np.arange(n_bins)
    c = np.full(n_bins, 2.0)
    c[0] = 1.0
    if n_fft % 2 == 0:
        c[-1] = 1.0
    ph = 2.0 * np.pi * ((n[:, None] * b[None, :]) % n_fft) / n_fft
    scale = hamming(n_fft)[:, None] * c[None, :] / n_fft
    out = np.zeros((KP, K2P), dtype=np.float64)
    out[:n_fft, 0:2 * n_bins:2] = scale * np.cos(ph)
    out[:n_fft, 1:2 * n_bins:2] = -scale * np.sin(ph)
    return out.astype(np.float32)


def check_synth_params(sr, win_t, hop_t, n_iter, momentum, preemphasis):
    n_fft, hop = check_params(sr, "spec", win_t, hop_t, 0)
    if hop > n_fft:
        raise ValueError("hop = %d exceeds n_fft = %d: the frames would leave gaps" % (hop, n_fft))
    if n_iter < 0:
        raise ValueError("n_iter = %d must not be negative" % n_iter)
    if not 0.0 <= momentum < 1.0:
        raise ValueError("momentum = %r is outside [0, 1)" % (momentum,))
    if not 0.0 <= preemphasis < 1.0:
        raise ValueError("preemphasis = %r is outside [0, 1)" % (preemphasis,))
    return n_fft, hop


def check_specs(specs, sr, n_fft, names=None):
    """-> the spectrograms as contiguous float32 arrays; ValueError for anything synthesize cannot invert."""
    n_bins = n_fft // 2 + 1
    out = []
    for j, S in enumerate(specs):
        name = names[j] if names is not None else "spectrogram %d" % j
        S = np.asarray(S)
        if S.ndim != 2:
            raise ValueError("%s: expected a (nframes, %d) array, got shape %s" % (name, n_bins, S.shape))
        if S.shape[1] != n_bins:
            hint = ""
            if S.shape[1] == 80:
                hint = (" (80 columns look like ftype=\"fbank\" features: mel inversion is out of scope, only \"spec\" features can be "
                        "synthesized here; synthesize_mel inverts mel features)")
            raise ValueError("%s: %d columns, but sr %d and the window give n_fft // 2 + 1 = %d%s" % (name, S.shape[1], sr, n_bins, hint))
        if S.shape[0] < 2:
            raise ValueError("%s: %d frame(s); at least 2 are needed" % (name, S.shape[0]))
        out.append(np.ascontiguousarray(S, dtype=np.float32))
    return out


def frame_batches(frames, max_frames=BATCH_FRAMES):
    """Consecutive index ranges [a, b) whose total frame count stays within max_frames (a longer utterance goes alone)."""
    return batches(frames, max_frames)


class _SynthBases:
    def __init__(self, n_fft, device):
        import torch

        self.dft = torch.from_numpy(dft_basis(n_fft)).to(device)
        self.syn = torch.from_numpy(synth_basis(n_fft)).to(device)
        self.wsq = torch.from_numpy(window_sq(n_fft)).to(device)


def _synth_batch(hb, specs, phases, n_fft, hop, n_iter, momentum, preemphasis, log, bases, device, spec_dev=None):
    """Griffin-Lim of one batch; every round is two library calls on the stream, nothing is read back before the end.
    `spec_dev`: the concatenated spectrograms already on the device (synthesize_mel); `specs` then only gives the frame
    counts."""
    import torch

    frames = np.array([len(S) for S in specs], dtype=np.int64)
    lens = hop * (frames - 1)
    wave_ptr, frame_ptr = _ptr(lens), _ptr(frames)
    n_frames, n_samples = int(frame_ptr[-1]), int(wave_ptr[-1])
    ptrs_d = torch.from_numpy(np.stack([wave_ptr, frame_ptr])).to(device)
    mag = spec_dev if spec_dev is not None else torch.from_numpy(np.concatenate(specs)).to(device)
    if log:
        mag = torch.exp(mag)
    ph = np.concatenate(phases)
    ang = torch.from_numpy(np.stack([ph.real, ph.imag], axis=-1).astype(np.float32)).to(device)
    cur = (mag.unsqueeze(-1) * ang).contiguous()
    del ang
    KP = (n_fft + 15) // 16 * 16
    ws = torch.empty((n_frames, KP), dtype=torch.float32, device=device)
    y = torch.empty(n_samples, dtype=torch.float32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    coef = momentum / (1.0 + momentum)
    keep = [torch.empty_like(cur), torch.empty_like(cur)] if coef != 0.0 and n_iter > 1 else None
    tprev = None
    for it in range(n_iter):
        hb.synth_istft(cur, ptrs_d[0], ptrs_d[1], bases.syn, bases.wsq, n_fft, hop, ws, y, status)
        rebuilt = keep[it % 2] if keep is not None and it + 1 < n_iter else None  # (the last round's is never read)
        hb.synth_project(y, ptrs_d[0], ptrs_d[1], bases.dft, mag, tprev, coef, n_fft, hop, rebuilt, cur, status)
        tprev = rebuilt
    hb.synth_istft(cur, ptrs_d[0], ptrs_d[1], bases.syn, bases.wsq, n_fft, hop, ws, y, status)
    out = torch.empty_like(y)
    hb.synth_deemph(y, ptrs_d[0], preemphasis, out, status)
    return _download(out, (status,), "fhvae_synth_*: status %d (inconsistent wave_ptr / frame_ptr)", wave_ptr)


def _check_init_phase(init_phase, shapes):
    if init_phase is None:
        return None
    if len(init_phase) != len(shapes):
        raise ValueError("init_phase has %d arrays for %d spectrograms" % (len(init_phase), len(shapes)))
    init_phase = [np.asarray(p, dtype=np.complex128) for p in init_phase]
    for j, (p, shape) in enumerate(zip(init_phase, shapes)):
        if p.shape != tuple(shape):
            raise ValueError("init_phase[%d] has shape %s, the spectrogram %s" % (j, p.shape, tuple(shape)))
    return init_phase


def synthesize(specs, sr, win_t=0.025, hop_t=0.010, n_iter=32, momentum=0.99, preemphasis=0.97, seed=0, init_phase=None,
               log=True, device="cuda", max_frames=BATCH_FRAMES, names=None):
    """Waveforms (float32, hop * (nframes - 1) samples each) of (nframes, n_fft // 2 + 1) spectrograms as
    compute_features(..., "spec") writes them (`log=True`: natural-log magnitudes; False: magnitudes), by n_iter rounds of
    Griffin-Lim with librosa 0.8.0's semantics and the inverse of the features' pre-emphasis (`preemphasis=0`: none).
    Initial phases are exp(2 pi i u), u drawn from numpy.random.RandomState(seed) utterance by utterance in input order,
    unless `init_phase` gives them: a list of complex (nframes, n_fft // 2 + 1) arrays of unit modulus.  Only "spec"
    features are taken here; mel ("fbank") features go through synthesize_mel."""
    n_fft, hop = check_synth_params(sr, win_t, hop_t, n_iter, momentum, preemphasis)
    specs = check_specs(specs, sr, n_fft, names)
    init_phase = _check_init_phase(init_phase, [S.shape for S in specs])
    rng = np.random.RandomState(seed)
    if not specs:
        return []
    import hip_binding as hb

    bases = _SynthBases(n_fft, device)
    out = []
    for a, b in frame_batches([len(S) for S in specs], max_frames):
        phases = init_phase[a:b] if init_phase is not None else [np.exp(2j * np.pi * rng.rand(*S.shape)) for S in specs[a:b]]
        out.extend(_synth_batch(hb, specs[a:b], phases, n_fft, hop, n_iter, momentum, preemphasis, log, bases, device))
    return out


# ---------------------------------------------------------------------------------------------------------- mel inversion
# "fbank" features are mel_filters . |STFT| (utils.py:257-268), so the way back to linear magnitudes is, per frame,
# min ||A x - m||^2 over x >= 0 (librosa 0.8.0 feature.inverse.mel_to_stft, power = 1).  The minimiser is not unique (A is
# n_mels x n_bins, and rank deficient at 16 kHz / 80 mels), so the algorithm is fixed instead: nnls_iters steps of FISTA
# from zero (csrc/melinv.hip), its constants computed here in float64.
NNLS_ITERS = 200


class MelBand:
    """A mel bank (n_mels, n_bins) float64 in the band form csrc/melinv.hip works on.  Slaney triangles overlap by half: a
    bin lies in at most two adjacent filters and a filter is one contiguous run of bins; a matrix of any other shape is
    refused (ValueError).  bin_filt (n_bins,) int32 / bin_w (n_bins, 2): the lower filter f of a bin and A[f, b], A[f + 1, b];
    filt_first (n_mels,) / filt_off (n_mels + 1,) int32 / filt_w (nnz,): the run of every filter and its weights."""

    def __init__(self, A):
        A = np.asarray(A, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] < 2 or not np.all(np.isfinite(A)):
            raise ValueError("a mel bank must be a finite (n_mels, n_bins) matrix, got shape %s" % (A.shape,))
        n_mels, n_bins = A.shape
        nz = A != 0.0
        self.n_mels, self.n_bins = n_mels, n_bins
        self.filt_first = np.zeros(n_mels, dtype=np.int32)
        self.filt_off = np.zeros(n_mels + 1, dtype=np.int32)
        w = []
        for j in range(n_mels):
            k = np.flatnonzero(nz[j])
            if len(k):
                if k[-1] - k[0] + 1 != len(k):
                    raise ValueError("the mel bank is not banded: filter %d is not one contiguous run of bins" % j)
                self.filt_first[j] = k[0]
                w.append(A[j, k[0]:k[-1] + 1])
            self.filt_off[j + 1] = self.filt_off[j] + len(k)
        self.filt_w = np.concatenate(w) if w else np.zeros(0)
        self.bin_filt = np.zeros(n_bins, dtype=np.int32)
        self.bin_w = np.zeros((n_bins, 2), dtype=np.float64)
        for b in range(n_bins):
            f = np.flatnonzero(nz[:, b])
            if len(f) > 2 or (len(f) == 2 and f[1] != f[0] + 1):
                raise ValueError("the mel bank is not banded: bin %d lies in filters %s, not in at most two adjacent ones"
                                 % (b, f.tolist()))
            if len(f):
                self.bin_filt[b] = f[0]
                self.bin_w[b, 0] = A[f[0], b]
                if len(f) == 2:
                    self.bin_w[b, 1] = A[f[1], b]

    def dense(self):
        """The (n_mels, n_bins) matrix again, from the filter side."""
        A = np.zeros((self.n_mels, self.n_bins))
        for j in range(self.n_mels):
            o0, o1 = self.filt_off[j], self.filt_off[j + 1]
            A[j, self.filt_first[j]:self.filt_first[j] + o1 - o0] = self.filt_w[o0:o1]
        return A

    def dense_from_bins(self):
        """The same matrix from the bin side (the two must agree: the kernel uses one per product)."""
        A = np.zeros((self.n_mels, self.n_bins))
        for b in range(self.n_bins):
            f = self.bin_filt[b]
            A[f, b] = self.bin_w[b, 0]
            if self.bin_w[b, 1] != 0.0:
                A[f + 1, b] = self.bin_w[b, 1]
        return A


def inversion_bank(sr, n_fft, n_mels):
    """The bank the "fbank" features of (sr, n_fft, n_mels) were taken with: (n_mels, n_fft // 2 + 1) float64."""
    return mel_filters(sr, 2 * (n_fft // 2), n_mels)


def nnls_constants(A, n_iter):
    """-> (inv_l float32, beta float32 (n_iter,)) of FISTA on ||A x - m||^2: L = lambda_max(A A^T) (numpy.linalg.eigvalsh,
    float64) nudged up by one part in 2**20 before 1 / L is rounded to f32, so that the f32 step is never above 1 / L;
    beta[k] = (t_k - 1) / t_{k+1}, t_0 = 1, t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2, tabulated in float64."""
    A = np.asarray(A, dtype=np.float64)
    L = float(np.linalg.eigvalsh(A @ A.T)[-1])
    if not L > 0.0:
        raise ValueError("the mel bank is zero: nothing to invert")
    inv_l = np.float32(1.0 / (L * (1.0 + 2.0 ** -20)))
    beta = np.empty(int(n_iter), dtype=np.float64)
    t = 1.0
    for k in range(int(n_iter)):
        tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        beta[k] = (t - 1.0) / tn
        t = tn
    return inv_l, beta.astype(np.float32)


def check_melinv_params(sr, win_t, hop_t, n_mels, nnls_iters):
    n_fft, hop = check_params(sr, "fbank", win_t, hop_t, n_mels)
    if nnls_iters < 1:
        raise ValueError("nnls_iters = %d must be at least 1" % nnls_iters)
    return n_fft, hop


def check_mels(mels, n_mels, names=None):
    """-> the mel features as contiguous float32 arrays; ValueError for anything mel_to_spec cannot invert.  n_mels None:
    the column count of the first array."""
    out = []
    for j, S in enumerate(mels):
        name = names[j] if names is not None else "mel features %d" % j
        S = np.asarray(S)
        if S.ndim != 2:
            raise ValueError("%s: expected a (nframes, n_mels) array, got shape %s" % (name, S.shape))
        if n_mels is None:
            n_mels = S.shape[1]
        if S.shape[1] != n_mels:
            raise ValueError("%s: %d columns, but n_mels = %d" % (name, S.shape[1], n_mels))
        if S.shape[0] < 2:
            raise ValueError("%s: %d frame(s); at least 2 are needed" % (name, S.shape[0]))
        out.append(np.ascontiguousarray(S, dtype=np.float32))
    return out, n_mels


class _MelInvDev:
    """Device copies of the band and the FISTA constants for one (sr, n_fft, n_mels, nnls_iters)."""

    def __init__(self, sr, n_fft, n_mels, nnls_iters, device):
        import torch

        A = inversion_bank(sr, n_fft, n_mels)
        band = MelBand(A)  # (refuses a bank that is not banded before anything is launched)
        self.inv_l, beta = nnls_constants(A, nnls_iters)
        self.n_bins = band.n_bins
        self.bin_filt = torch.from_numpy(band.bin_filt).to(device)
        self.bin_w = torch.from_numpy(band.bin_w.astype(np.float32)).to(device)
        self.filt_first = torch.from_numpy(band.filt_first).to(device)
        self.filt_off = torch.from_numpy(band.filt_off).to(device)
        self.filt_w = torch.from_numpy(band.filt_w.astype(np.float32)).to(device)
        self.beta = torch.from_numpy(beta).to(device)


def _melinv_batch(hb, mels, md, log, device):
    """One launch: the mel features of a batch -> ((n_frames, n_bins) device tensor, status word)."""
    import torch

    mel_d = _upload(mels, device)
    out = torch.empty((len(mel_d), md.n_bins), dtype=torch.float32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    hb.mel_invert(mel_d, md.bin_filt, md.bin_w, md.filt_first, md.filt_off, md.filt_w, md.inv_l, md.beta, out, status, in_log=log,
                  out_log=log)
    return out, status


def mel_to_spec(mels, sr, win_t=0.025, hop_t=0.010, n_mels=None, nnls_iters=NNLS_ITERS, log=True, device="cuda",
                max_frames=BATCH_FRAMES, names=None):
    """(nframes, n_fft // 2 + 1) float32 spectrograms of (nframes, n_mels) mel features as compute_features(..., "fbank")
    writes them (`log=True`: log-mels in, max(log magnitude, -50) out, as "spec" features look; False: magnitudes in and
    out), in input order: per frame the non-negative least-squares fit against mel_filters by `nnls_iters` steps of FISTA
    from zero (fhvae_mel_invert), batched into launches of at most `max_frames` frames.  `n_mels` defaults to the column
    count.  A frame's result depends on that frame alone."""
    mels, n_mels = check_mels(mels, n_mels, names)
    if n_mels is None:
        n_mels = 80  # (no features: only the parameters are checked)
    n_fft, _ = check_melinv_params(sr, win_t, hop_t, n_mels, nnls_iters)
    if not mels:
        return []
    import hip_binding as hb

    md = _MelInvDev(sr, n_fft, n_mels, nnls_iters, device)
    out = []
    for a, b in frame_batches([len(S) for S in mels], max_frames):
        spec, status = _melinv_batch(hb, mels[a:b], md, log, device)
        out.extend(_download(spec, (status,), "fhvae_mel_invert: status %d (the band points outside its arrays)",
                             _ptr([len(S) for S in mels[a:b]])))
    return out


def synthesize_mel(mels, sr, win_t=0.025, hop_t=0.010, n_mels=None, nnls_iters=NNLS_ITERS, n_iter=32, momentum=0.99,
                   preemphasis=0.97, seed=0, init_phase=None, log=True, device="cuda", max_frames=BATCH_FRAMES, names=None):
    """Waveforms (float32, hop * (nframes - 1) samples each) of (nframes, n_mels) mel features: mel_to_spec, then Griffin-Lim
    as synthesize runs it, on the device buffer the inversion left (no host round trip).  Bitwise equal to
    synthesize(mel_to_spec(mels, ...), ...) with the same arguments: the phases are drawn exactly as synthesize draws them."""
    n_fft, hop = check_synth_params(sr, win_t, hop_t, n_iter, momentum, preemphasis)
    mels, n_mels = check_mels(mels, n_mels, names)
    if n_mels is None:
        n_mels = 80
    check_melinv_params(sr, win_t, hop_t, n_mels, nnls_iters)
    n_bins = n_fft // 2 + 1
    init_phase = _check_init_phase(init_phase, [(len(S), n_bins) for S in mels])
    rng = np.random.RandomState(seed)
    if not mels:
        return []
    import hip_binding as hb

    md = _MelInvDev(sr, n_fft, n_mels, nnls_iters, device)
    bases = _SynthBases(n_fft, device)
    out = []
    for a, b in frame_batches([len(S) for S in mels], max_frames):
        phases = init_phase[a:b] if init_phase is not None else [np.exp(2j * np.pi * rng.rand(len(S), n_bins)) for S in mels[a:b]]
        spec, status = _melinv_batch(hb, mels[a:b], md, log, device)
        out.extend(_synth_batch(hb, mels[a:b], phases, n_fft, hop, n_iter, momentum, preemphasis, log, bases, device, spec_dev=spec))
        st = int(status.cpu().item())
        if st != 0:
            raise RuntimeError("fhvae_mel_invert: status %d (the band points outside its arrays)" % st)
    return out


# ---------------------------------------------------------------------------------------------------------- Kaldi fbank
# compute-fbank-feats (FbankOptions, FrameExtractionOptions, MelBanksOptions) with Kaldi's defaults.  Nothing here runs a
# Kaldi binary: the arithmetic is restated in include/fhvae_hip.h and runs in csrc/kaldi_fbank.hip.
KALDI_DEFAULTS = {
    "sample-frequency": 16000.0, "frame-length": 25.0, "frame-shift": 10.0, "preemphasis-coefficient": 0.97,
    "remove-dc-offset": True, "dither": 1.0, "window-type": "povey", "blackman-coeff": 0.42, "num-mel-bins": 23,
    "low-freq": 20.0, "high-freq": 0.0, "use-log-fbank": True, "use-power": True, "htk-compat": False, "snip-edges": True,
    "round-to-power-of-two": True, "use-energy": False, "energy-floor": 0.0, "raw-energy": True,
}
KALDI_WINDOWS = ("hamming", "hanning", "povey", "rectangular", "blackman")
KALDI_FIXED = {"snip-edges": True, "round-to-power-of-two": True, "use-energy": False}  # the only values implemented
KALDI_MAX_P = 2048  # FHVAE_KALDI_MAX_P
KALDI_MAX_N = 1504  # FHVAE_KALDI_MAX_N
KALDI_SYNTAX = "one option per line as --name=value (for example --num-mel-bins=80); blank lines and # comments are skipped"


def _kaldi_bool(text):
    t = str(text).strip().lower()
    if t in ("true", "t", "1", ""):
        return True
    if t in ("false", "f", "0"):
        return False
    raise ValueError("not a boolean: %r" % (text,))


def kaldi_fbank_options(source=None):
    """The option set of Kaldi's compute-fbank-feats from a config file (path) or a dict of option names (dashes, as Kaldi
    spells them) -> dict with every supported option, Kaldi's defaults filled in.  An unknown option, or a value that is not
    implemented (use-energy=true, snip-edges=false, round-to-power-of-two=false, any vtln-* option), raises ValueError naming
    the option and the file, as Kaldi dies on unknown options."""
    where = "options"
    given = {}
    if source is None:
        pass
    elif isinstance(source, dict):
        given = {str(k).lstrip("-").replace("_", "-"): v for k, v in source.items()}
    else:
        where = str(source)
        try:
            fh = open(where)
        except OSError as e:
            raise ValueError("%s: cannot read the Kaldi fbank configuration (%s); expected a text file with %s"
                             % (where, e.strerror or e, KALDI_SYNTAX)) from None
        with fh:
            for ln, raw in enumerate(fh, 1):
                line = raw.split("#", 1)[0].strip()
                if not line:
                    continue
                if not line.startswith("--"):
                    raise ValueError("%s:%d: %r is not an option; expected %s" % (where, ln, line, KALDI_SYNTAX))
                name, _, value = line[2:].partition("=")
                given[name.strip()] = value.strip()
    opts = dict(KALDI_DEFAULTS)
    for name, value in given.items():
        if name.startswith("vtln-"):
            raise ValueError("%s: option --%s is not supported (no VTLN warping)" % (where, name))
        if name not in KALDI_DEFAULTS:
            raise ValueError("%s: unknown option --%s (supported: %s)" % (where, name, ", ".join(sorted(KALDI_DEFAULTS))))
        kind = type(KALDI_DEFAULTS[name])
        try:
            opts[name] = _kaldi_bool(value) if kind is bool and not isinstance(value, bool) else kind(value)
        except ValueError:
            raise ValueError("%s: option --%s has the value %r, not a %s" % (where, name, value, kind.__name__)) from None
    for name, only in KALDI_FIXED.items():
        if opts[name] != only:
            raise ValueError("%s: option --%s=%s is not supported (only %s is implemented)"
                             % (where, name, str(opts[name]).lower(), str(only).lower()))
    if opts["window-type"] not in KALDI_WINDOWS:
        raise ValueError("%s: option --window-type=%s is not one of %s" % (where, opts["window-type"], ", ".join(KALDI_WINDOWS)))
    return opts


def kaldi_frame_sizes(opts):
    """(N, S, P): samples per frame and per shift by Kaldi's truncation int(sr * 0.001 * ms), and the FFT size, the smallest
    power of two >= N."""
    sr = opts["sample-frequency"]
    N, S = int(sr * 0.001 * opts["frame-length"]), int(sr * 0.001 * opts["frame-shift"])
    P = 1
    while P < N:
        P *= 2
    return N, S, P


def kaldi_num_frames(n, N, S):
    """Frames of n samples with snip-edges=true: 0 if n < N, else 1 + (n - N) // S.  Works on arrays."""
    n = np.asarray(n, dtype=np.int64)
    out = np.where(n < N, 0, 1 + (n - N) // S)
    return out if out.ndim else int(out)


def kaldi_window(N, window="povey", blackman_coeff=0.42):
    """Kaldi's FeatureWindowFunction, float64 (N,): symmetric (i / (N - 1)), unlike the periodic window of dft_basis."""
    a = 2.0 * np.pi * np.arange(N) / (N - 1)
    if window == "hamming":
        return 0.54 - 0.46 * np.cos(a)
    if window == "hanning":
        return 0.5 - 0.5 * np.cos(a)
    if window == "povey":
        return (0.5 - 0.5 * np.cos(a)) ** 0.85
    if window == "rectangular":
        return np.ones(N)
    if window == "blackman":
        return blackman_coeff - 0.5 * np.cos(a) + (0.5 - blackman_coeff) * np.cos(2.0 * a)
    raise ValueError("window type %r is not one of %s" % (window, ", ".join(KALDI_WINDOWS)))


def kaldi_mel_filters(sr, P, n_mels, low=20.0, high=0.0):
    """(n_mels, P // 2) float64: Kaldi's MelBanks without VTLN.  mel(f) = 1127 ln(1 + f / 700); n_mels + 2 points equally spaced
    in mel from `low` to `high` (<= 0: added to the Nyquist frequency); filter b rises over (point b, point b+1] and falls
    over (point b+1, point b+2) in the mel of the bin frequency i * sr / P; no area normalisation."""
    nyquist = 0.5 * sr
    hi = high if high > 0.0 else nyquist + high
    if not (0.0 <= low < nyquist and 0.0 < hi <= nyquist and low < hi):
        raise ValueError("low-freq %g / high-freq %g do not fit a Nyquist frequency of %g" % (low, high, nyquist))
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)  # noqa: E731
    pts = mel(low) + (mel(hi) - mel(low)) / (n_mels + 1) * np.arange(n_mels + 2)
    m = mel(np.arange(P // 2) * (float(sr) / P))[None, :]
    left, centre, right = pts[:-2, None], pts[1:-1, None], pts[2:, None]
    up, down = (m - left) / (centre - left), (right - m) / (right - centre)
    return np.where((m > left) & (m <= centre), up, np.where((m > centre) & (m < right), down, 0.0))


def kaldi_dft_basis(N, P, window="povey", blackman_coeff=0.42):
    """The kernel's (32 * G, KP) f32 basis (_dft_layout) of the P-point DFT over the N samples of a frame under kaldi_window,
    bins 0 .. P / 2 - 1, KP = N rounded up to 16."""
    return _dft_layout(kaldi_window(N, window, blackman_coeff), P, P // 2, (N + 15) // 16 * 16)


def kaldi_mel_basis(sr, P, n_mels, low=20.0, high=0.0):
    """The kernel's (16 * ceil(n_mels / 16), 16 * G) f32 mel basis (kaldi_mel_filters, zero-padded)."""
    return _mel_layout(kaldi_mel_filters(sr, P, n_mels, low, high))


def check_kaldi_options(opts):
    """-> (N, S, P) or ValueError for sizes the kernel does not take."""
    N, S, P = kaldi_frame_sizes(opts)
    if N < 2 or N > KALDI_MAX_N:
        raise ValueError("frame-length gives %d samples per frame, outside [2, %d]" % (N, KALDI_MAX_N))
    if not 1 <= S <= N:
        raise ValueError("frame-shift gives %d samples, outside [1, %d] (the frame length)" % (S, N))
    if not 1 <= opts["num-mel-bins"] <= MAX_NMELS:
        raise ValueError("num-mel-bins = %d is outside [1, %d]" % (opts["num-mel-bins"], MAX_NMELS))
    return N, S, P


def kaldi_stream_id(key):
    """The dither stream of an utterance key: zlib.crc32 of its UTF-8 bytes, so that a file's noise does not depend on its
    place in a list."""
    import zlib

    return zlib.crc32(str(key).encode("utf-8"))


class _KaldiBases:
    """Device copies of the bases for one option set, built once per compute_kaldi_fbank call."""

    def __init__(self, opts, N, P, device):
        import torch

        sr = opts["sample-frequency"]
        self.dft = torch.from_numpy(kaldi_dft_basis(N, P, opts["window-type"], opts["blackman-coeff"])).to(device)
        self.mel = torch.from_numpy(kaldi_mel_basis(sr, P, opts["num-mel-bins"], opts["low-freq"], opts["high-freq"])).to(device)


def _kaldi_batch(hb, waves, ids, opts, sizes, seed, bases, device, compress=None, names=None, vad=None):
    import torch

    N, S, P = sizes
    n_mels = opts["num-mel-bins"]
    lens = np.array([len(w) for w in waves], dtype=np.int64)
    frame_ptr = _ptr(kaldi_num_frames(lens, N, S))
    wave_d = _upload(waves, device, scale=32768.0)  # Kaldi's int16 scale (exact: a power of two)
    ptrs_d = _upload_ptrs([_ptr(lens), frame_ptr], device)
    dither = float(opts["dither"])
    ids_d = torch.from_numpy(np.asarray(ids, dtype=np.uint64).view(np.int64).copy()).to(device) if dither != 0.0 else None
    out = torch.empty((int(frame_ptr[-1]), n_mels), dtype=torch.float32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    flags = ((hb.KALDI_REMOVE_DC if opts["remove-dc-offset"] else 0) | (hb.KALDI_USE_LOG if opts["use-log-fbank"] else 0)
             | (hb.KALDI_USE_POWER if opts["use-power"] else 0))
    hb.kaldi_fbank_fwd(wave_d, ptrs_d[0], ptrs_d[1], ids_d, bases.dft, bases.mel, N, S, P, n_mels,
                       opts["preemphasis-coefficient"], dither, seed, flags, out, status)
    what = "fhvae_kaldi_fbank_fwd: status %d (inconsistent wave_ptr / frame_ptr)"
    if vad is not None:
        return _vad_finish(wave_d, ptrs_d, frame_ptr, out, vad, (status,), what, compress, names)
    if compress is None:
        return _download(out, (status,), what, frame_ptr)
    st = int(status.cpu().item())
    if st:
        raise RuntimeError(what % st)
    return kaldi_compress(out, np.diff(frame_ptr), compress, names)


def kaldi_compress(feats, rows, method="auto", names=None):
    """Codes the utterances stacked in `feats` ((frames, F) f32 on the device; utterance j is the next rows[j] rows) as Kaldi
    compressed matrices on the device (fhvae_kaldi_compress) -> one kaldi_io_lite.CompressedMatrix each.  `method`: "auto"
    (Kaldi's: CM above 8 rows, else CM2), "two-byte" (CM2) or "one-byte" (CM3).  Only the coded bytes and the (min, range)
    headers come back from the device."""
    import struct

    import torch

    import hip_binding as hb
    import kaldi_io_lite as K

    rows = [int(r) for r in rows]
    F = int(feats.shape[1])
    if sum(rows) != feats.shape[0] or min(rows) < 1:
        raise ValueError("kaldi_compress: %d rows in all for a matrix of %d; every utterance needs a row" % (sum(rows), feats.shape[0]))
    tokens = [K.token_for(r, method) for r in rows]
    desc, n_tiles, n_bytes = hb.kaldi_cm_descs(tokens, rows, F, _ptr(rows)[:-1])
    desc_d = torch.from_numpy(desc.view(np.uint8)).to(feats.device)
    payload = torch.empty(n_bytes, dtype=torch.uint8, device=feats.device)
    status = torch.zeros(1, dtype=torch.int32, device=feats.device)
    hb.kaldi_compress(feats, desc_d, n_tiles, payload, status)
    host = torch.empty(n_bytes, dtype=torch.uint8, pin_memory=True)
    host.copy_(payload, non_blocking=True)
    got = desc_d.cpu().numpy().view(hb.KALDI_CM_DESC)
    st = int(status.cpu().item())
    if st & hb.KALDI_CM_NONFINITE:
        bad = [j for j in range(len(rows)) if not (np.isfinite(got["min_value"][j]) and np.isfinite(got["range"][j]))]
        raise ValueError("%s: NaN or Inf in the features to compress" % ", ".join((names[j] if names is not None else "utterance %d" % j) for j in bad))
    if st:
        raise RuntimeError("fhvae_kaldi_compress: status %d (inconsistent descriptors)" % st)
    blob = host.numpy()
    out = []
    for j, (tok, r) in enumerate(zip(tokens, rows)):
        off = int(desc["payload_off"][j])
        out.append(K.CompressedMatrix(tok, struct.pack("<ffii", got["min_value"][j], got["range"][j], r, F),
                                      blob[off:off + K.payload_size(tok, r, F)].tobytes()))
    return out


def compute_kaldi_fbank(waves, opts=None, seed=0, stream_ids=None, names=None, device="cuda", max_samples=BATCH_SAMPLES,
                        rates=None, compress=None, vad=None):
    """Kaldi filterbank features of every waveform -> list of float32 (nframes, num-mel-bins), in input order.  `waves` are
    float32 1-D arrays as read_wav returns them (full scale 1.0; they are put on Kaldi's int16 scale here) at the rate
    sample-frequency of `opts` (what kaldi_fbank_options takes: a config file, a dict, or None for Kaldi's defaults).  `seed` and `stream_ids` (one 64-bit
    integer per waveform, default its index) select the dither noise, which depends on nothing else: the same
    (seed, stream id) gives the same features in any batch.  `rates` (optional, one source rate per waveform): waveforms at
    another rate are first converted with `resample`; without it every waveform is taken to be at sample-frequency, as
    Kaldi refuses other rates.  An utterance shorter than one frame is an error that names it (`names`).  With `compress`
    ("auto", "two-byte" or "one-byte") the features stay on the device, are coded there as Kaldi compressed matrices
    (kaldi_compress) and come back as kaldi_io_lite.CompressedMatrix (token, header, payload) instead of arrays.  `vad`
    (optional, a dict with "opts" (what kaldi_vad_options takes, default Kaldi's) and "drop" (default False)): ->
    (features, decisions), the decisions of kaldi_energy_vad computed from the waveform already on the device, one bool array
    over the utterance's frames each; with drop only the voiced rows are selected on the device, in front of the compression
    and the download, and an utterance left with none comes back as an empty (0, num-mel-bins) array."""
    if compress is not None:
        import kaldi_io_lite

        kaldi_io_lite.token_for(1, compress)  # (an unknown method fails before any work)
    opts = kaldi_fbank_options(opts)
    sizes = check_kaldi_options(opts)
    sr = opts["sample-frequency"]
    if sr != int(sr):
        raise ValueError("sample-frequency %r is not a whole number of Hz" % (sr,))
    kaldi_mel_filters(sr, sizes[2], opts["num-mel-bins"], opts["low-freq"], opts["high-freq"])  # (bad band edges fail here)
    waves = [np.ascontiguousarray(w, dtype=np.float32).reshape(-1) for w in waves]
    names = list(names) if names is not None else ["utterance %d" % j for j in range(len(waves))]
    ids = list(range(len(waves))) if stream_ids is None else [int(v) & 0xFFFFFFFFFFFFFFFF for v in stream_ids]
    if len(ids) != len(waves) or len(names) != len(waves):
        raise ValueError("stream_ids / names must have one entry per waveform (%d)" % len(waves))
    if rates is not None:
        groups = {r: idx for r, idx in _rate_groups(rates, len(waves)).items() if r != int(sr)}
        for r in groups:
            resample_bank(r, int(sr))  # (an unsupported ratio fails before any work)
        for r, idx in groups.items():
            for j, y in zip(idx, resample([waves[j] for j in idx], r, int(sr), device, max_samples)):
                waves[j] = y
    for j, w in enumerate(waves):
        if len(w) < sizes[0]:
            raise ValueError("%s: %d samples%s; one frame needs %d (Kaldi would skip the utterance)"
                             % (names[j], len(w), " after resampling" if rates is not None else "", sizes[0]))
    spec = _vad_spec_kaldi(vad, opts, sizes) if vad is not None else None
    if not waves:
        return [] if vad is None else ([], [])
    import hip_binding as hb

    bases = _KaldiBases(opts, sizes[0], sizes[2], device)
    out, vads = [], []
    for a, b in batches([len(w) for w in waves], max_samples):
        got = _kaldi_batch(hb, waves[a:b], ids[a:b], opts, sizes, int(seed), bases, device, compress, names[a:b], spec)
        if vad is not None:
            vads.extend(got[1])
            got = got[0]
        out.extend(got)
    return out if vad is None else (out, vads)


# ---------------------------------------------------------------------------------------------------------- energy VAD
# include/fhvae_vad.h holds the definitions; vad.py the binding.  Nothing here runs librosa or a Kaldi binary.
KALDI_VAD_DEFAULTS = {"vad-energy-threshold": 5.0, "vad-energy-mean-scale": 0.5, "vad-frames-context": 0,
                      "vad-proportion-threshold": 0.6}
VAD_MAX_FRAME = 4096  # FHVAE_VAD_MAX_FRAME
VAD_MAX_CTX = 1024  # FHVAE_VAD_MAX_CTX
VAD_TH_RATIO = 1.04 / 2  # utils.py:280
KALDI_VAD_SYNTAX = KALDI_SYNTAX.replace("--num-mel-bins=80", "--vad-energy-threshold=5.5")


def kaldi_vad_options(source=None):
    """The option set of Kaldi's compute-vad-decision from a config file (path) or a dict of option names (dashes, as Kaldi
    spells them) -> dict with the four options, the defaults of include/fhvae_vad.h filled in.  An unknown option, a value of
    the wrong kind or outside its range raises ValueError naming the option and the file, as kaldi_fbank_options does."""
    where = "options"
    given = {}
    if source is None:
        pass
    elif isinstance(source, dict):
        given = {str(k).lstrip("-").replace("_", "-"): v for k, v in source.items()}
    else:
        where = str(source)
        try:
            fh = open(where)
        except OSError as e:
            raise ValueError("%s: cannot read the Kaldi VAD configuration (%s); expected a text file with %s"
                             % (where, e.strerror or e, KALDI_VAD_SYNTAX)) from None
        with fh:
            for ln, raw in enumerate(fh, 1):
                line = raw.split("#", 1)[0].strip()
                if not line:
                    continue
                if not line.startswith("--"):
                    raise ValueError("%s:%d: %r is not an option; expected %s" % (where, ln, line, KALDI_VAD_SYNTAX))
                name, _, value = line[2:].partition("=")
                given[name.strip()] = value.strip()
    opts = dict(KALDI_VAD_DEFAULTS)
    for name, value in given.items():
        if name not in KALDI_VAD_DEFAULTS:
            raise ValueError("%s: unknown option --%s (supported: %s)" % (where, name, ", ".join(sorted(KALDI_VAD_DEFAULTS))))
        kind = type(KALDI_VAD_DEFAULTS[name])
        try:
            if kind is int and not isinstance(value, str) and int(value) != value:
                raise ValueError
            opts[name] = kind(value)
        except (TypeError, ValueError):
            raise ValueError("%s: option --%s has the value %r, not a %s" % (where, name, value, kind.__name__)) from None
    try:
        check_vad_decision(opts["vad-energy-threshold"], opts["vad-energy-mean-scale"], opts["vad-frames-context"],
                           opts["vad-proportion-threshold"])
    except ValueError as e:
        raise ValueError("%s: %s" % (where, e)) from None
    return opts


def check_vad_decision(thr_abs, mean_scale, ctx, proportion):
    """ValueError for parameters fhvae_vad_decide refuses."""
    if not (np.isfinite(thr_abs) and np.isfinite(mean_scale)):
        raise ValueError("the energy threshold %r and mean scale %r must be finite" % (thr_abs, mean_scale))
    if int(ctx) != ctx or not 0 <= ctx <= VAD_MAX_CTX:
        raise ValueError("the frames context %r is not a whole number in [0, %d]" % (ctx, VAD_MAX_CTX))
    if not 0.0 < proportion <= 1.0:
        raise ValueError("the proportion threshold %r is outside (0, 1]" % (proportion,))


def _vad_dict(vad, allowed):
    if not isinstance(vad, dict) or set(vad) - set(allowed):
        raise ValueError("vad must be a dict with the keys %s, got %r" % (", ".join(allowed), vad))
    return vad


def _vad_spec(mode, flags, frame_len, hop, thr_abs, mean_scale, ctx, proportion, drop):
    check_vad_decision(thr_abs, mean_scale, ctx, proportion)
    if not 2 <= frame_len <= VAD_MAX_FRAME or hop < 1:
        raise ValueError("a VAD frame of %d samples every %d is outside [2, %d] / below 1" % (frame_len, hop, VAD_MAX_FRAME))
    return {"mode": mode, "flags": flags, "frame_len": int(frame_len), "hop": int(hop), "thr_abs": float(thr_abs),
            "mean_scale": float(mean_scale), "ctx": int(ctx), "proportion": float(proportion), "drop": bool(drop)}


def _vad_spec_reference(vad, n_fft, hop):
    """The reference's convention (utils.py:295-299): centred RMS over the feature's own frames, voiced above th_ratio * mean."""
    import vad as V

    vad = _vad_dict(vad, ("th_ratio", "drop"))
    return _vad_spec(V.VAD_RMS_CENTER, 0, n_fft, hop, 0.0, vad.get("th_ratio", VAD_TH_RATIO), 0, 1.0, vad.get("drop", False))


def _vad_spec_kaldi(vad, fbank_opts, sizes):
    """Kaldi's convention: raw log energy over the fbank's own snip-edges frames, ComputeVadEnergy's four options."""
    import vad as V

    vad = _vad_dict(vad, ("opts", "drop"))
    o = kaldi_vad_options(vad.get("opts"))
    return _vad_spec(V.VAD_LOGE_SNIP, V.VAD_REMOVE_DC if fbank_opts["remove-dc-offset"] else 0, sizes[0], sizes[1],
                     o["vad-energy-threshold"], o["vad-energy-mean-scale"], o["vad-frames-context"], o["vad-proportion-threshold"],
                     vad.get("drop", False))


VAD_WHAT = "fhvae_vad_energy / fhvae_vad_decide / fhvae_vad_select: status %d (inconsistent wave_ptr / frame_ptr / rank)"


def _vad_device(wave_d, ptrs_d, n_frames, spec):
    """Energies and decisions of a batch that is on the device -> (vad uint8, rank int64, status), all on the device."""
    import torch

    import vad as V

    status = torch.zeros(1, dtype=torch.int32, device=wave_d.device)
    e = V.energy(wave_d, ptrs_d[0], ptrs_d[1], n_frames, spec["frame_len"], spec["hop"], spec["mode"], spec["flags"], status)
    vad_d, rank_d = V.decide(e, ptrs_d[1], spec["thr_abs"], spec["mean_scale"], spec["ctx"], spec["proportion"], status)
    return vad_d, rank_d, status


def _vad_host(vad_d, rank_d, status, ptrs_d, frame_ptr, statuses=(), what=None):
    """Downloads the decisions and the voiced count of every utterance (rank at frame_ptr), which synchronises; a set status
    word raises.  -> (one bool array per utterance, voiced_ptr (U + 1,) int64)."""
    voiced_ptr = rank_d[ptrs_d[1]].cpu().numpy()
    v = vad_d.cpu().numpy()
    st = tuple(int(s.cpu().item()) for s in statuses)
    if any(st):
        raise RuntimeError(what % (st[0] if len(st) == 1 else (st,)))
    sv = int(status.cpu().item())
    if sv:
        raise RuntimeError(VAD_WHAT % sv)
    return [v[frame_ptr[j]:frame_ptr[j + 1]].astype(bool) for j in range(len(frame_ptr) - 1)], voiced_ptr


def _vad_finish(wave_d, ptrs_d, frame_ptr, out, spec, statuses, what, compress=None, names=None):
    """The end of a feature batch with VAD: the decisions from the waveform on the device, then the features (`out`, on the
    device) whole, or with drop their voiced rows only (fhvae_vad_select in front of the download / of kaldi_compress).
    -> (features, decisions)."""
    import torch

    import vad as V

    vad_d, rank_d, status = _vad_device(wave_d, ptrs_d, int(frame_ptr[-1]), spec)
    vads, voiced_ptr = _vad_host(vad_d, rank_d, status, ptrs_d, frame_ptr, statuses, what)
    rows_ptr = frame_ptr
    if spec["drop"]:
        out = V.select(out, vad_d, rank_d, int(voiced_ptr[-1]), status)
        rows_ptr = voiced_ptr
    if compress is None:
        feats = _download(out, (status,), VAD_WHAT, rows_ptr)
    else:
        sv = int(status.cpu().item())
        if sv:
            raise RuntimeError(VAD_WHAT % sv)
        rows = np.diff(rows_ptr)
        keep = [j for j in range(len(rows)) if rows[j] > 0]  # (kaldi_compress needs a row)
        coded = kaldi_compress(out, rows[keep], compress, [names[j] for j in keep] if names is not None else None) if keep else []
        feats = [np.zeros((0, out.shape[1]), dtype=np.float32) for _ in rows]
        for j, c in zip(keep, coded):
            feats[j] = c
    return feats, vads


def _vad_waves(waves, scale, spec, min_len, frames_of, names, device, max_samples):
    waves = [np.ascontiguousarray(w, dtype=np.float32).reshape(-1) for w in waves]
    for j, w in enumerate(waves):
        if len(w) < min_len:
            raise ValueError("%s: %d samples; at least %d are needed" % (names[j] if names is not None else "utterance %d" % j, len(w), min_len))
    out = []
    for a, b in batches([len(w) for w in waves], max_samples):
        lens = np.array([len(w) for w in waves[a:b]], dtype=np.int64)
        frame_ptr = _ptr(frames_of(lens))
        wave_d = _upload(waves[a:b], device, scale=scale)
        ptrs_d = _upload_ptrs([_ptr(lens), frame_ptr], device)
        vad_d, rank_d, status = _vad_device(wave_d, ptrs_d, int(frame_ptr[-1]), spec)
        out.extend(_vad_host(vad_d, rank_d, status, ptrs_d, frame_ptr)[0])
    return out


def energy_vad(waves, sr, win_t=0.025, hop_t=0.010, th_ratio=VAD_TH_RATIO, names=None, device="cuda", max_samples=BATCH_SAMPLES):
    """The reference's AudioUtils.energy_vad (utils.py:275-300) for every waveform (float32 1-D arrays at rate `sr`, full scale
    1.0) -> one (frames,) bool array each: the RMS energy of the centred frames of int(sr * win_t) samples every
    int(sr * hop_t) (librosa.feature.rms), voiced where it exceeds th_ratio times the utterance's mean.  The frames are those
    of compute_features.  An utterance shorter than win_length // 2 + 1 samples is an error that names it."""
    n_fft, hop = frame_sizes(sr, win_t, hop_t)
    spec = _vad_spec_reference({"th_ratio": th_ratio}, n_fft, hop)
    return _vad_waves(waves, None, spec, n_fft // 2 + 1, lambda n: num_frames(n, n_fft, hop), names, device, max_samples)


def kaldi_energy_vad(waves, fbank_opts=None, vad_opts=None, names=None, device="cuda", max_samples=BATCH_SAMPLES):
    """compute-vad-decision for every waveform (float32 1-D arrays at full scale 1.0, at the sample-frequency of `fbank_opts`)
    -> one (frames,) bool array each.  The frames are those of compute_kaldi_fbank for `fbank_opts` (frame-length, frame-shift,
    snip-edges; remove-dc-offset applies to the energy too); the energy is Kaldi's raw log energy without dither; `vad_opts` is
    what kaldi_vad_options takes."""
    opts = kaldi_fbank_options(fbank_opts)
    sizes = check_kaldi_options(opts)
    spec = _vad_spec_kaldi({"opts": vad_opts}, opts, sizes)
    return _vad_waves(waves, 32768.0, spec, sizes[0], lambda n: kaldi_num_frames(n, sizes[0], sizes[1]), names, device, max_samples)


def vad_decide(energies, thr_abs, mean_scale, ctx, proportion, device="cuda"):
    """The decision of include/fhvae_vad.h on energies that come from anywhere (a list of 1-D arrays, one per utterance, each
    with at least one frame; they are rounded to float32) -> one bool array each:
    voiced where at least `proportion` of the frames within `ctx` of it exceed thr_abs + mean_scale * the utterance's mean."""
    import torch

    import vad as V

    check_vad_decision(thr_abs, mean_scale, ctx, proportion)
    energies = [np.ascontiguousarray(e, dtype=np.float32).reshape(-1) for e in energies]
    if not energies:
        return []
    for j, e in enumerate(energies):
        if len(e) < 1:
            raise ValueError("utterance %d has no frame" % j)
    frame_ptr = _ptr([len(e) for e in energies])
    e_d = _upload(energies, device)
    ptr_d = _upload_ptrs([frame_ptr], device)
    status = torch.zeros(1, dtype=torch.int32, device=e_d.device)
    vad_d, _ = V.decide(e_d, ptr_d[0], thr_abs, mean_scale, ctx, proportion, status)
    v = vad_d.cpu().numpy()
    sv = int(status.cpu().item())
    if sv:
        raise RuntimeError(VAD_WHAT % sv)
    return [v[frame_ptr[j]:frame_ptr[j + 1]].astype(bool) for j in range(len(energies))]
