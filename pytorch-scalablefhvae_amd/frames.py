"""frames.py -- a trained model applied to a whole corpus, frame by frame ("Frame-level latents"):

  encode_frames    one z1 / z2 posterior mean per window of every utterance (one per frame at shift 1: the domain-invariant
                   features the FHVAE papers hand to a recogniser) and the closed-form mu2 of every utterance
  convert_frames   every utterance decoded under its own z2 (reconstruction) or another sequence's mu2 (conversion), the
                   overlapping windows averaged back to one row per frame, un-normalised

Geometry.  An utterance of n >= 1 frames has W = ceil(n / shift) windows of the model's T frames; window k is centred on frame
k * shift: its position t stands for local frame p = k * shift - T // 2 + t and reads frame min(max(p, 0), n - 1) (edge
replication).  No utterance is too short and no tail is dropped (NumpyDataset's segments start at frame 0, need n >= T and
leave the last (n - T) % shift frames out).  The corpus is the concatenation of its utterances, described by two CSR arrays
on the device (utt_ptr: frame offsets, win_ptr: window offsets); the kernels (csrc/frames.hip, include/fhvae_frames.h) cut
windows from, and average them back onto, that description alone.

The host geometry (left, num_windows, covering, chunk_plan) is pure numpy and needs no GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hip_ext

#: bits of the int32 device status word the two kernels set (include/fhvae_frames.h, FHVAE_FRAMES_*)
FRAMES_BAD_PTR, FRAMES_BAD_RANGE = 1, 2

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry points of include/fhvae_frames.h: name -> (restype, argtypes).  They are exported from libfhvae_hip.so but are
#: not part of include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
FRAMES_SIGNATURES = {
    "fhvae_frames_gather": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fhvae_frames_overlap_mean": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
}


def load_library():
    """hip_binding.load_library() with the frames entry points bound (argtypes from FRAMES_SIGNATURES)."""
    return hip_ext.load(FRAMES_SIGNATURES)


# ------------------------------------------------------------------------------------------------------------ host geometry
def left(T: int) -> int:
    """Frames of a window in front of its centre."""
    return int(T) // 2


def max_overlap_shift(T: int) -> int:
    """The largest shift at which every frame of every utterance is covered by a window: T - T // 2."""
    return int(T) - int(T) // 2


def num_windows(n, shift: int):
    """W = ceil(n / shift) (n: an int or an integer array)."""
    return -(-n // int(shift))


def covering(f: int, n: int, T: int, shift: int):
    """(k0, k1): the windows k0 .. k1 (inclusive) of an n-frame utterance that hold local frame f at a position that is not
    a replicated edge; k1 < k0 when there is none (possible only for shift > T - T // 2)."""
    fl = int(f) + left(T)
    k0 = max(0, -(-(fl - int(T) + 1) // int(shift)))
    k1 = min(int(num_windows(int(n), shift)) - 1, fl // int(shift))
    return k0, k1


def _ptrs(lengths, shift):
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.size == 0 or lengths.min() < 1:
        raise ValueError("every utterance needs at least one frame (and the corpus one utterance)")
    if int(shift) < 1:
        raise ValueError("shift = %d must be at least 1" % shift)
    utt_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    win_ptr = np.concatenate([[0], np.cumsum(num_windows(lengths, shift))]).astype(np.int64)
    return lengths, utt_ptr, win_ptr


def chunk_plan(lengths, T: int, shift: int, max_windows: int, overlap: bool):
    """The corpus cut into chunks of at most `max_windows` windows: a list of (w0, B, g0, G).

    overlap=False  the window ranges [w0, w0 + B) tile [0, total windows); g0 = G = 0.
    overlap=True   the frame ranges [g0, g0 + G) tile [0, total frames), and [w0, w0 + B) is exactly the windows that cover
                   those frames (the first covering window of frame g0 to the last of frame g0 + G - 1), so the overlap mean
                   of a chunk reads that chunk's windows only.  Chunks are filled greedily.  A chunk boundary inside an
                   utterance makes both neighbours encode the windows that reach across it: of the windows of a chunk, at most
                   H = ceil(T / shift) - 1 per side are centred on a frame outside its frame range (the halo).  Utterances
                   are split only when max_windows >= 2 H + 1 (a halo on both sides and a window of its own); below that a
                   chunk ends where an utterance ends.
    Raises ValueError when max_windows is too small: an utterance does not fit into a chunk and may not be split."""
    T, shift, max_windows = int(T), int(shift), int(max_windows)
    lengths, utt_ptr, win_ptr = _ptrs(lengths, shift)
    if T < 1 or max_windows < 1:
        raise ValueError("T = %d and max_windows = %d must be positive" % (T, max_windows))
    n_win, n_frames, U = int(win_ptr[-1]), int(utt_ptr[-1]), lengths.shape[0]
    if not overlap:
        return [(w0, min(max_windows, n_win - w0), 0, 0) for w0 in range(0, n_win, max_windows)]
    if shift > max_overlap_shift(T):
        raise ValueError("shift = %d leaves frames uncovered: the overlap mean needs shift <= T - T // 2 = %d" % (shift, max_overlap_shift(T)))
    halo = -(-T // shift) - 1
    can_split = max_windows >= 2 * halo + 1
    plan, g0 = [], 0
    while g0 < n_frames:
        u = int(np.searchsorted(utt_ptr, g0, side="right")) - 1
        w_lo = int(win_ptr[u]) + covering(g0 - int(utt_ptr[u]), int(lengths[u]), T, shift)[0]
        w_max = w_lo + max_windows - 1
        # every utterance whose last window is <= w_max fits whole; of the next one, the frames whose last covering window does
        v = int(np.searchsorted(win_ptr, w_max + 1, side="right")) - 1  # utterances [u, v) fit (win_ptr[v] <= w_max + 1)
        g1 = int(utt_ptr[v])
        if v < U and can_split and int(win_ptr[v]) <= w_max:
            k_max = w_max - int(win_ptr[v])  # (below W - 1, or the utterance would fit whole)
            g1 += max(0, min(int(lengths[v]), (k_max + 1) * shift - left(T)))
        if g1 <= g0:
            raise ValueError("max_windows = %d is too small: utterance %d has %d windows and may only be split with a halo of %d windows "
                             "on both sides (max_windows >= %d)" % (max_windows, v, int(win_ptr[v + 1] - win_ptr[v]), halo, 2 * halo + 1))
        ul = int(np.searchsorted(utt_ptr, g1 - 1, side="right")) - 1
        w_hi = int(win_ptr[ul]) + covering(g1 - 1 - int(utt_ptr[ul]), int(lengths[ul]), T, shift)[1]
        plan.append((w_lo, w_hi - w_lo + 1, g0, g1 - g0))
        g0 = g1
    return plan


# ------------------------------------------------------------------------------------------------------------ resident pool
class FramePool:
    """A corpus resident in HBM with its two CSR arrays: windows(w0, B) cuts dense windows (fhvae_frames_gather, MVN fused),
    overlap_mean(seg, w0, g0, G) puts per-window values back onto frames (fhvae_frames_overlap_mean, MVN undone).

    source  a list of (n_i, F) arrays, or a datasets.NumpyDataset / KaldiDataset (uploaded as ResidentSegmentPool uploads it:
            compressed Kaldi entries go up as the bytes on disk and are decoded by fhvae_kaldi_decompress).  Every utterance
            with n >= 1 is kept; an entry without rows raises ValueError naming its key.
    T       the model's segment length;  shift  frames between window centres
    mean, std  per-feature MVN statistics (default: the dataset's mvn_params; None: no normalisation)."""

    def __init__(self, source, T: int, shift: int = 1, mean=None, std=None, device="cuda"):
        import torch

        import hip_binding as hb

        self.hb, self.lib = hb, load_library()
        self.T, self.shift = int(T), int(shift)
        if self.T < 1 or self.shift < 1:
            raise ValueError("T = %d and shift = %d must be positive" % (T, shift))
        if hasattr(source, "load_seq"):
            self.keys = list(source.seq_keys)
            if mean is None and std is None and source.mvn_params is not None:
                mean, std = source.mvn_params["mean"], source.mvn_params["std"]
            self.pool, offs = self._upload_dataset(source, device)
        else:
            feats = [np.asarray(f, dtype=np.float32) for f in source]
            self.keys = [str(i) for i in range(len(feats))]
            if not feats:
                raise ValueError("no utterance to hold resident")
            for k, f in zip(self.keys, feats):
                self._check_rows(k, f.shape[0] if f.ndim == 2 else 0)
                if f.shape[1] != feats[0].shape[1]:
                    raise ValueError("utterance %s: %d columns, the first utterance has %d" % (k, f.shape[1], feats[0].shape[1]))
            offs = np.concatenate([[0], np.cumsum([f.shape[0] for f in feats])]).astype(np.int64)
            self.pool = torch.from_numpy(np.concatenate(feats, axis=0)).to(device)
        self.lengths, utt_ptr, win_ptr = _ptrs(np.diff(offs), self.shift)
        self.utt_ptr_host, self.win_ptr_host = utt_ptr, win_ptr
        self.num_utts, self.num_frames, self.num_windows = len(self.keys), int(utt_ptr[-1]), int(win_ptr[-1])
        self.F = int(self.pool.shape[1])
        dev = self.pool.device
        self.utt_ptr, self.win_ptr = torch.from_numpy(utt_ptr).to(dev), torch.from_numpy(win_ptr).to(dev)
        self.status = hip_ext.status_word(dev)
        if (mean is None) != (std is None):
            raise ValueError("mean and std come together")
        self.mean = self.std = self.inv_std = None
        if mean is not None:
            std64 = np.asarray(std, dtype=np.float64).reshape(-1)
            if std64.shape[0] != self.F or np.asarray(mean).size != self.F:
                raise ValueError("the MVN statistics have %d / %d entries for %d features" % (np.asarray(mean).size, std64.shape[0], self.F))
            self.mean = torch.from_numpy(np.asarray(mean, dtype=np.float32).reshape(-1).copy()).to(dev)
            self.std = torch.from_numpy(std64.astype(np.float32)).to(dev)
            self.inv_std = torch.from_numpy((1.0 / std64).astype(np.float32)).to(dev)  # (as ResidentSegmentPool)
        self._win_utt = None

    @staticmethod
    def _check_rows(key, rows):
        if rows < 1:
            raise ValueError("utterance %s has no frames (a 2-D matrix with at least one row is needed)" % key)

    def _upload_dataset(self, ds, device):
        import torch

        from datasets import KaldiDataset, ResidentSegmentPool

        if not self.keys:
            raise ValueError("no utterance to hold resident")
        for k, n in zip(self.keys, ds.seq_lens):
            self._check_rows(k, int(n))
        if isinstance(ds, KaldiDataset):
            self.CM_BATCH_BYTES = ResidentSegmentPool.CM_BATCH_BYTES
            pool, offs = ResidentSegmentPool._kaldi_pool(self, ds, device)  # (reads self.hb and self.CM_BATCH_BYTES only)
        else:
            feats = [ds.load_seq(i).astype(np.float32) for i in range(len(self.keys))]
            for k, f in zip(self.keys, feats):
                self._check_rows(k, f.shape[0] if f.ndim == 2 else 0)
            offs = np.concatenate([[0], np.cumsum([f.shape[0] for f in feats])]).astype(np.int64)
            pool = torch.from_numpy(np.concatenate(feats, axis=0)).to(device)
        for k, n in zip(self.keys, np.diff(offs)):  # (what the files hold, whatever len.scp says)
            self._check_rows(k, int(n))
        return pool, offs

    @property
    def win_utt(self):
        """(total windows,) int64 on the device: the utterance of every window (what the sorted mu2 sums are keyed by)."""
        import torch

        if self._win_utt is None:
            dev = self.pool.device
            counts = torch.from_numpy(np.diff(self.win_ptr_host)).to(dev)
            self._win_utt = torch.repeat_interleave(torch.arange(self.num_utts, device=dev), counts, output_size=self.num_windows)
        return self._win_utt

    def windows(self, w0: int, B: int, time_major: bool = False, batch_major: bool = True, normalise: bool = True):
        """Windows [w0, w0 + B) -> (B, T, F) (batch_major), (T, B, F) (time_major), or both as a pair."""
        import torch

        w0, B = int(w0), int(B)
        if not (batch_major or time_major):
            raise ValueError("windows: ask for batch_major, time_major or both")
        if w0 < 0 or B < 0 or w0 + B > self.num_windows:
            raise ValueError("windows [%d, %d) lie outside the corpus' %d windows" % (w0, w0 + B, self.num_windows))
        dev = self.pool.device
        btf = torch.empty(B, self.T, self.F, device=dev, dtype=torch.float32) if batch_major else None
        tbf = torch.empty(self.T, B, self.F, device=dev, dtype=torch.float32) if time_major else None
        mvn = normalise and self.mean is not None
        p = self.hb._p
        self.hb._call("fhvae_frames_gather", p(self.pool), self.pool.shape[0], p(self.utt_ptr), p(self.win_ptr), self.num_utts, w0, B,
                      self.T, self.F, self.shift, p(self.mean) if mvn else None, p(self.inv_std) if mvn else None, p(btf), p(tbf),
                      p(self.status))
        return (btf, tbf) if (batch_major and time_major) else (btf if batch_major else tbf)

    def overlap_mean(self, seg, w0: int, g0: int, G: int, out=None, denormalise: bool = True):
        """seg (B, T, F): per-window values of windows [w0, w0 + B) -> (G, F): the overlap mean for corpus frames [g0, g0 + G),
        then * std + mean.  Every covering window of those frames must lie in [w0, w0 + B) (chunk_plan's chunks do)."""
        import torch

        hb = self.hb
        hb._need_gpu(seg, out)
        hb._want("overlap_mean", "seg", seg, torch.float32, shape=(None, self.T, self.F))
        w0, g0, G, B = int(w0), int(g0), int(G), int(seg.shape[0])
        if self.shift > max_overlap_shift(self.T):
            raise ValueError("shift = %d leaves frames uncovered: the overlap mean needs shift <= T - T // 2 = %d"
                             % (self.shift, max_overlap_shift(self.T)))
        if w0 < 0 or w0 + B > self.num_windows or g0 < 0 or G < 0 or g0 + G > self.num_frames:
            raise ValueError("windows [%d, %d) / frames [%d, %d) lie outside the corpus (%d windows, %d frames)"
                             % (w0, w0 + B, g0, g0 + G, self.num_windows, self.num_frames))
        if out is None:
            out = torch.empty(G, self.F, device=seg.device, dtype=torch.float32)
        hb._want("overlap_mean", "out", out, torch.float32, shape=(G, self.F))
        mvn = denormalise and self.mean is not None
        p = hb._p
        hb._call("fhvae_frames_overlap_mean", p(seg), w0, B, p(self.utt_ptr), p(self.win_ptr), self.num_utts, g0, G, self.T, self.F,
                 self.shift, p(self.mean) if mvn else None, p(self.std) if mvn else None, p(out), p(self.status))
        return out

    def check(self):
        """Reads the status word (one host sync) and raises on what the kernels refused."""
        hip_ext.check_status("frame kernels", self.status, ((FRAMES_BAD_PTR, "utt_ptr / win_ptr are inconsistent"),
                                                            (FRAMES_BAD_RANGE, "a frame's covering window lies outside the windows given")))

    def split_frames(self, rows):
        """(total frames, X) -> one (n_u, X) view per utterance."""
        return [rows[int(a):int(b)] for a, b in zip(self.utt_ptr_host[:-1], self.utt_ptr_host[1:])]

    def split_windows(self, rows):
        """(total windows, X) -> one (W_u, X) view per utterance."""
        return [rows[int(a):int(b)] for a, b in zip(self.win_ptr_host[:-1], self.win_ptr_host[1:])]


def pool_from_scp(data_format: str, feat_scp, len_scp, mvn_path, T: int, shift: int = 1, device="cuda") -> FramePool:
    """The corpus a --feat-scp / --len-scp pair names ("numpy" or "kaldi"), resident: every key kept (min_len 0), the MVN
    statistics of mvn_path.  What extract_latents.py and eval_model.py --abx-item work on."""
    from datasets import KaldiDataset, NumpyDataset

    Dataset = NumpyDataset if data_format == "numpy" else KaldiDataset
    ds = Dataset(feat_scp, len_scp, 0, mvn_path, T, shift, False)  # min_len 0: no key is dropped
    return FramePool(ds, T, shift, device=device)


# ------------------------------------------------------------------------------------------------------------ model drivers
def _check_model(model, pool):
    T = int(getattr(model, "seg_len", pool.T))
    if T != pool.T:
        raise ValueError("the pool cuts windows of %d frames, the model takes %d" % (pool.T, T))
    width = int(model.n_feat) if hasattr(model, "n_feat") else int(model.dec_gauss_layer.mulayer.out_features) // pool.T
    if width != pool.F:
        raise ValueError("the pool holds %d features per frame, the model takes %d" % (pool.F, width))


def encode_frames(model, pool: FramePool, batch_size: int = 16384):
    """-> (z1_mu (total windows, z1_dim), z2_mu (total windows, z2_dim), mu2 (U, z2_dim)), device tensors.  Latents are
    model.encode of each chunk's windows (z1 conditioned on the window's own z2 mean); mu2[u] = sum of the utterance's z2_mu /
    (W_u + ratio), the closed form of utils.estimate_mu2_dict over THESE windows, summed without float atomics
    (fhvae_mu2_accumulate_sorted: the windows arrive sorted by utterance).  Nothing is read back between chunks; one host sync
    at the end reads the status words."""
    import torch

    from utils import mu2_ratio

    hb = pool.hb
    _check_model(model, pool)
    dev = pool.pool.device
    z1 = torch.empty(pool.num_windows, model.z1_dim, device=dev, dtype=torch.float32)
    z2 = torch.empty(pool.num_windows, model.z2_dim, device=dev, dtype=torch.float32)
    est = hb.SortedMu2Estimator(pool.num_utts, model.z2_dim, dev)
    win_utt = pool.win_utt
    with torch.no_grad():
        for w0, B, _, _ in chunk_plan(pool.lengths, pool.T, pool.shift, batch_size, overlap=False):
            a, b = model.encode(pool.windows(w0, B))
            z1[w0:w0 + B], z2[w0:w0 + B] = a, b
            est.add(z2[w0:w0 + B], win_utt[w0:w0 + B])
        mu2 = torch.empty(pool.num_utts, model.z2_dim, device=dev, dtype=torch.float32)
        scratch = torch.empty(2, pool.num_utts, model.z2_dim, device=dev, dtype=torch.float32)  # (the table's Adam rows: none here)
        est.load_into(mu2, scratch[0], scratch[1], mu2_ratio(model))
    est.check()
    pool.check()
    return z1, z2, mu2


def corpus_rows(model, pool: FramePool, on, what, batch_size: int = 16384):
    """The (total frames, D) rows of a shift-1 pool that a corpus-level feature works on: "z1", encode_frames' frame-level z1
    (shift 1: row f is frame f); "feats", the normalised input.  `what` names the feature in the ValueError for any other `on`."""
    if on == "z1":
        return encode_frames(model, pool, batch_size)[0]
    if on == "feats":
        return pool.pool if pool.mean is None else (pool.pool - pool.mean) * pool.inv_std
    raise ValueError("%s on %r: one of z1, feats" % (what, on))


def convert_frames(model, pool: FramePool, z2=None, batch_size: int = 16384):
    """-> (total frames, F) un-normalised features, a device tensor: per chunk model.decode(z1_mu, z2) of the chunk's windows, then
    the overlap mean with the MVN undone.  z2: None (reconstruction: every window's own z2 mean), one (z2_dim,) vector for the
    whole corpus, or (U, z2_dim), one per utterance (e.g. rows of encode_frames' mu2)."""
    import torch

    _check_model(model, pool)
    if pool.shift > max_overlap_shift(pool.T):
        raise ValueError("shift = %d leaves frames uncovered: decoding back to frames needs shift <= T - T // 2 = %d"
                         % (pool.shift, max_overlap_shift(pool.T)))
    dev = pool.pool.device
    per_utt = None
    if z2 is not None:
        z2 = torch.as_tensor(z2).to(device=dev, dtype=torch.float32)
        if z2.dim() == 2 and z2.shape == (pool.num_utts, model.z2_dim):
            per_utt, win_utt = z2.contiguous(), pool.win_utt
        elif z2.shape != (model.z2_dim,):
            raise ValueError("z2 must be (%d,) or (%d, %d); got %s" % (model.z2_dim, pool.num_utts, model.z2_dim, tuple(z2.shape)))
    out = torch.empty(pool.num_frames, pool.F, device=dev, dtype=torch.float32)
    with torch.no_grad():
        for w0, B, g0, G in chunk_plan(pool.lengths, pool.T, pool.shift, batch_size, overlap=True):
            z1_mu, z2_mu = model.encode(pool.windows(w0, B))
            target = z2_mu if z2 is None else (per_utt[win_utt[w0:w0 + B]] if per_utt is not None else z2)
            x_mu = model.decode(z1_mu, target)[0].reshape(B, pool.T, pool.F)
            pool.overlap_mean(x_mu, w0, g0, G, out=out[g0:g0 + G])
    pool.check()
    return out
