"""vad.py -- the binding of include/fhvae_vad.h (csrc/vad.hip): energy voice-activity detection on the device.

  energy   one energy per frame of a batch of waveforms (centred RMS as the reference's librosa call, or Kaldi's snip-edges
           raw log energy)
  decide   the decision of every frame (threshold from the utterance's mean energy, context vote) and `rank`, the exclusive
           prefix count of the decisions over the batch: every voiced row's destination
  select   the voiced rows of a (frames, F) matrix, packed

All three take and return device tensors and only enqueue; the user-facing functions (lists of waveforms in, numpy out) are
features.energy_vad / kaldi_energy_vad / vad_decide.  The definitions are the header's.
"""
from __future__ import annotations

import ctypes as C

import hip_ext

#: mode of fhvae_vad_energy, its flag, and the bits of the int32 device status word (include/fhvae_vad.h, FHVAE_VAD_*)
VAD_RMS_CENTER, VAD_LOGE_SNIP = 0, 1
VAD_REMOVE_DC = 1
VAD_BAD_PTR, VAD_BAD_RANK = 1, 2
VAD_MAX_FRAME, VAD_MAX_CTX, VAD_CHUNK, VAD_TILE = 4096, 1024, 1024, 1024

_vp, _i64 = C.c_void_p, C.c_int64
#: the entry points of include/fhvae_vad.h: name -> (restype, argtypes).  They are exported from libfhvae_hip.so but are not
#: part of include/fhvae_hip.h (ABI 12 is unchanged), so they are bound from this table (hip_ext.load) and not in hip_binding.SIGNATURES
VAD_SIGNATURES = {
    "fhvae_vad_energy": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, C.c_int, C.c_int, _vp, _vp, _vp]),
    "fhvae_vad_ws_bytes": (_i64, [_i64, _i64]),
    "fhvae_vad_decide": (C.c_int, [_vp, _vp, _i64, _i64, C.c_double, C.c_double, _i64, C.c_float, _vp, _i64, _vp, _vp, _vp, _vp]),
    "fhvae_vad_select": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
}


def load_library():
    """hip_binding.load_library() with the VAD entry points bound (argtypes from VAD_SIGNATURES)."""
    return hip_ext.load(VAD_SIGNATURES)


def energy(wave, wave_ptr, frame_ptr, n_frames, frame_len, frame_shift, mode, flags, status):
    """fhvae_vad_energy: wave (n_samples,) f32, wave_ptr / frame_ptr (U + 1,) int64, status (1,) int32, all on the device
    -> energy (n_frames,) f32."""
    import torch

    import hip_binding as hb

    load_library()
    hb._need_gpu(wave, wave_ptr, frame_ptr, status)
    hb._want("vad_energy", "wave", wave, torch.float32)
    hb._want("vad_energy", "wave_ptr", wave_ptr, torch.int64)
    hb._want("vad_energy", "frame_ptr", frame_ptr, torch.int64, shape=tuple(wave_ptr.shape))
    hb._want("vad_energy", "status", status, torch.int32, contiguous=False)
    out = torch.empty(int(n_frames), dtype=torch.float32, device=wave.device)
    hb._call("fhvae_vad_energy", hb._p(wave), wave.numel(), hb._p(wave_ptr), hb._p(frame_ptr), wave_ptr.shape[0] - 1, int(n_frames),
             int(frame_len), int(frame_shift), int(mode), int(flags), hb._p(out), hb._p(status))
    return out


def decide(energy, frame_ptr, thr_abs, mean_scale, ctx, proportion, status):
    """fhvae_vad_decide: energy (n_frames,) f32 and frame_ptr (U + 1,) int64 on the device -> (vad (n_frames,) uint8,
    rank (n_frames + 1,) int64).  The workspace is allocated here."""
    import torch

    import hip_binding as hb

    lib = load_library()
    hb._need_gpu(energy, frame_ptr, status)
    hb._want("vad_decide", "energy", energy, torch.float32)
    hb._want("vad_decide", "frame_ptr", frame_ptr, torch.int64)
    hb._want("vad_decide", "status", status, torch.int32, contiguous=False)
    n, U = int(energy.numel()), int(frame_ptr.shape[0]) - 1
    nbytes = int(lib.fhvae_vad_ws_bytes(n, U))
    if nbytes < 0:
        raise ValueError("fhvae_vad_ws_bytes(%d, %d) = %d" % (n, U, nbytes))
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=energy.device)
    vad = torch.empty(n, dtype=torch.uint8, device=energy.device)
    rank = torch.zeros(n + 1, dtype=torch.int64, device=energy.device)  # (n == 0 launches nothing: rank = [0])
    hb._call("fhvae_vad_decide", hb._p(energy), hb._p(frame_ptr), U, n, float(thr_abs), float(mean_scale), int(ctx), float(proportion),
             hb._p(ws), nbytes, hb._p(vad), hb._p(rank), hb._p(status))
    return vad, rank


def select(rows, vad, rank, n_out, status):
    """fhvae_vad_select: rows (n_frames, F) f32, vad / rank of decide, n_out = rank[-1] as the caller read it -> (n_out, F)."""
    import torch

    import hip_binding as hb

    load_library()
    hb._need_gpu(rows, vad, rank, status)
    hb._want("vad_select", "rows", rows, torch.float32, shape=(int(vad.shape[0]), None))
    hb._want("vad_select", "vad", vad, torch.uint8)
    hb._want("vad_select", "rank", rank, torch.int64, shape=(int(vad.shape[0]) + 1,))
    hb._want("vad_select", "status", status, torch.int32, contiguous=False)
    out = torch.empty((int(n_out), int(rows.shape[1])), dtype=torch.float32, device=rows.device)
    hb._call("fhvae_vad_select", hb._p(rows), hb._p(vad), hb._p(rank), int(vad.shape[0]), int(rows.shape[1]), int(n_out), hb._p(out),
             hb._p(status))
    return out
