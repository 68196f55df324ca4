"""numpy oracles of the data, layout and exchange entry points (csrc/data.hip, the layout utilities, K4's gather, the final loss
and the row shard's pack / unpack helpers of csrc/loss.hip), written from the comments of include/fhvae_hip.h and the
reference lines they cite -- plain loops and index arithmetic, no torch on the compared path.  tests/test_glue_cpu.py checks
each against an independent torch-CPU expression; tests/test_glue_gpu.py compares the kernels with them."""
import numpy as np

F32 = np.float32


def segment_gather_ref(pool, start, T, mean=None, inv_std=None):
    """(B,T,F) float32 batch, its (T,B,F) twin and the oob bit.  Frame start[b] + t of the pool (datasets.py:214-223); a frame
    outside [0, pool_frames) is a row of zeros, also with mean / inv_std given; apply_mvn (datasets.py:100-105) is float32
    (x - mean) * inv_std, two float32 operations."""
    pool_frames, F = pool.shape
    B = len(start)
    btf = np.zeros((B, T, F), F32)
    tbf = np.zeros((T, B, F), F32)
    oob = 0
    for b in range(B):
        for t in range(T):
            fr = int(start[b]) + t
            if fr < 0 or fr >= pool_frames:
                oob = 1
                continue
            row = pool[fr].astype(F32)
            if mean is not None:
                row = (row - mean.astype(F32)).astype(F32) * inv_std.astype(F32)
            btf[b, t] = row
            tbf[t, b] = row
    return btf, tbf, oob


def mu2_accumulate_ref(z, idx, S):
    """float64 sums of z rows per id, float64 sums of |z|, integer counts (utils.py:45-56); ids outside [0, S) are skipped."""
    D = z.shape[1]
    zsum, absum, cnt = np.zeros((S, D)), np.zeros((S, D)), np.zeros(S, np.int64)
    for n in range(z.shape[0]):
        s = int(idx[n])
        if s < 0 or s >= S:
            continue
        zsum[s] += z[n].astype(np.float64)
        absum[s] += np.abs(z[n].astype(np.float64))
        cnt[s] += 1
    return zsum, absum, cnt


def mu2_finalize_ref(zsum, cnt, ratio):
    """float32 zsum / (cnt + float32(ratio)), 0 where cnt == 0 (utils.py:57-59)."""
    zsum, cnt = zsum.astype(F32), cnt.astype(F32)
    out = np.zeros_like(zsum)
    for s in range(zsum.shape[0]):
        if cnt[s] > 0:
            out[s] = zsum[s] / F32(cnt[s] + F32(ratio))
    return out


def to_time_major_ref(x):
    """(B,T,F) -> (T,B,F): out[t, b, f] = x[b, t, f]."""
    B, T, F = x.shape
    out = np.empty((T, B, F), x.dtype)
    for b in range(B):
        for t in range(T):
            out[t, b] = x[b, t]
    return out


def bf16_rne(x):
    """float32 -> bf16 bit patterns (uint16), round to nearest, ties to even, on the integer bit pattern; denormals are rounded
    like every other value; every NaN becomes 0x7FC0 (compare NaNs with bf16_same: a device may quiet a payload differently)."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r[nan] = 0x7FC0
    return r.reshape(np.shape(x))


def bf16_is_nan(h):
    h = np.asarray(h, np.uint16)
    return (h & 0x7FFF) > 0x7F80


def gather_fwd_ref(table, idx, off):
    """mu2[b] = table[idx[b] - off] (simple_fhvae.py:53); rows outside the table are zeros and raise the oob bit."""
    S, D = table.shape
    out = np.zeros((len(idx), D), F32)
    oob = 0
    for b in range(len(idx)):
        s = int(idx[b]) - int(off)
        if s < 0 or s >= S:
            oob = 1
        else:
            out[b] = table[s]
    return out, oob


def loss_fwd_ref(lb, log_qy, alpha):
    """float64 -(mean(lb) + alpha * log_qy) (train_model.py:243-251), sum |lb|, and the nan bit: isnan(mean(lb))."""
    lb64 = lb.astype(np.float64)
    with np.errstate(invalid="ignore"):
        mean = lb64.sum() / lb64.shape[0]
        loss = -(mean + np.float64(F32(alpha)) * np.float64(F32(log_qy)))
    return loss, float(np.abs(lb64).sum()), int(np.isnan(mean))


def loss_bwd_ref(g, alpha, B):
    """float32 d_lower_bound element -g / float32(B) and d_log_qy = -alpha * g."""
    g = F32(g)
    return F32(-g) / F32(B), F32(-F32(alpha)) * g


def shard_pack_ref(q, idx):
    """(B, D+1) rows [q[b] | int32 bits of idx[b]] as raw uint32 words."""
    B, D = q.shape
    out = np.empty((B, D + 1), np.uint32)
    out[:, :D] = np.ascontiguousarray(q, F32).view(np.uint32)
    out[:, D] = idx.astype(np.int32).view(np.uint32)
    return out


def shard_unpack_ref(words):
    """raw uint32 (N, D+1) rows -> q as float32 (its words unchanged) and int64 idx = the last word read as int32."""
    D = words.shape[1] - 1
    q = np.ascontiguousarray(words[:, :D]).view(F32)
    idx = np.ascontiguousarray(words[:, D]).view(np.int32).astype(np.int64)
    return q, idx


def shard_bwd_pack_ref(dq_all, dq_scale, dmu2_local, own0, n_own, N, D):
    """(N, 2D) float32: [dq_all * dq_scale | dmu2_local rows at rows own0 .. own0 + n_own, zeros elsewhere]; a missing operand
    is zeros."""
    out = np.zeros((N, 2 * D), F32)
    if dq_all is not None:
        out[:, :D] = dq_all.astype(F32) * F32(dq_scale)
    if dmu2_local is not None:
        for j in range(n_own):
            out[own0 + j, D:] = dmu2_local[j]
    return out


def shard_bwd_unpack_ref(buf, own0, n_own):
    """dq of the local queries (n_own, D) and dmu2 of all queries (N, D)."""
    D = buf.shape[1] // 2
    dq = np.empty((n_own, D), F32)
    for j in range(n_own):
        dq[j] = buf[own0 + j, :D]
    return dq, np.array(buf[:, D:], F32)
