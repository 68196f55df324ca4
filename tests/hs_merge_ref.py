"""Numpy model of the block merge of distributed hierarchical sampling (csrc/hs.hip: fhvae_hs_pack_partials +
fhvae_mu2_merge_load_shard): the CPU tests check it against the definition, the GPU tests use it as the kernels' oracle."""
import numpy as np


def pack(zsum, count):
    """(K, D+1) f32: [zsum | count]."""
    return np.concatenate([np.asarray(zsum, np.float32), np.asarray(count, np.float32)[:, None]], axis=1)


def merge_rows_f32(parts, row0, row1, ratio):
    """The kernel's arithmetic in float32: rows [row0, row1) of sum_w parts[w] added in rank order from 0, the count column the
    same way, then sum / (count + ratio), 0 where the count is 0.  parts (W, K, D+1)."""
    parts = np.asarray(parts, np.float32)
    s = np.zeros((row1 - row0, parts.shape[2]), np.float32)
    for w in range(parts.shape[0]):
        s = (s + parts[w, row0:row1]).astype(np.float32)
    n = s[:, -1:]
    q = (s[:, :-1] / (n + np.float32(ratio))).astype(np.float32)
    return np.where(n > 0, q, np.float32(0)).astype(np.float32)


def merge_rows_f64(parts, row0, row1, ratio):
    """The same quantity in float64 (any order)."""
    s = np.asarray(parts, np.float64)[:, row0:row1].sum(axis=0)
    n = s[:, -1:]
    return np.where(n > 0, s[:, :-1] / (n + float(ratio)), 0.0)


def shard_rows(K, world, rank):
    """dist_shard.ShardCtx's rows of a rank: ceil(K / W) per rank, the last ones ragged or empty."""
    per = (K + world - 1) // world
    row0 = min(K, rank * per)
    return row0, min(K, row0 + per)
