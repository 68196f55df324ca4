"""tsne.py -- exact t-SNE maps of embeddings: the picture that goes with verification.py's number.

The FHVAE papers show 2-D t-SNE maps of the latents coloured by speaker: in a model that factorized, the per-sequence mu2 falls
into one island per speaker and the per-sequence mean of z1 does not.

This is exact t-SNE (every pair, no tree, no neighbour lists) without the dense (N, N) affinity matrix: the perplexity search
keeps three numbers per row (hip_binding.tsne_affinity: beta, m, Z) and every gradient pass recomputes p_ij from them inside
the all-pairs kernel (hip_binding.tsne_step, csrc/tsne.hip).  The descent is scikit-learn's (TSNE(method="exact")): gains,
momentum 0.5 and exaggeration 12 for the first `exaggeration_iters` iterations, then 0.8 and 1; learning rate max(N / 48, 50);
Y0 = 1e-4 RandomState(seed).randn(N, 2).
"""
from __future__ import annotations

import numpy as np

EXAGGERATION = 12.0


def check_params(n: int, perplexity: float, n_iter: int, exaggeration_iters: int = 250):
    """ValueError for what tsne() does not take (nothing is clamped)."""
    if n < 8:
        raise ValueError("t-SNE needs at least 8 rows, got N = %d" % n)
    if not (perplexity >= 1.0) or perplexity > (n - 1) / 3.0:
        raise ValueError("perplexity %g is outside [1, (N - 1) / 3 = %g] for N = %d rows" % (perplexity, (n - 1) / 3.0, n))
    if n_iter < 1:
        raise ValueError("n_iter %d must be at least 1" % n_iter)
    if exaggeration_iters < 0:
        raise ValueError("exaggeration_iters %d must not be negative" % exaggeration_iters)


def learning_rate(n: int) -> float:
    return max(n / 48.0, 50.0)


def initial_map(n: int, seed: int) -> np.ndarray:
    return (1e-4 * np.random.RandomState(seed).randn(n, 2)).astype(np.float32)


def tsne(emb, perplexity: float = 30.0, n_iter: int = 1000, seed: int = 0, exaggeration_iters: int = 250, device=None):
    """emb (N, D) embeddings (array or tensor, D <= 128) -> (Y (N, 2) float32 numpy, {"kl", "perplexity", "n_iter", "seed"}).

    "kl" is the KL divergence the last iteration's gradient pass saw (at the map before its update, as scikit-learn's
    kl_divergence_).  Runs on the GPU (no CPU fallback); the loop enqueues n_iter steps and reads back once."""
    import torch

    import hip_binding as hb

    if device is None:
        device = emb.device if isinstance(emb, torch.Tensor) and emb.is_cuda else torch.device("cuda:0")
    x = emb.detach().cpu().numpy() if isinstance(emb, torch.Tensor) else np.asarray(emb)
    if x.ndim != 2:
        raise ValueError("tsne takes (N, D) embeddings, got shape %s" % (x.shape,))
    n, d = x.shape
    if d < 1 or d > 128:
        raise ValueError("tsne takes 1 <= D <= 128 columns, got D = %d" % d)
    perplexity, n_iter, seed = float(perplexity), int(n_iter), int(seed)
    check_params(n, perplexity, n_iter, exaggeration_iters)
    x = x.astype(np.float32).astype(np.float64)
    x = (x - x.mean(axis=0)).astype(np.float32)  # the means in float64, one rounding: the expanded distance cancels less
    rows = torch.zeros(n, (d + 15) // 16 * 16, device=device, dtype=torch.float32)  # (the layout the kernels read in place)
    rows[:, :d] = torch.from_numpy(x).to(device)
    ws = hb.tsne_workspace(rows)
    beta, m, z = hb.tsne_affinity(rows, perplexity, ws=ws)
    y = torch.from_numpy(initial_map(n, seed)).to(device)
    v, g = torch.zeros_like(y), torch.ones_like(y)
    kl = torch.zeros(1, device=device, dtype=torch.float32)
    lr = learning_rate(n)
    for it in range(n_iter):
        a, mom = (EXAGGERATION, 0.5) if it < exaggeration_iters else (1.0, 0.8)
        hb.tsne_step(rows, beta, m, z, y, v, g, a, mom, lr, kl=kl if it == n_iter - 1 else None, ws=ws)
    return y.cpu().numpy(), {"kl": float(kl.item()), "perplexity": perplexity, "n_iter": n_iter, "seed": seed}


def scatter_png(path, Y, labels, title: str) -> bool:
    """One colour per label (labels < 0: grey), Agg backend -> False (and nothing written) without matplotlib."""
    try:
        import matplotlib
    except ImportError:
        return False
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    Y, labels = np.asarray(Y), np.asarray(labels)
    fig, ax = plt.subplots(figsize=(6, 6), dpi=120)
    known = labels >= 0
    if (~known).any():
        ax.scatter(Y[~known, 0], Y[~known, 1], s=6, c="0.7", linewidths=0)
    if known.any():
        ax.scatter(Y[known, 0], Y[known, 1], s=6, c=labels[known], cmap="nipy_spectral", linewidths=0)
    ax.set_title(title)
    ax.set_xticks([]), ax.set_yticks([])
    fig.savefig(path)
    plt.close(fig)
    return True
