"""The grid arithmetic of the matrix-core K5 kernels (csrc/disc.hip: mfma_chunk, onepass_group_bytes), mirrored in Python for the tests that size workspaces
by it.  No imports: CPU and GPU tests share it."""


def cdiv(a, b):
    return -(-a // b)


def mfma_chunk(nx, ny, target):
    """Streamed rows per workgroup for about `target` workgroups (mfma_chunk)."""
    want = cdiv(target, cdiv(nx, 256))
    return max(64, cdiv(cdiv(ny, want), 64) * 64)


def group_bytes(tiles, B, S, D):
    """Workspace of the one-pass backward for query groups of `tiles` 256-query tiles (onepass_group_bytes)."""
    rows = min(B, tiles * 256)
    nchunks = cdiv(S, mfma_chunk(rows, S, 512))
    return (nchunks * rows * D + tiles * S * (D + 1)) * 4
