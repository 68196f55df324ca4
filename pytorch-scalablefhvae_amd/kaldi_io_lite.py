"""kaldi_io_lite.py -- the Kaldi containers the loaders need, without the kaldiio package: binary archives (ark) of
float matrices with their script files (scp), and the text length table feat-to-len writes.

A binary archive is a sequence of entries
    key, one space, "\\0B", the token "FM " (float32) or "DM " (float64), "\\4" + int32 rows, "\\4" + int32 cols,
    rows * cols little-endian values, row-major
and an scp line "key ARK_PATH:OFFSET" points at the "\\0" of the entry (what `ark,scp:` writes and kaldiio.load_mat seeks to).

  write_ark_scp(ark_path, scp_path, items)   (key, matrix) pairs -> one float32 archive and its scp
  load_mat("path:offset" | "path")           one matrix; FM and DM read, compressed (CM, CM2, CM3) and text forms refused
  read_ark(path)                             iterates (key, matrix) over a binary archive
  write_len_scp(path, items)                 "key nframes" per line (feat-to-len scp:... ark,t:...)

Not built: compressed matrices, text archives, vectors, piped ("... |") script entries; each is refused with a message
that says which and where.
"""
from __future__ import annotations

import struct

import numpy as np

_TOKENS = {b"FM": np.dtype("<f4"), b"DM": np.dtype("<f8")}


def write_ark_scp(ark_path, scp_path, items):
    """Writes every (key, matrix) of `items` (2-D, stored as float32) to the binary archive `ark_path` and one
    "key ark_path:offset" line per entry to `scp_path`.  Returns the number of entries."""
    count = 0
    with open(ark_path, "wb") as ark, open(scp_path, "w") as scp:
        for key, mat in items:
            key = str(key)
            if not key or any(c.isspace() for c in key):
                raise ValueError("%r is not a Kaldi key (empty or with blanks)" % key)
            m = np.ascontiguousarray(mat, dtype="<f4")
            if m.ndim != 2:
                raise ValueError("%s: a matrix is 2-D, got shape %s" % (key, m.shape))
            ark.write(key.encode("utf-8") + b" ")
            scp.write("%s %s:%d\n" % (key, ark_path, ark.tell()))
            ark.write(b"\0BFM " + b"\4" + struct.pack("<i", m.shape[0]) + b"\4" + struct.pack("<i", m.shape[1]))
            ark.write(m.tobytes())
            count += 1
    return count


def _read_matrix(fh, where):
    """The matrix whose "\\0B" header starts at the current position of `fh`."""
    head = fh.read(2)
    if head != b"\0B":
        raise ValueError("%s: not a binary Kaldi matrix (text archives are not supported; write with ark, not ark,t)" % where)
    tok = b""
    while not tok.endswith(b" "):
        c = fh.read(1)
        if not c or len(tok) > 8:
            raise ValueError("%s: no matrix token after the binary marker" % where)
        tok += c
    tok = tok[:-1]
    if tok in (b"CM", b"CM2", b"CM3"):
        raise ValueError("%s: compressed matrix (%s) is not supported; write it uncompressed (copy-feats --compress=false)"
                         % (where, tok.decode()))
    if tok not in _TOKENS:
        raise ValueError("%s: %r is not a float matrix token (FM or DM)" % (where, tok.decode("latin-1")))
    dims = fh.read(10)
    if len(dims) != 10 or dims[0:1] != b"\4" or dims[5:6] != b"\4":
        raise ValueError("%s: bad matrix header" % where)
    rows, cols = struct.unpack("<i", dims[1:5])[0], struct.unpack("<i", dims[6:10])[0]
    if rows < 0 or cols < 0:
        raise ValueError("%s: negative matrix size %d x %d" % (where, rows, cols))
    dt = _TOKENS[tok]
    raw = fh.read(rows * cols * dt.itemsize)
    if len(raw) != rows * cols * dt.itemsize:
        raise ValueError("%s: the file ends inside a %d x %d matrix" % (where, rows, cols))
    return np.frombuffer(raw, dtype=dt).reshape(rows, cols).astype(dt.newbyteorder("="))


def load_mat(rxfilename):
    """The matrix an scp value names: "path:offset" (offset of the entry's "\\0B") or "path" (a file that starts there)."""
    spec = str(rxfilename).strip()
    if spec.endswith("|"):
        raise ValueError("%s: piped entries are not supported" % spec)
    path, sep, off = spec.rpartition(":")
    if not sep or not off.isdigit():
        path, off = spec, "0"
    with open(path, "rb") as fh:
        fh.seek(int(off))
        return _read_matrix(fh, "%s:%s" % (path, off))


def read_ark(path):
    """Iterates (key, matrix) over the binary archive at `path`."""
    with open(path, "rb") as fh:
        while True:
            key = b""
            while True:
                c = fh.read(1)
                if not c:
                    if key.strip():
                        raise ValueError("%s: the file ends inside a key" % path)
                    return
                if c == b" ":
                    break
                key += c
            yield key.decode("utf-8"), _read_matrix(fh, "%s:%d" % (path, fh.tell()))


def write_len_scp(path, items):
    """`items`: (key, nframes) pairs -> "key nframes" per line."""
    with open(path, "w") as fh:
        for key, n in items:
            fh.write("%s %d\n" % (key, int(n)))
