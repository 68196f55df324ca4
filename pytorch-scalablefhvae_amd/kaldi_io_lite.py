"""kaldi_io_lite.py -- the Kaldi containers the loaders need, without the kaldiio package: binary archives (ark) of
float and compressed matrices with their script files (scp), and the text length table feat-to-len writes.

A binary archive is a sequence of entries
    key, one space, "\\0B", the token "FM " (float32) or "DM " (float64), "\\4" + int32 rows, "\\4" + int32 cols,
    rows * cols little-endian values, row-major
or, compressed (what copy-feats --compress=true writes; layout and formulas of Kaldi's matrix/compressed-matrix.{h,cc}),
    key, one space, "\\0B", the token "CM ", "CM2 " or "CM3 ", float32 min_value, float32 range, int32 rows, int32 cols,
    CM:  cols headers of four uint16 (p0, p25, p75, p100), then cols * rows uint8 column-major
    CM2: rows * cols uint16 row-major          CM3: rows * cols uint8 row-major
and an scp line "key ARK_PATH:OFFSET" points at the "\\0" of the entry (what `ark,scp:` writes and kaldiio.load_mat seeks to).

Decoding, in float32 with one rounding per operation: u(w) = min_value + range * w / 65535; CM2 is u(w), CM3 is
min_value + range * b / 255, and a CM byte b of a column whose header decodes to P0, P25, P75, P100 = u(p0) .. u(p100) is
P0 + (P25 - P0) * b / 64 up to 64, P25 + (P75 - P25) * (b - 64) / 128 up to 192 and P75 + (P100 - P75) * (b - 192) / 63 above.
The device decode (fhvae_kaldi_decompress) evaluates the same operations in the same order: the two agree bit for bit.

  write_ark_scp(ark_path, scp_path, items, compress=None)   (key, matrix) pairs -> one archive and its scp
  compress_mat(m, method="auto")             (token, payload bytes) of a float32 matrix, Kaldi's automatic method
  load_mat("path:offset" | "path")           one matrix; FM, DM, CM, CM2 and CM3 read, text forms refused
  read_raw("path:offset" | "path")           (token, min_value, range, rows, cols, payload) without decoding
  read_ark(path)                             iterates (key, matrix) over a binary archive
  write_len_scp(path, items)                 "key nframes" per line (feat-to-len scp:... ark,t:...)
  write_vec_ark_scp(ark_path, scp_path, items)   (key, vector) pairs -> an archive of float vectors and its scp
  load_vec("path:offset" | "path") / read_vec_ark(path)   one float vector; iterates (key, vector)

A float vector entry (what compute-vad-decision writes as vad.ark) is
    key, one space, "\\0B", the token "FV " (float32) or "DV " (float64), "\\4" + int32 dim, dim little-endian values.

A compressed header with range <= 0, a non-finite min_value or range, or a non-positive size is refused.  Kaldi writes
an EMPTY compressed matrix as an all-zero header: it falls under the range <= 0 refusal (an utterance without frames
has no place in a corpus).

Not built: text archives, integer vectors, piped ("... |") script entries, Kaldi's fixed-range integer compression methods;
each is refused with a message that says which and where.
"""
from __future__ import annotations

import struct

import numpy as np

_TOKENS = {b"FM": np.dtype("<f4"), b"DM": np.dtype("<f8")}
_COMPRESSED = (b"CM", b"CM2", b"CM3")
METHODS = ("auto", "two-byte", "one-byte")
_F = np.float32
_INV_65535 = _F(1.52590218966964e-05)  # the constant of Kaldi's Uint16ToFloat


class CompressedMatrix:
    """A matrix already coded (features.compute_kaldi_fbank(compress=...) codes on the device): `token` "CM" | "CM2" |
    "CM3", `header` the 16 bytes (min_value, range, rows, cols), `payload` the bytes behind it.  write_ark_scp writes it as
    it is; len() is its number of rows."""

    __slots__ = ("token", "header", "payload")

    def __init__(self, token, header, payload):
        self.token, self.header, self.payload = str(token), bytes(header), bytes(payload)
        if self.token.encode() not in _COMPRESSED or len(self.header) != 16:
            raise ValueError("not a compressed matrix: token %r, %d header bytes" % (token, len(self.header)))
        if len(self.payload) != payload_size(self.token, *self.shape):
            raise ValueError("%s payload of %d bytes for a %d x %d matrix" % ((self.token, len(self.payload)) + self.shape))

    @property
    def shape(self):
        return struct.unpack("<ii", self.header[8:16])

    def __len__(self):
        return self.shape[0]

    def decode(self):
        mn, rg = struct.unpack("<ff", self.header[:8])
        return decompress(self.token, mn, rg, self.shape[0], self.shape[1], self.payload)


def payload_size(token, rows, cols):
    """Bytes behind the 16-byte header of a compressed `rows` x `cols` matrix."""
    return {"CM": cols * (8 + rows), "CM2": 2 * rows * cols, "CM3": rows * cols}[token]


# ---------------------------------------------------------------------------------------------------------------- decode
def decompress(token, min_value, rng, rows, cols, payload):
    """float32 (rows, cols) of a compressed payload: the module docstring's formulas, one float32 rounding per operation,
    in the order fhvae_kaldi_decompress uses."""
    mn, rg = _F(min_value), _F(rng)
    buf = np.frombuffer(payload, dtype=np.uint8)

    def u(w):
        return mn + (rg * w.astype(_F)) / _F(65535.0)

    if token == "CM2":
        return u(buf.view("<u2")).reshape(rows, cols)
    if token == "CM3":
        return (mn + (rg * buf.astype(_F)) / _F(255.0)).reshape(rows, cols)
    P = u(buf[:8 * cols].view("<u2")).reshape(cols, 4)
    b = buf[8 * cols:].reshape(cols, rows).T  # column-major on disk
    P0, P25, P75, P100 = (P[:, k][None, :] for k in range(4))
    bf = b.astype(_F)
    lo = P0 + ((P25 - P0) * bf) * _F(1.0 / 64)
    mid = P25 + ((P75 - P25) * (bf - _F(64.0))) * _F(1.0 / 128)
    hi = P75 + ((P100 - P75) * (bf - _F(192.0))) / _F(63.0)
    return np.ascontiguousarray(np.where(b <= 64, lo, np.where(b <= 192, mid, hi)), dtype=_F)


# ---------------------------------------------------------------------------------------------------------------- encode
def _quant(v, mn, rg, top):
    """Kaldi's FloatToUint16 / FloatToUint8: f = (v - mn) / range clamped to [0, 1]; trunc(double(float32(f * top)) + 0.499)."""
    f = np.clip((v - mn) / rg, _F(0.0), _F(1.0))
    return np.trunc((f * _F(top)).astype(np.float64) + 0.499).astype(np.int64)


def global_range(m):
    """(min_value, range) float32 of a float32 matrix: a constant matrix gets range 1 + |min|; a zero minimum is +0.0
    whichever zeros the matrix holds (numpy's min may return either), so the header does not depend on who computed it."""
    mn, mx = _F(m.min()) + _F(0.0), _F(m.max())
    if mx == mn:
        mx = mn + (_F(1.0) + np.abs(mn))
    return mn, _F(mx - mn)


def token_for(rows, method="auto"):
    if method not in METHODS:
        raise ValueError("compression method %r: one of %s" % (method, ", ".join(METHODS)))
    return "CM3" if method == "one-byte" else "CM2" if method == "two-byte" or rows <= 8 else "CM"


def compress_mat(m, method="auto"):
    """(token, payload) of the float32 matrix `m` (2-D, not empty, finite) by Kaldi's automatic method ("auto": CM above
    8 rows, else CM2), "two-byte" (CM2) or "one-byte" (CM3); the 16-byte header is header_bytes(m)."""
    m = np.ascontiguousarray(m, dtype=_F)
    if m.ndim != 2 or m.size == 0:
        raise ValueError("a compressed matrix is 2-D and not empty, got shape %s" % (m.shape,))
    if not np.isfinite(m).all():
        raise ValueError("NaN or Inf in a matrix to compress")
    rows, cols = m.shape
    token = token_for(rows, method)
    mn, rg = global_range(m)
    if token == "CM2":
        return token, _quant(m, mn, rg, 65535.0).astype("<u2").tobytes()
    if token == "CM3":
        return token, _quant(m, mn, rg, 255.0).astype(np.uint8).tobytes()
    s = np.sort(m, axis=0)
    q = rows // 4
    p0 = np.minimum(_quant(s[0], mn, rg, 65535.0), 65532)
    p25 = np.minimum(np.maximum(_quant(s[q], mn, rg, 65535.0), p0 + 1), 65533)
    p75 = np.minimum(np.maximum(_quant(s[3 * q], mn, rg, 65535.0), p25 + 1), 65534)
    p100 = np.maximum(_quant(s[rows - 1], mn, rg, 65535.0), p75 + 1)
    words = np.stack([p0, p25, p75, p100], axis=1)  # (cols, 4)
    P = mn + (rg * _INV_65535) * words.astype(_F)
    P0, P25, P75, P100 = (P[:, k][None, :] for k in range(4))

    def seg(base, lo, hi, scale, first, last):
        f = (m - lo) / (hi - lo)
        return np.clip(base + np.trunc((f * _F(scale)).astype(np.float64) + 0.5), first, last)

    with np.errstate(over="ignore", invalid="ignore"):
        b = np.where(m < P25, seg(0, P0, P25, 64.0, 0, 64),
                     np.where(m < P75, seg(64, P25, P75, 128.0, 64, 192), seg(192, P75, P100, 63.0, 192, 255)))
    return token, words.astype("<u2").tobytes() + np.ascontiguousarray(b.T).astype(np.uint8).tobytes()


def header_bytes(m):
    """The 16 bytes (min_value, range, rows, cols) that precede compress_mat's payload."""
    m = np.ascontiguousarray(m, dtype=_F)
    mn, rg = global_range(m)
    return struct.pack("<ffii", mn, rg, m.shape[0], m.shape[1])


def write_ark_scp(ark_path, scp_path, items, compress=None):
    """Writes every (key, matrix) of `items` to the binary archive `ark_path` and one "key ark_path:offset" line per entry
    to `scp_path`.  A matrix is 2-D and stored as float32, or with `compress` ("auto", "two-byte", "one-byte") coded by
    compress_mat; a CompressedMatrix is written as it is.  Returns the number of entries."""
    if compress is not None and compress not in METHODS:
        raise ValueError("compress=%r: None or one of %s" % (compress, ", ".join(METHODS)))
    count = 0
    with open(ark_path, "wb") as ark, open(scp_path, "w") as scp:
        for key, mat in items:
            key = str(key)
            if not key or any(c.isspace() for c in key):
                raise ValueError("%r is not a Kaldi key (empty or with blanks)" % key)
            if isinstance(mat, CompressedMatrix):
                entry = b"\0B" + mat.token.encode() + b" " + mat.header + mat.payload
            else:
                m = np.ascontiguousarray(mat, dtype="<f4")
                if m.ndim != 2:
                    raise ValueError("%s: a matrix is 2-D, got shape %s" % (key, m.shape))
                if compress is None:
                    entry = b"\0BFM " + b"\4" + struct.pack("<i", m.shape[0]) + b"\4" + struct.pack("<i", m.shape[1]) + m.tobytes()
                else:
                    try:
                        token, payload = compress_mat(m, compress)
                    except ValueError as e:
                        raise ValueError("%s: %s" % (key, e)) from None
                    entry = b"\0B" + token.encode() + b" " + header_bytes(m) + payload
            ark.write(key.encode("utf-8") + b" ")
            scp.write("%s %s:%d\n" % (key, ark_path, ark.tell()))
            ark.write(entry)
            count += 1
    return count


def _read_raw(fh, where):
    """(token, min_value, range, rows, cols, payload) of the matrix whose "\\0B" header starts at the current position of
    `fh`; for FM and DM min_value and range are None and the payload is the array of values."""
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
    if tok in _COMPRESSED:
        name = tok.decode()
        hdr = fh.read(16)
        if len(hdr) != 16:
            raise ValueError("%s: compressed matrix (%s) header cut short by the end of the file" % (where, name))
        mn, rg, rows, cols = struct.unpack("<ffii", hdr)
        if not (np.isfinite(mn) and np.isfinite(rg)):
            raise ValueError("%s: compressed matrix (%s) with a non-finite header (min_value %r, range %r)" % (where, name, mn, rg))
        if rg <= 0:
            raise ValueError("%s: compressed matrix (%s) with range %r <= 0 (an all-zero header is Kaldi's empty matrix, "
                             "which is not supported)" % (where, name, rg))
        if rows <= 0 or cols <= 0:
            raise ValueError("%s: compressed matrix (%s) of size %d x %d" % (where, name, rows, cols))
        need = payload_size(name, rows, cols)
        payload = fh.read(need)
        if len(payload) != need:
            raise ValueError("%s: compressed matrix (%s) payload cut short: the file ends %d bytes into the %d of a %d x %d matrix"
                             % (where, name, len(payload), need, rows, cols))
        return name, mn, rg, rows, cols, payload
    if tok not in _TOKENS:
        raise ValueError("%s: %r is not a matrix token (FM, DM, CM, CM2 or CM3)" % (where, tok.decode("latin-1")))
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
    return tok.decode(), None, None, rows, cols, np.frombuffer(raw, dtype=dt).reshape(rows, cols).astype(dt.newbyteorder("="))


def _read_matrix(fh, where):
    """The matrix whose "\\0B" header starts at the current position of `fh`."""
    token, mn, rg, rows, cols, payload = _read_raw(fh, where)
    return payload if mn is None else decompress(token, mn, rg, rows, cols, payload)


def _open_spec(rxfilename):
    spec = str(rxfilename).strip()
    if spec.endswith("|"):
        raise ValueError("%s: piped entries are not supported" % spec)
    path, sep, off = spec.rpartition(":")
    if not sep or not off.isdigit():
        path, off = spec, "0"
    return path, off


def load_mat(rxfilename):
    """The matrix an scp value names: "path:offset" (offset of the entry's "\\0B") or "path" (a file that starts there)."""
    path, off = _open_spec(rxfilename)
    with open(path, "rb") as fh:
        fh.seek(int(off))
        return _read_matrix(fh, "%s:%s" % (path, off))


def read_raw(rxfilename):
    """The entry an scp value names, not decoded: (token, min_value, range, rows, cols, payload bytes) for CM, CM2 and CM3;
    (token, None, None, rows, cols, values) for FM and DM."""
    path, off = _open_spec(rxfilename)
    with open(path, "rb") as fh:
        fh.seek(int(off))
        return _read_raw(fh, "%s:%s" % (path, off))


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


# ---------------------------------------------------------------------------------------------------------------- vectors
_VEC_TOKENS = {b"FV": np.dtype("<f4"), b"DV": np.dtype("<f8")}


def write_vec_ark_scp(ark_path, scp_path, items):
    """Writes every (key, vector) of `items` to the binary archive `ark_path` as a float32 vector ("FV ") and one
    "key ark_path:offset" line per entry to `scp_path` (compute-vad-decision's vad.ark / vad.scp).  Returns the number of entries."""
    count = 0
    with open(ark_path, "wb") as ark, open(scp_path, "w") as scp:
        for key, vec in items:
            key = str(key)
            if not key or any(c.isspace() for c in key):
                raise ValueError("%r is not a Kaldi key (empty or with blanks)" % key)
            v = np.ascontiguousarray(vec, dtype="<f4")
            if v.ndim != 1:
                raise ValueError("%s: a vector is 1-D, got shape %s" % (key, v.shape))
            ark.write(key.encode("utf-8") + b" ")
            scp.write("%s %s:%d\n" % (key, ark_path, ark.tell()))
            ark.write(b"\0BFV " + b"\4" + struct.pack("<i", v.shape[0]) + v.tobytes())
            count += 1
    return count


def _read_vector(fh, where):
    """The vector whose "\\0B" header starts at the current position of `fh`."""
    if fh.read(2) != b"\0B":
        raise ValueError("%s: not a binary Kaldi vector (text archives are not supported; write with ark, not ark,t)" % where)
    tok = fh.read(3)
    if len(tok) != 3 or tok[2:3] != b" " or tok[:2] not in _VEC_TOKENS:
        raise ValueError("%s: %r is not a vector token (FV or DV)" % (where, tok.decode("latin-1")))
    dims = fh.read(5)
    if len(dims) != 5 or dims[0:1] != b"\4":
        raise ValueError("%s: bad vector header" % where)
    dim = struct.unpack("<i", dims[1:5])[0]
    if dim < 0:
        raise ValueError("%s: negative vector size %d" % (where, dim))
    dt = _VEC_TOKENS[tok[:2]]
    raw = fh.read(dim * dt.itemsize)
    if len(raw) != dim * dt.itemsize:
        raise ValueError("%s: the file ends inside a vector of %d" % (where, dim))
    return np.frombuffer(raw, dtype=dt).astype(dt.newbyteorder("="))


def load_vec(rxfilename):
    """The float vector an scp value names: "path:offset" (offset of the entry's "\\0B") or "path"."""
    path, off = _open_spec(rxfilename)
    with open(path, "rb") as fh:
        fh.seek(int(off))
        return _read_vector(fh, "%s:%s" % (path, off))


def read_vec_ark(path):
    """Iterates (key, vector) over the binary archive of float vectors at `path`."""
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
            yield key.decode("utf-8"), _read_vector(fh, "%s:%d" % (path, fh.tell()))
