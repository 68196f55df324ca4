"""Oracle of Kaldi's compressed matrices (CM, CM2, CM3), written from the format description alone: scalar Python, `struct`
and numpy.float32 SCALARS for the encoder (one rounding per operation, no fused multiply-add), float64 for the decoder.
Shares no code with kaldi_io_lite.

  decode(token, min_value, range, rows, cols, payload) -> float64 (rows, cols), the formulas evaluated literally
  encode(m, method)  -> (token, header 16 bytes, payload bytes)
  entry(key, token, header, payload) -> the bytes of one archive entry
  tol(min_value, range) -> 2^-21 (|min_value| + range): eight half-ulps of float32 at the matrix's scale
"""
import math
import struct

import numpy as np

F = np.float32
C16 = F(1.52590218966964e-05)


def tol(min_value, rng):
    return 2.0 ** -21 * (abs(float(min_value)) + float(rng))


def payload_size(token, rows, cols):
    return {"CM": cols * (8 + rows), "CM2": 2 * rows * cols, "CM3": rows * cols}[token]


# ---------------------------------------------------------------------------------------------------------------- decode
def decode(token, min_value, rng, rows, cols, payload):
    mn, rg = float(min_value), float(rng)  # (the header's float32 values, exact in float64)
    assert len(payload) == payload_size(token, rows, cols)
    out = np.empty((rows, cols), dtype=np.float64)

    def u(w):
        return mn + rg * w / 65535.0

    if token == "CM2":
        words = struct.unpack("<%dH" % (rows * cols), payload)
        for i in range(rows):
            for j in range(cols):
                out[i, j] = u(words[i * cols + j])
        return out
    if token == "CM3":
        for i in range(rows):
            for j in range(cols):
                out[i, j] = mn + rg * payload[i * cols + j] / 255.0
        return out
    assert token == "CM"
    for j in range(cols):
        p0, p25, p75, p100 = (u(w) for w in struct.unpack_from("<4H", payload, 8 * j))
        col = payload[8 * cols + j * rows: 8 * cols + (j + 1) * rows]
        for i in range(rows):
            b = col[i]
            if b <= 64:
                out[i, j] = p0 + (p25 - p0) * b / 64.0
            elif b <= 192:
                out[i, j] = p25 + (p75 - p25) * (b - 64) / 128.0
            else:
                out[i, j] = p75 + (p100 - p75) * (b - 192) / 63.0
    return out


def column_levels(min_value, rng, words):
    """float64 (P0, P25, P75, P100) of one CM column header."""
    return tuple(float(min_value) + float(rng) * w / 65535.0 for w in words)


# ---------------------------------------------------------------------------------------------------------------- encode
def global_range(m):
    mn, mx = F(F(min(m.flat)) + F(0.0)), F(max(m.flat))  # a zero minimum is stored as +0.0, whichever zero min() met first
    if mx == mn:
        mx = F(mn + F(F(1.0) + F(abs(mn))))
    return mn, F(mx - mn)


def _q(v, mn, rg, top):
    f = F(F(v - mn) / rg)
    f = min(max(f, F(0.0)), F(1.0))
    return int(math.trunc(float(F(f * F(top))) + 0.499))


def q16(v, mn, rg):
    return _q(F(v), mn, rg, 65535.0)


def q8(v, mn, rg):
    return _q(F(v), mn, rg, 255.0)


def column_header(col, mn, rg):
    s = sorted(F(v) for v in col)
    n = len(s)
    q = n // 4
    p0 = min(q16(s[0], mn, rg), 65532)
    p25 = min(max(q16(s[q], mn, rg), p0 + 1), 65533)
    p75 = min(max(q16(s[3 * q], mn, rg), p25 + 1), 65534)
    p100 = max(q16(s[n - 1], mn, rg), p75 + 1)
    return p0, p25, p75, p100


def _level(mn, rg, w):
    return F(mn + F(F(rg * C16) * F(w)))


def _clamp(x, lo, hi):
    return min(max(x, lo), hi)


def byte_of(v, P0, P25, P75, P100):
    v = F(v)
    if v < P25:
        f = F(F(v - P0) / F(P25 - P0))
        return _clamp(int(math.trunc(float(F(f * F(64.0))) + 0.5)), 0, 64)
    if v < P75:
        f = F(F(v - P25) / F(P75 - P25))
        return _clamp(64 + int(math.trunc(float(F(f * F(128.0))) + 0.5)), 64, 192)
    f = F(F(v - P75) / F(P100 - P75))
    return _clamp(192 + int(math.trunc(float(F(f * F(63.0))) + 0.5)), 192, 255)


def token_for(rows, method):
    return {"auto": "CM" if rows > 8 else "CM2", "two-byte": "CM2", "one-byte": "CM3"}[method]


def encode(m, method="auto"):
    m = np.asarray(m, dtype=np.float32)
    rows, cols = m.shape
    token = token_for(rows, method)
    mn, rg = global_range(m)
    header = struct.pack("<ffii", mn, rg, rows, cols)
    if token == "CM2":
        return token, header, struct.pack("<%dH" % m.size, *(q16(v, mn, rg) for v in m.flat))
    if token == "CM3":
        return token, header, bytes(q8(v, mn, rg) for v in m.flat)
    heads, body = [], []
    for j in range(cols):
        words = column_header(m[:, j], mn, rg)
        heads.append(struct.pack("<4H", *words))
        P = [_level(mn, rg, w) for w in words]
        body.append(bytes(byte_of(v, *P) for v in m[:, j]))
    return token, header, b"".join(heads) + b"".join(body)


def entry(key, token, header, payload):
    return key.encode() + b" \0B" + token.encode() + b" " + header + payload
