"""The oracle of the FLAC tests: a scalar Python decoder of RFC 9639 (frames read one after the other, every bit by hand)
and a small encoder that emits exactly what it is told to.  Shares no code with flac_lite.py or the device decoder.

  decode(data)                 -> (samples int64 (n, channels), rate, bps, md5 of STREAMINFO); raises FlacError on anything wrong
  pcm_md5(samples, bps)        the MD5 the format defines (interleaved little-endian samples of ceil(bps / 8) bytes)
  Sub(...)                     how to code one subframe
  encode_frame(...)            one frame with its CRCs
  encode_stream(...)           a whole file: fLaC, STREAMINFO, frames
  stream_file(frames, ...)     fLaC + STREAMINFO around frame bytes made elsewhere (fixture B)
"""
import hashlib

import numpy as np

FIXTURE_A = bytes.fromhex(
    "664c6143" "80000022" "10001000" "00000f00" "000f0ac4" "42f00000" "00013e84" "b41807dc" "69030758" "6a3dad1a" "2e0f" "fff86918" "0000bf"
    "0358fd03" "128b" "aa9a")
FIXTURE_B = bytes.fromhex(
    "fff86998" "000f9912" "08670162" "3d144299" "8f5df70d" "6fe00c17" "caeb2100" "0ee7a77a" "24a1590c" "1217b603" "097b784f" "aa9a33d2"
    "85e070ad" "5b1b4851" "b4010d99" "d2cd1a68" "f1e6b810")
A_LEFT, A_RIGHT = [25588], [10416]
B_LEFT = [10372, 18041, 14942, 17876, 15627, 17899, 16242, 18077, 16824, 18263, 17295, -14418, -15201, -14508, -15195, -14818]
B_RIGHT = [6070, 10545, 8743, 10449, 9143, 10463, 9502, 10569, 9840, 10680, 10113, -8428, -8895, -8476, -8896, -8653]

RATES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
SIZES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}
FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


class FlacError(Exception):
    pass


def crc8(data):
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def crc16(data):
    c = 0
    for b in data:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


def pcm_md5(samples, bps):
    width = (bps + 7) // 8
    out = bytearray()
    for v in np.asarray(samples).reshape(-1).tolist():
        out += (v & ((1 << (8 * width)) - 1)).to_bytes(width, "little")
    return hashlib.md5(bytes(out)).digest()


# ------------------------------------------------------------------------------------------------------------------ decoder
class _Bits:
    def __init__(self, data, pos):
        self.d, self.p = data, pos * 8

    def get(self, n):
        v = 0
        for _ in range(n):
            if self.p >= 8 * len(self.d):
                raise FlacError("the stream ends inside a frame")
            v = (v << 1) | ((self.d[self.p >> 3] >> (7 - (self.p & 7))) & 1)
            self.p += 1
        return v

    def sget(self, n):
        v = self.get(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self):
        q = 0
        while self.get(1) == 0:
            q += 1
        return q


def _subframe(br, bs, bps):
    if br.get(1):
        raise FlacError("subframe padding bit")
    t = br.get(6)
    w = 0
    if br.get(1):
        w = br.unary() + 1
        if w >= bps:
            raise FlacError("wasted bits")
        bps -= w
    if t == 0:
        x = [br.sget(bps)] * bs
    elif t == 1:
        x = [br.sget(bps) for _ in range(bs)]
    else:
        if 8 <= t <= 12:
            order = t - 8
        elif t >= 32:
            order = t - 31
        else:
            raise FlacError("reserved subframe type %d" % t)
        if order > bs:
            raise FlacError("order above block size")
        x = [br.sget(bps) for _ in range(order)]
        shift = 0
        if t >= 32:
            prec = br.get(4) + 1
            if prec == 16:
                raise FlacError("precision 1111")
            shift = br.sget(5)
            if shift < 0:
                raise FlacError("negative shift")
            coef = [br.sget(prec) for _ in range(order)]
        else:
            coef = FIXED[order]
        method = br.get(2)
        if method > 1:
            raise FlacError("residual method")
        pb = 4 + method
        po = br.get(4)
        if bs % (1 << po) or (bs >> po) < order:
            raise FlacError("partition order")
        for part in range(1 << po):
            cnt = (bs >> po) - (order if part == 0 else 0)
            k = br.get(pb)
            if k == (1 << pb) - 1:
                n = br.get(5)
                res = [br.sget(n) for _ in range(cnt)]
            else:
                res = []
                for _ in range(cnt):
                    u = (br.unary() << k) | br.get(k)
                    res.append((u >> 1) ^ -(u & 1))
            for r in res:
                pred = sum(c * x[-1 - i] for i, c in enumerate(coef)) >> shift
                x.append(pred + r)
    return [v << w for v in x]


def decode(data):
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC")
    pos, si = 4, None
    while True:
        last, t, ln = data[pos] >> 7, data[pos] & 127, int.from_bytes(data[pos + 1:pos + 4], "big")
        if si is None:
            if t != 0:
                raise FlacError("no STREAMINFO")
            si = data[pos + 4:pos + 4 + ln]
        pos += 4 + ln
        if last:
            break
    min_block = int.from_bytes(si[0:2], "big")
    v = int.from_bytes(si[10:18], "big")
    rate, nch, bps, total, md5 = v >> 44, ((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1), si[18:34]
    chans = [[] for _ in range(nch)]
    while pos < len(data):
        start = pos
        br = _Bits(data, pos)
        if br.get(15) != 0x7FFC:
            raise FlacError("no sync at %d" % pos)
        strategy, bsc, rc, assign, ssc = br.get(1), br.get(4), br.get(4), br.get(4), br.get(3)
        if br.get(1) or bsc == 0 or rc == 15 or assign > 10 or ssc == 3:
            raise FlacError("reserved header field")
        f = br.get(8)
        ones = 0
        while ones < 8 and f & (0x80 >> ones):
            ones += 1
        if ones == 1 or ones == 8:
            raise FlacError("coded number")
        num = f & (0xFF >> (ones + 1)) if ones else f
        for _ in range(max(ones - 1, 0)):
            c = br.get(8)
            if c >> 6 != 2:
                raise FlacError("coded number continuation")
            num = (num << 6) | (c & 63)
        bs = {1: 192}.get(bsc) or (576 << (bsc - 2) if bsc <= 5 else br.get(8) + 1 if bsc == 6 else br.get(16) + 1 if bsc == 7 else 256 << (bsc - 8))
        frate = {v: k for k, v in RATES.items()}.get(rc) or (br.get(8) * 1000 if rc == 12 else br.get(16) if rc == 13 else br.get(16) * 10 if rc == 14 else rate)
        fbps = {v: k for k, v in SIZES.items()}.get(ssc, 32 if ssc == 7 else bps)
        if (frate, fbps, assign + 1 if assign < 8 else 2) != (rate, bps, nch):
            raise FlacError("header disagrees with STREAMINFO")
        hend = br.p >> 3
        if crc8(data[start:hend]) != br.get(8):
            raise FlacError("CRC-8")
        if num * (1 if strategy else min_block) != len(chans[0]):
            raise FlacError("frame position")
        side = {8: 1, 9: 0, 10: 1}.get(assign)
        sub = [_subframe(br, bs, bps + (1 if c == side else 0)) for c in range(nch)]
        if br.get(-br.p % 8):
            raise FlacError("padding")
        fend = br.p >> 3
        if crc16(data[start:fend]) != br.get(16):
            raise FlacError("CRC-16 of the frame at %d" % start)
        pos = fend + 2
        if assign == 8:
            sub[1] = [a - b for a, b in zip(*sub)]
        elif assign == 9:
            sub[0] = [a + b for a, b in zip(*sub)]
        elif assign == 10:
            mid = [(m << 1) | (s & 1) for m, s in zip(*sub)]
            sub = [[(m + s) >> 1 for m, s in zip(mid, sub[1])], [(m - s) >> 1 for m, s in zip(mid, sub[1])]]
        for c in range(nch):
            chans[c] += sub[c]
    if total and total != len(chans[0]):
        raise FlacError("sample total")
    return np.array(chans, dtype=np.int64).T.reshape(len(chans[0]), nch), rate, bps, md5


# ------------------------------------------------------------------------------------------------------------------ encoder
class _Out:
    def __init__(self):
        self.bits = []

    def put(self, v, n):
        v &= (1 << n) - 1 if n else 0
        self.bits += [(v >> (n - 1 - i)) & 1 for i in range(n)]

    def unary(self, q):
        self.bits += [0] * q + [1]

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def bytes(self):
        assert len(self.bits) % 8 == 0
        return bytes(int("".join(map(str, self.bits[i:i + 8])), 2) for i in range(0, len(self.bits), 8))


class Sub:
    """How to code one subframe.  kind: "constant", "verbatim", "fixed" (order 0..4) or "lpc" (coefs, precision, shift; order =
    len(coefs)).  wasted: low zero bits to strip.  method: 0 (4-bit Rice parameters) or 1 (5-bit).  part_order and params: one
    Rice parameter per partition (None: the best one), or ("esc", n) for an escape partition of raw n-bit residuals."""

    def __init__(self, kind="fixed", order=0, coefs=None, precision=None, shift=0, wasted=0, method=0, part_order=0, params=None):
        self.kind, self.order, self.coefs, self.precision, self.shift = kind, order, coefs, precision, shift
        self.wasted, self.method, self.part_order, self.params = wasted, method, part_order, params


def _fits(v, n):
    return n > 0 and -(1 << (n - 1)) <= v < (1 << (n - 1)) or (n == 0 and v == 0)


def _put_subframe(o, x, bps, s):
    bs = len(x)
    if s.wasted:
        assert all(v % (1 << s.wasted) == 0 for v in x), "wasted bits are not zero"
        x = [v >> s.wasted for v in x]
        bps -= s.wasted
    assert all(_fits(v, bps) for v in x), "sample outside %d bits" % bps
    coefs = list(s.coefs) if s.kind == "lpc" else FIXED[s.order] if s.kind == "fixed" else []
    order = len(coefs)
    o.put(0, 1)
    o.put({"constant": 0, "verbatim": 1, "fixed": 8 + order, "lpc": 31 + order}[s.kind], 6)
    o.put(1 if s.wasted else 0, 1)
    if s.wasted:
        o.unary(s.wasted - 1)
    if s.kind == "constant":
        assert len(set(x)) == 1
        o.put(x[0], bps)
        return
    if s.kind == "verbatim":
        for v in x:
            o.put(v, bps)
        return
    for v in x[:order]:
        o.put(v, bps)
    if s.kind == "lpc":
        assert all(_fits(c, s.precision) for c in coefs) and 1 <= s.precision <= 15 and 0 <= s.shift <= 15
        o.put(s.precision - 1, 4)
        o.put(s.shift, 5)
        for c in coefs:
            o.put(c, s.precision)
    shift = s.shift if s.kind == "lpc" else 0
    res = [x[n] - (sum(c * x[n - 1 - i] for i, c in enumerate(coefs)) >> shift) for n in range(order, bs)]
    assert all(_fits(r, 32) and r != -(1 << 31) for r in res), "residual outside 32 bits"
    pb, po = 4 + s.method, s.part_order
    assert bs % (1 << po) == 0 and (bs >> po) >= order
    o.put(s.method, 2)
    o.put(po, 4)
    at = 0
    for part in range(1 << po):
        cnt = (bs >> po) - (order if part == 0 else 0)
        r = res[at:at + cnt]
        at += cnt
        fold = [(v << 1) if v >= 0 else ((-v) << 1) - 1 for v in r]
        p = s.params[part] if s.params is not None else None
        if p is None:
            p = min(range((1 << pb) - 1), key=lambda k: sum((u >> k) + 1 + k for u in fold))
        if isinstance(p, tuple):
            o.put((1 << pb) - 1, pb)
            o.put(p[1], 5)
            for v in r:
                assert _fits(v, p[1]), "residual %d outside an escape of %d bits" % (v, p[1])
                o.put(v, p[1])
        else:
            assert 0 <= p < (1 << pb) - 1
            o.put(p, pb)
            for u in fold:
                o.unary(u >> p)
                o.put(u, p)


def _block_code(bs, force=None):
    """(4-bit code, trailing field (value, bits) or None) for block size bs; force: "8bit" or "16bit" use the explicit fields."""
    if force == "8bit":
        return 6, (bs - 1, 8)
    if force == "16bit":
        return 7, (bs - 1, 16)
    if bs == 192:
        return 1, None
    for c in range(2, 6):
        if bs == 576 << (c - 2):
            return c, None
    for c in range(8, 16):
        if bs == 256 << (c - 8):
            return c, None
    return (6, (bs - 1, 8)) if bs <= 256 else (7, (bs - 1, 16))


def _utf8(n):
    if n < 0x80:
        return bytes([n])
    for nb in range(2, 8):
        if n < 1 << (5 * nb + 1):
            first = ((0xFF << (8 - nb)) & 0xFF) | (n >> (6 * (nb - 1)))
            return bytes([first] + [0x80 | ((n >> (6 * i)) & 63) for i in range(nb - 2, -1, -1)])
    raise ValueError(n)


def encode_frame(chans, number, bps, rate, subs, stereo="indep", strategy=0, block_code=None, rate_code=None, size_code=None):
    """One frame.  chans: per channel the samples of the block (left, right for the stereo modes "left_side", "side_right",
    "mid_side"); number: the frame number (strategy 0) or the first sample's number (strategy 1); subs: a Sub per coded channel.
    rate_code: None (the table, else 0 = from STREAMINFO), or 0, 12, 13, 14 to force that form; size_code likewise (0)."""
    bs, nch = len(chans[0]), len(chans)
    coded, widths, assign = [list(c) for c in chans], [bps] * nch, nch - 1
    if stereo != "indep":
        left, right = chans
        side = [a - b for a, b in zip(left, right)]
        if stereo == "left_side":
            coded, widths, assign = [list(left), side], [bps, bps + 1], 8
        elif stereo == "side_right":
            coded, widths, assign = [side, list(right)], [bps + 1, bps], 9
        else:
            coded, widths, assign = [[(a + b) >> 1 for a, b in zip(left, right)], side], [bps, bps + 1], 10
    bc, bfield = _block_code(bs, block_code)
    rc = RATES.get(rate, 0) if rate_code is None else rate_code
    rfield = {12: (rate // 1000, 8), 13: (rate, 16), 14: (rate // 10, 16)}.get(rc)
    sc = SIZES.get(bps, 0) if size_code is None else size_code
    o = _Out()
    o.put(0x7FFC, 15)
    o.put(strategy, 1)
    o.put(bc, 4)
    o.put(rc, 4)
    o.put(assign, 4)
    o.put(sc, 3)
    o.put(0, 1)
    for b in _utf8(number):
        o.put(b, 8)
    for fld in (bfield, rfield):
        if fld:
            o.put(*fld)
    o.put(crc8(o.bytes()), 8)
    for x, w, s in zip(coded, widths, subs):
        _put_subframe(o, x, w, s)
    o.align()
    body = o.bytes()
    return body + crc16(body).to_bytes(2, "big")


def stream_file(frames, rate, nch, bps, total, min_block, max_block, md5=bytes(16), extra_blocks=()):
    """fLaC, STREAMINFO and `extra_blocks` ((type, payload) metadata blocks) in front of the frame bytes."""
    v = (rate << 44) | ((nch - 1) << 41) | ((bps - 1) << 36) | total
    si = min_block.to_bytes(2, "big") + max_block.to_bytes(2, "big") + bytes(6) + v.to_bytes(8, "big") + md5
    blocks = [(0, si)] + list(extra_blocks)
    out = b"fLaC"
    for i, (t, payload) in enumerate(blocks):
        out += bytes([(0x80 if i == len(blocks) - 1 else 0) | t]) + len(payload).to_bytes(3, "big") + payload
    return out + frames


def encode_stream(pcm, bps, rate, block=4096, subs=None, stereo="indep", strategy=0, block_code=None, rate_code=None, size_code=None,
                  blocks=None, extra_blocks=(), md5=True):
    """A whole file from pcm (n, channels).  block: the block size (the last frame is shorter when n is no multiple), or
    `blocks`: every frame's size (strategy 1 for sizes that vary).  subs: a Sub, a list of one per channel, or a function
    (frame index, channel) -> Sub; default fixed order 2 (order 0 in blocks shorter than 2)."""
    pcm = np.asarray(pcm, dtype=np.int64).reshape(len(pcm), -1)
    n, nch = pcm.shape
    sizes = list(blocks) if blocks is not None else [block] * (n // block) + ([n % block] if n % block else [])
    assert sum(sizes) == n
    frames, at = b"", 0
    for fi, bs in enumerate(sizes):
        chans = [pcm[at:at + bs, c].tolist() for c in range(nch)]
        if callable(subs):
            ss = [subs(fi, c) for c in range(nch)]
        elif isinstance(subs, Sub):
            ss = [subs] * nch
        elif subs is None:
            ss = [Sub("fixed", order=min(2, bs))] * nch
        else:
            ss = subs
        frames += encode_frame(chans, at if strategy else fi, bps, rate, ss, stereo, strategy, block_code, rate_code, size_code)
        at += bs
    # (a fixed-blocksize stream: min = max = the block size, whatever the last frame holds)
    lo, hi = (min(sizes[:-1] or sizes), max(sizes)) if strategy == 0 else (min(sizes), max(sizes))
    return stream_file(frames, rate, nch, bps, n, lo, hi, pcm_md5(pcm, bps) if md5 else bytes(16), extra_blocks)
