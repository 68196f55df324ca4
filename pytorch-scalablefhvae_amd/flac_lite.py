"""flac_lite.py -- the container side of a native FLAC file (RFC 9639, section 8), on the host in pure Python: the `fLaC`
marker, the metadata blocks and STREAMINFO.  The frames behind them are decoded on the device (csrc/flac.hip through
features.decode_flac); nothing here touches a sample.

  parse_flac(buf, where)  -> FlacInfo: sample rate, channels, bits per sample, total samples (0: unknown), minimum and
                             maximum block size, the 16-byte MD5 of the decoded audio, and the byte offset of the first frame

Refused with a ValueError that names `where` and the reason: a leading ID3v2 tag, an Ogg container, anything else that does
not start with `fLaC`, a first metadata block that is not STREAMINFO, more than 24 or fewer than 4 bits per sample, and a
file that ends inside the metadata its block headers announce.
"""
from __future__ import annotations

from collections import namedtuple

MAGIC = b"fLaC"
STREAMINFO_BYTES = 34
MAX_BPS, MIN_BPS = 24, 4

FlacInfo = namedtuple("FlacInfo", "sample_rate channels bps total_samples min_block max_block md5 first_frame")


def parse_flac(buf, where="<bytes>"):
    """`buf`: the whole file (bytes-like).  `where`: what to call it in an error message."""
    buf = memoryview(buf).cast("B") if not isinstance(buf, (bytes, bytearray)) else buf
    head = bytes(buf[:4])
    if head[:3] == b"ID3":
        raise ValueError("%s: starts with an ID3v2 tag, which is not part of FLAC; strip the tag" % where)
    if head == b"OggS":
        raise ValueError("%s: an Ogg container (Ogg FLAC is not supported); only native FLAC files" % where)
    if head != MAGIC:
        raise ValueError("%s: not a FLAC file (no fLaC marker)" % where)
    pos, info, first = 4, None, True
    while True:
        if pos + 4 > len(buf):
            raise ValueError("%s: truncated: the file ends at byte %d, inside its metadata" % (where, len(buf)))
        last, btype = buf[pos] >> 7, buf[pos] & 0x7F
        length = int.from_bytes(bytes(buf[pos + 1:pos + 4]), "big")
        pos += 4
        if pos + length > len(buf):
            raise ValueError("%s: truncated: metadata block type %d claims %d bytes at offset %d, the file has %d"
                             % (where, btype, length, pos, len(buf)))
        if first:
            if btype != 0 or length < STREAMINFO_BYTES:
                raise ValueError("%s: no STREAMINFO: the first metadata block has type %d and %d bytes" % (where, btype, length))
            b = bytes(buf[pos:pos + STREAMINFO_BYTES])
            v = int.from_bytes(b[10:18], "big")  # 20 bits rate, 3 channels - 1, 5 bps - 1, 36 total samples
            info = (v >> 44, ((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1), int.from_bytes(b[0:2], "big"),
                    int.from_bytes(b[2:4], "big"), b[18:34])
            first = False
        pos += length
        if last:
            break
    rate, ch, bps = info[0], info[1], info[2]
    if bps > MAX_BPS:
        raise ValueError("%s: %d bits per sample; at most %d are supported" % (where, bps, MAX_BPS))
    if bps < MIN_BPS:
        raise ValueError("%s: %d bits per sample; FLAC has at least %d" % (where, bps, MIN_BPS))
    return FlacInfo(*info, first_frame=pos)
