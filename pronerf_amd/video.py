"""Motion-JPEG in an AVI container: JPEG files as they come from ``ops.JpegEncoder`` / ``ops.jpeg_encode_host``, a few RIFF headers around them.

    with MjpegAviWriter(path, W, H, fps) as v:
        v.add(jpeg_bytes)

The file: RIFF ``AVI `` { LIST ``hdrl`` { ``avih``, LIST ``strl`` { ``strh`` (``vids`` / ``MJPG``), ``strf`` (BITMAPINFOHEADER, compression ``MJPG``,
24 bit, 8 bit for gray frames) } }, LIST ``movi`` { one ``00dc`` chunk per frame, padded to even length }, ``idx1`` (every frame a key frame, offsets
relative to the ``movi`` tag) }.  Frame count, sizes and buffer hints are patched on ``close``.  OpenDML is not written: ``add`` refuses the frame
that would take the closed file past 2^31 - 2^20 bytes, and the file closed at that point is valid.  Nothing here looks into the frames."""
from __future__ import annotations

import struct
from fractions import Fraction

from ._lib import PnrfError

AVI_LIMIT = (1 << 31) - (1 << 20)
_AVIF_HASINDEX, _AVIIF_KEYFRAME = 0x10, 0x10


class MjpegAviWriter:
    def __init__(self, path, W, H, fps, gray=False, limit=AVI_LIMIT):
        W, H = int(W), int(H)
        rate = Fraction(fps).limit_denominator(1001) if fps else Fraction(0)
        if not (1 <= W <= 65535 and 1 <= H <= 65535) or rate <= 0:
            raise PnrfError(f'MjpegAviWriter: frames of {W} x {H} at {fps!r} per second (sides 1 .. 65535, a positive rate)')
        self.path, self.W, self.H, self.gray, self.limit = path, W, H, bool(gray), int(limit)
        self.rate, self.scale = rate.numerator, rate.denominator
        self.index, self.largest, self.closed = [], 0, False
        self.f = open(path, 'wb')
        self.f.write(self._head(0))
        self.movi = self.f.tell() - 4                       # where the 'movi' tag stands
        self.pos = self.f.tell()

    def _head(self, movi_bytes):
        n, W, H = len(self.index), self.W, self.H
        bits = 8 if self.gray else 24
        per_sec = (sum(s for _, s in self.index) * self.rate // (self.scale * n)) if n else 0
        avih = struct.pack('<14I', 1000000 * self.scale // self.rate, per_sec, 0, _AVIF_HASINDEX, n, 0, 1, self.largest, W, H, 0, 0, 0, 0)
        strh = struct.pack('<4s4sIHHIIIIIIII4H', b'vids', b'MJPG', 0, 0, 0, 0, self.scale, self.rate, 0, n, self.largest, 0xffffffff, 0, 0, 0, W, H)
        strf = struct.pack('<IiiHH4sIiiII', 40, W, H, 1, bits, b'MJPG', W * H * bits // 8, 0, 0, 0, 0)
        chunk = lambda tag, body: tag + struct.pack('<I', len(body)) + body
        strl = b'LIST' + struct.pack('<I', 4 + 8 + len(strh) + 8 + len(strf)) + b'strl' + chunk(b'strh', strh) + chunk(b'strf', strf)
        hdrl = b'LIST' + struct.pack('<I', 4 + 8 + len(avih) + len(strl)) + b'hdrl' + chunk(b'avih', avih) + strl
        movi = b'LIST' + struct.pack('<I', 4 + movi_bytes) + b'movi'
        riff = 4 + len(hdrl) + len(movi) + movi_bytes + 8 + 16 * n
        return b'RIFF' + struct.pack('<I', riff) + b'AVI ' + hdrl + movi

    def add(self, jpeg):
        """Appends one frame: the bytes of a JPEG file of the writer's size."""
        if self.closed:
            raise PnrfError('MjpegAviWriter: add after close')
        n = len(jpeg)
        if n < 4 or bytes(jpeg[:2]) != b'\xff\xd8':
            raise PnrfError('MjpegAviWriter: a frame has to be the bytes of a JPEG file')
        after = self.pos + 8 + n + (n & 1) + 8 + 16 * (len(self.index) + 1)
        if after > self.limit:
            raise PnrfError(f'MjpegAviWriter: frame {len(self.index)} would take {self.path} to {after} bytes, past {self.limit} (OpenDML is not written)')
        self.f.write(b'00dc' + struct.pack('<I', n))
        self.f.write(jpeg)
        if n & 1:
            self.f.write(b'\0')
        self.index.append((self.pos - self.movi, n))
        self.largest = max(self.largest, n)
        self.pos += 8 + n + (n & 1)

    def close(self):
        if self.closed:
            return
        self.closed = True
        self.f.write(b'idx1' + struct.pack('<I', 16 * len(self.index)))
        for off, n in self.index:
            self.f.write(struct.pack('<4sIII', b'00dc', _AVIIF_KEYFRAME, off, n))
        self.f.seek(0)
        self.f.write(self._head(self.pos - self.movi - 4))
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
