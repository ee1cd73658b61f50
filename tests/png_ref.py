"""a PNG reader for the tests, independent of chore_amd.utils.render_utils.write_png: zlib + the five row filters of the
PNG specification, 8-bit grey and RGB, no interlacing"""
import struct
import zlib

import numpy as np


def read_png(path):
    """-> (H,W) or (H,W,3) uint8"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG signature"
    pos, idat, head = 8, b"", None
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])
        assert crc == (zlib.crc32(tag + data) & 0xffffffff), "bad CRC in chunk %r" % tag
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", data)
        elif tag == b"IDAT":
            idat += data
        elif tag == b"IEND":
            break
        pos += 12 + n
    w, h, depth, colour, comp, filt, interlace = head
    assert depth == 8 and colour in (0, 2) and (comp, filt, interlace) == (0, 0, 0), head
    bpp = 3 if colour == 2 else 1
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * bpp)
    out = np.zeros((h, w * bpp), np.int64)
    for y in range(h):
        f, line = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(w * bpp, np.int64)
        if f == 0:
            out[y] = line
        elif f == 2:
            out[y] = (line + up) & 255
        else:
            for x in range(w * bpp):
                a = out[y, x - bpp] if x >= bpp else 0
                b, c = up[x], (up[x - bpp] if x >= bpp else 0)
                if f == 1:
                    pred = a
                elif f == 3:
                    pred = (a + b) // 2
                else:
                    assert f == 4, f
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                out[y, x] = (line[x] + pred) & 255
    out = out.astype(np.uint8)
    return out.reshape(h, w, 3) if colour == 2 else out.reshape(h, w)
