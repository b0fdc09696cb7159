"""Regenerates tests/golden/extdata_ovr/ from the reference's bundled raster overviews:

    python tests/golden/make_geotiff_overviews.py <the reference's inst/extdata directory>

TWI.tif.ovr and slope.tif.ovr (tiled 128 x 128, deflate, INT2S, GDAL_NODATA, four overview levels) are cut down to
their north-west corner without decoding anything: level k keeps the tiles that cover the first ceil(W / 2^k) x
ceil(H / 2^k) cells (W x H below), its width and height become that window's, and every kept tile's compressed bytes
are copied verbatim.  The cut keeps what tests/test_geotiff_host.py exercises -- the files' own deflate streams, tag
types, NoData strings and directory chain, and edge tiles that reach past the image -- at a few hundred kB instead of
6.4 MB.  The .tfw sidecars are copied as they are (the window starts at the raster's origin).
"""
import os
import shutil
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "extdata_ovr")
W, H = 300, 200            # level-0 window (level 0 of the .ovr is 1632 x 1238)
SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 16: 8}      # TIFF type -> bytes per value (BYTE, ASCII, SHORT, LONG, LONG8)


def read_ifds(raw):
    assert raw[:4] == b"II*\x00", "classic little-endian TIFF expected"
    off = struct.unpack_from("<I", raw, 4)[0]
    ifds = []
    while off:
        n = struct.unpack_from("<H", raw, off)[0]
        tags = {}
        for e in range(n):
            tag, typ, cnt, val = struct.unpack_from("<HHII", raw, off + 2 + 12 * e)
            nb = SIZE[typ] * cnt
            data = raw[off + 2 + 12 * e + 8:off + 2 + 12 * e + 8 + nb] if nb <= 4 else raw[val:val + nb]
            tags[tag] = (typ, cnt, bytes(data))
        ifds.append(tags)
        off = struct.unpack_from("<I", raw, off + 2 + 12 * n)[0]
    return ifds


def values(entry):
    typ, cnt, data = entry
    return list(struct.unpack("<%d%s" % (cnt, {3: "H", 4: "I"}[typ]), data))


def cut(src, dst):
    raw = open(src, "rb").read()
    ifds = read_ifds(raw)
    body = bytearray(b"II*\x00\x00\x00\x00\x00")
    out_ifds = []
    for k, tags in enumerate(ifds):
        width, height = values(tags[256])[0], values(tags[257])[0]
        tw, th = values(tags[322])[0], values(tags[323])[0]
        across = -(-width // tw)
        w, h = min(width, -(-W // 2 ** k)), min(height, -(-H // 2 ** k))
        offs, cnts = values(tags[324]), values(tags[325])
        new_offs, new_cnts = [], []
        for r in range(-(-h // th)):
            for c in range(-(-w // tw)):
                t = r * across + c
                new_offs.append(len(body))
                new_cnts.append(cnts[t])
                body += raw[offs[t]:offs[t] + cnts[t]]
                if len(body) % 2:
                    body += b"\x00"
        tags = dict(tags)
        tags[256] = (3, 1, struct.pack("<H", w)) if tags[256][0] == 3 else (4, 1, struct.pack("<I", w))
        tags[257] = (3, 1, struct.pack("<H", h)) if tags[257][0] == 3 else (4, 1, struct.pack("<I", h))
        tags[324] = (4, len(new_offs), struct.pack("<%dI" % len(new_offs), *new_offs))
        tags[325] = (4, len(new_cnts), struct.pack("<%dI" % len(new_cnts), *new_cnts))
        out_ifds.append(tags)
    next_slot = []
    for k, tags in enumerate(out_ifds):
        # values longer than four bytes first, then the directory that points at them
        ext = {}
        for tag in sorted(tags):
            typ, cnt, data = tags[tag]
            if len(data) > 4:
                ext[tag] = len(body)
                body += data
                if len(body) % 2:
                    body += b"\x00"
        start = len(body)
        if k == 0:
            struct.pack_into("<I", body, 4, start)
        else:
            struct.pack_into("<I", body, next_slot[-1], start)
        body += struct.pack("<H", len(tags))
        for tag in sorted(tags):
            typ, cnt, data = tags[tag]
            field = struct.pack("<I", ext[tag]) if tag in ext else data.ljust(4, b"\x00")
            body += struct.pack("<HHI", tag, typ, cnt) + field
        next_slot.append(len(body))
        body += b"\x00\x00\x00\x00"
    with open(dst, "wb") as f:
        f.write(bytes(body))


def main():
    ref = sys.argv[1]
    os.makedirs(OUT, exist_ok=True)
    for name in ("TWI", "slope"):
        cut(os.path.join(ref, name + ".tif.ovr"), os.path.join(OUT, name + ".tif.ovr"))
        shutil.copyfile(os.path.join(ref, name + ".tfw"), os.path.join(OUT, name + ".tfw"))
        print(name, os.path.getsize(os.path.join(OUT, name + ".tif.ovr")), "bytes")


if __name__ == "__main__":
    main()
