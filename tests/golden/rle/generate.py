"""Generator of packbits_libtiff.npz: the byte planes of two CT-like uint16 images (40 x 48, and 33 x 301 whose rows are longer than
one 128-byte run) encoded by libtiff's PackBits encoder (through Pillow) -- a third-party encoder whose strips are Annex G
segments: one strip per plane, every row encoded on its own.  Checked here: one strip, a plain PackBits decoder returns the source,
no 0x80 control (libtiff writes none, so the check reads every control of the chain).
Run: python tests/golden/rle/generate.py"""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def images():
    rng = np.random.default_rng(20261019)
    for rows, cols in ((40, 48), (33, 301)):
        yy, xx = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        body = ((yy - rows / 2) ** 2 / (rows * 0.4) ** 2 + (xx - cols / 2) ** 2 / (cols * 0.4) ** 2) < 1
        hu = np.where(body, 40 + rng.normal(0, 12, body.shape), -1000)           # flat air (long runs), noisy tissue (literals)
        yield (np.clip(np.round(hu), -1024, 3071) + 1024).astype(np.uint16)


def packbits_strips(plane):
    """uint8 [rows, cols] -> (the strips libtiff wrote, rows per strip)."""
    from PIL import Image, features
    assert features.check("libtiff"), "Pillow without libtiff"
    buf = io.BytesIO()
    Image.fromarray(plane).save(buf, format="TIFF", compression="packbits")
    raw = buf.getvalue()
    tif = Image.open(io.BytesIO(raw))
    assert tif.tag_v2[259] == 32773                                            # Compression = PackBits
    return [raw[o:o + n] for o, n in zip(tif.tag_v2[273], tif.tag_v2[279])], int(tif.tag_v2[278])


def unpack(strip, row_bytes, rows):
    """Plain PackBits, row by row as TIFF defines it -> (bytes, number of 0x80 controls met)."""
    out, p, noops = bytearray(), 0, 0
    for _ in range(rows):
        row = bytearray()
        while len(row) < row_bytes:
            c = strip[p]
            if c < 128:
                row += strip[p + 1:p + 2 + c]
                p += 2 + c
            elif c > 128:
                row += strip[p + 1:p + 2] * (257 - c)
                p += 2
            else:
                noops += 1
                p += 1
        assert len(row) == row_bytes, "a run crosses the row end"
        out += row
    assert p == len(strip)
    return bytes(out), noops


def main():
    out, total = {}, 0
    for i, img in enumerate(images()):
        out[f"source_{i}"] = img
        for k, shift in enumerate((8, 0)):                                      # plane 0 = the most significant byte
            plane = ((img >> shift) & 0xFF).astype(np.uint8)
            strips, rps = packbits_strips(plane)
            assert len(strips) == 1 and rps >= img.shape[0], "libtiff wrote more than one strip"
            got, noops = unpack(strips[0], img.shape[1], img.shape[0])
            assert got == plane.tobytes() and noops == 0
            out[f"strip_{i}_{k}"] = np.frombuffer(strips[0], dtype=np.uint8)
            total += len(strips[0])
    np.savez_compressed(os.path.join(HERE, "packbits_libtiff.npz"), **out)
    print(f"{len(out)} arrays, {total} strip bytes")


if __name__ == "__main__":
    main()
