"""Test-only helpers of the irreversible (9/7) JPEG 2000 tests: codestreams from OpenJPEG through Pillow with irreversible=True
(where Pillow imports; the GPU tests never import it), signed streams by the Ssiz patch of j2k_writer.encode_signed, the committed
fixtures of tests/golden/j2k97 (a stream and OpenJPEG's own decode of it), and the numpy model's decode of a fixture, computed once
and shared by the tests of a run."""
import glob
import io
import json
import os

import numpy as np

import j2k_writer as JW

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "golden", "j2k97")
_MODEL = {}


def encode(x, **kw) -> bytes:
    """OpenJPEG (through Pillow) irreversible codestream of x: uint8 -> P = 8, uint16 -> P = 16; kw: Pillow's JPEG 2000 options."""
    from PIL import Image
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint8:
        im = Image.fromarray(x)
    elif x.dtype == np.uint16:
        im = Image.frombytes("I;16", (x.shape[1], x.shape[0]), x.astype("<u2").tobytes())
    else:
        raise TypeError(x.dtype)
    b = io.BytesIO()
    im.save(b, format="JPEG2000", no_jp2=True, irreversible=True, **kw)
    return b.getvalue()


def stream_of(x, bits, signed, **kw) -> bytes:
    """Irreversible codestream of the stored values x at P = bits; signed: the unsigned stream of x + 2^(P-1) with the sign bit
    of Ssiz set (the DC level shift is what removes the offset; the quantisation steps depend on P only)."""
    x = np.asarray(x).astype(np.int64)
    if signed:
        assert x.min() >= -(1 << (bits - 1)) and x.max() < (1 << (bits - 1))
        x = x + (1 << (bits - 1))
    st = bytearray(encode(x.astype(np.uint8 if bits == 8 else np.uint16), **kw))
    if signed:
        p = JW._ssiz_pos(st)
        assert st[p] == bits - 1
        st[p] |= 0x80
    return bytes(st)


def phantom_source(p, rows, cols, cache={}):
    """The stored values a fixture's `phantom` entry describes (boa_hip.synthetic.ct_phantom slice z + offset, cropped)."""
    from boa_hip.synthetic import ct_phantom
    key = (tuple(p["shape"]), p["seed"])
    if key not in cache:
        cache[key] = ct_phantom(key[0], seed=key[1]).transpose(2, 1, 0)
    src = cache[key][p["z"]].astype(np.int64) + p["offset"]
    y0, x0 = p.get("crop", (0, 0))
    return src[y0:y0 + rows, x0:x0 + cols]


def load_fixtures():
    """The committed fixtures -> list of dicts: name, stream (bytes), rows, cols, bits, signed, options, openjpeg (its version),
    decoded (int64 [rows][cols]: OpenJPEG's own decode; for phantom frames the file holds decoded - source)."""
    out = []
    for path in sorted(glob.glob(os.path.join(FIXTURES, "*.npz"))):
        g = np.load(path)
        for k, m in enumerate(json.loads(str(g["meta"]))):
            if "phantom" in m:
                dec = phantom_source(m["phantom"], m["rows"], m["cols"]) + g[f"residual_{k}"].astype(np.int64)
            else:
                dec = g[f"decoded_{k}"].astype(np.int64)
            out.append(dict(m, stream=g[f"stream_{k}"].tobytes(), decoded=dec, file=os.path.basename(path)))
    return out


def expected(fx):
    """The uint16 output of the decoder for a fixture: OpenJPEG's sample modulo 2^16."""
    return (fx["decoded"] & 0xFFFF).astype(np.uint16)


def parse(fx, name=None):
    from boa_hip import jpeg2000 as J
    return J.parse_frame(fx["stream"], rows=fx["rows"], cols=fx["cols"], name=name or fx["name"])


def model(fx):
    """(uint16 samples, float32 coefficient plane before the transform) of the numpy model for a fixture; computed once."""
    import j2k97_reference as M
    if fx["name"] not in _MODEL:
        fr = parse(fx)
        plane, ok = M.block_plane(fr)
        assert ok, fx["name"]
        _MODEL[fx["name"]] = (M.samples(M.synthesise(plane, fr.levels), fr.precision, fr.signed), plane)
    return _MODEL[fx["name"]]
