"""Test-only JPEG 2000 helpers: reversible codestreams (lossless, or truncated by their layers) from OpenJPEG through Pillow (where Pillow imports; the GPU tests never
import it), signed streams built from unsigned ones, the committed fixtures of tests/golden/j2k, and DICOM slices / series that
wrap a codestream (ljpeg_writer.write_compressed_slice with a JPEG 2000 transfer syntax)."""
import glob
import io
import json
import os
import struct

import numpy as np

import ljpeg_writer as LW

J2K_LOSSLESS = "1.2.840.10008.1.2.4.90"
J2K = "1.2.840.10008.1.2.4.91"
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "golden", "j2k")


def have_pillow_j2k():
    try:
        from PIL import features
        return bool(features.check("jpg_2000"))
    except Exception:
        return False


def _ssiz_pos(stream: bytes) -> int:
    i = stream.index(b"\xFF\x51")
    return i + 2 + 2 + 2 + 32 + 2                 # marker, Lsiz, Rsiz, 8 x 4 bytes of sizes / origins, Csiz


def encode(x, *, jp2=False, **kw) -> bytes:
    """OpenJPEG (through Pillow) reversible codestream of x: uint8 -> P = 8, uint16 -> P = 16; kw: Pillow's JPEG 2000 options
    (lossless unless quality_layers ends in a layer other than 0)."""
    from PIL import Image
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint8:
        im = Image.fromarray(x, mode="L") if x.size else None
    elif x.dtype == np.uint16:
        im = Image.frombytes("I;16", (x.shape[1], x.shape[0]), x.astype("<u2").tobytes())
    else:
        raise TypeError(x.dtype)
    b = io.BytesIO()
    im.save(b, format="JPEG2000", no_jp2=not jp2, irreversible=False, **kw)
    return b.getvalue()


def encode_signed(s, bits, **kw) -> bytes:
    """A signed P-bit stream of s (P = bits, 8 or 16): the unsigned stream of u = s + 2^(P-1) with the sign bit of Ssiz set.
    Both carry the same coded data: the DC level shift is what removes the offset, and the QCD exponents depend on P only."""
    s = np.asarray(s).astype(np.int64)
    assert s.min() >= -(1 << (bits - 1)) and s.max() < (1 << (bits - 1))
    u = (s + (1 << (bits - 1))).astype(np.uint8 if bits == 8 else np.uint16)
    st = bytearray(encode(u, **kw))
    p = _ssiz_pos(st)
    assert st[p] == bits - 1
    st[p] |= 0x80
    return bytes(st)


def openjpeg_decode(stream: bytes) -> np.ndarray:
    """What OpenJPEG decodes (int64).  Pillow hands a signed component over shifted by 2^(P-1): that shift is undone here."""
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(stream))).astype(np.int64)
    ssiz = stream[_ssiz_pos(stream)] if stream[:2] == b"\xFF\x4F" else None
    if ssiz is not None and ssiz & 0x80:
        a -= 1 << (ssiz & 0x7F)
    return a


def load_fixtures():
    """The committed fixtures -> list of dicts: name, stream (bytes), source (int64 [rows][cols]), bits, signed; and decoded
    (int64, OpenJPEG's own decode) for the streams that are not lossless."""
    out = []
    phantoms = {}
    for path in sorted(glob.glob(os.path.join(FIXTURES, "*.npz"))):
        g = np.load(path)
        for k, m in enumerate(json.loads(str(g["meta"]))):
            if "noise16_seed" in m:
                src = np.random.default_rng(m["noise16_seed"]).integers(0, 1 << 16, (m["rows"], m["cols"]))
            elif "phantom" in m:
                from boa_hip.synthetic import ct_phantom
                p = m["phantom"]
                key = (tuple(p["shape"]), p["seed"])
                if key not in phantoms:
                    phantoms[key] = ct_phantom(key[0], seed=key[1]).transpose(2, 1, 0)
                src = phantoms[key][p["z"]].astype(np.int64) + p["offset"]
                if "crop" in p:
                    y0, x0 = p["crop"]
                    src = src[y0:y0 + m["rows"], x0:x0 + m["cols"]]
            else:
                src = g[f"source_{k}"].astype(np.int64)
            out.append(dict(m, stream=g[f"stream_{k}"].tobytes(), source=src, file=os.path.basename(path)))
            if f"decoded_{k}" in g.files:
                out[-1]["decoded"] = g[f"decoded_{k}"].astype(np.int64)
    return out


def expected(fx):
    """The uint16 output of the decoder for a fixture: the sample modulo 2^16.  The sample is the source for a lossless stream
    and what OpenJPEG decodes (`decoded`) for a truncated one."""
    return (np.asarray(fx.get("decoded", fx["source"])).astype(np.int64) & 0xFFFF).astype(np.uint16)


def write_slice(path, pixels, stream, *, transfer_syntax=J2K_LOSSLESS, **kw):
    """A DICOM slice whose PixelData is the encapsulated codestream `stream`."""
    LW.write_compressed_slice(path, pixels, stream, transfer_syntax=transfer_syntax, **kw)


def write_series(folder, volume_zyx_stored, streams, *, origin=(-100.0, -120.0, 50.0), dz=1.5, transfer_syntax=J2K_LOSSLESS,
                 name="IM%04d.dcm", **kw):
    """dicom_writer.write_series for JPEG 2000: slice z at origin + z * dz along +z, its PixelData the codestream streams[z]."""
    os.makedirs(folder, exist_ok=True)
    paths = []
    for z in range(len(volume_zyx_stored)):
        p = os.path.join(folder, name % z)
        write_slice(p, volume_zyx_stored[z], streams[z], transfer_syntax=transfer_syntax,
                    ipp=np.asarray(origin, dtype=float) + np.array([0.0, 0.0, z * dz]), instance=z + 1, **kw)
        paths.append(p)
    return paths


def stream_of(x, bits, signed, **kw):
    """Codestream of the stored values x (int) at P = bits: unsigned directly, signed through encode_signed."""
    if signed:
        return encode_signed(x, bits, **kw)
    return encode(np.asarray(x).astype(np.uint8 if bits == 8 else np.uint16), **kw)


def patch_marker(stream: bytes, marker: int, offset: int, value: int) -> bytes:
    """Set byte `offset` of the body (after the length field) of the first marker segment `marker` to `value`."""
    i = stream.index(struct.pack(">H", marker))
    st = bytearray(stream)
    st[i + 4 + offset] = value
    return bytes(st)


def patch_exponents(stream: bytes, exponent: int) -> bytes:
    """Every subband exponent of the QCD segment set to `exponent` (quantisation style 0: one byte per subband)."""
    i = stream.index(b"\xFF\x5C")
    ln = struct.unpack(">H", stream[i + 2:i + 4])[0]
    st = bytearray(stream)
    st[i + 5:i + 2 + ln] = bytes([exponent << 3]) * (ln - 3)
    return bytes(st)


def quant_header(stream: bytes):
    """(guard bits, subband exponents) of the QCD segment (quantisation style 0)."""
    i = stream.index(b"\xFF\x5C")
    ln = struct.unpack(">H", stream[i + 2:i + 4])[0]
    return stream[i + 4] >> 5, [b >> 3 for b in stream[i + 5:i + 2 + ln]]
