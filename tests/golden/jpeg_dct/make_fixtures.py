"""Writes the fixtures of this folder: DCT JPEG streams encoded by libjpeg-turbo together with libjpeg-turbo's own default
decode (JDCT_ISLOW) of every stream.
  p8.npz       P = 8 through Pillow (SOF0)
  p12.npz      P = 12 (SOF1) through the 12-bit entry points of the libjpeg-turbo 3.x that Pillow bundles, driven by ctypes
  phantom12.npz  two 512 x 512 slices of boa_hip.synthetic.ct_phantom (stored = HU + 1024) at P = 12, for tools/jpeg_dct_decode_time.py
Every file holds `names` and per name `stream_<name>` (uint8) and `decoded_<name>` (uint16 [rows, cols]); the phantom slices,
to stay small, hold `sha256_<name>` of the little-endian uint16 bytes of libjpeg-turbo's pixels in their place.
Needs Pillow >= 11 with its bundled libjpeg-turbo 3.x:  python tests/golden/jpeg_dct/make_fixtures.py\n(--probe: only check that the library can be driven this way, by exit status)"""
import ctypes as C
import glob
import hashlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))

_LIB = None
_KEEP = []


def lib12():
    """The bundled libjpeg-turbo as a plain CDLL, or None where Pillow or the 12-bit entry points are missing."""
    global _LIB
    if _LIB is None:
        try:
            import PIL
            cand = glob.glob(os.path.join(os.path.dirname(PIL.__file__), "..", "pillow.libs", "libjpeg-*.so.62.*"))
            L = C.CDLL(cand[0])
            L.jpeg12_read_scanlines, L.jpeg12_write_scanlines      # noqa: B018
            L.jpeg_std_error.restype = C.c_void_p
            L.jpeg_std_error.argtypes = [C.c_void_p]
            for fn in (L.jpeg_CreateCompress, L.jpeg_CreateDecompress):
                fn.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
            L.jpeg_mem_dest.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_ulong)]
            L.jpeg_mem_src.argtypes = [C.c_void_p, C.c_char_p, C.c_ulong]
            for fn in (L.jpeg_set_defaults, L.jpeg_finish_compress, L.jpeg_destroy_compress, L.jpeg_start_decompress,
                       L.jpeg_finish_decompress, L.jpeg_destroy_decompress):
                fn.argtypes = [C.c_void_p]
            L.jpeg_set_quality.argtypes = [C.c_void_p, C.c_int, C.c_int]
            L.jpeg_start_compress.argtypes = [C.c_void_p, C.c_int]
            L.jpeg_read_header.argtypes = [C.c_void_p, C.c_int]
            for fn in (L.jpeg12_write_scanlines, L.jpeg12_read_scanlines):
                fn.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint]
            _LIB = L
        except Exception:
            _LIB = False
    return _LIB or None


def _error_manager():
    """jpeg_std_error on a 1 KiB buffer with an error_exit that reports msg_code and ends the process (libjpeg's own would too)."""
    L = lib12()
    err = C.create_string_buffer(1024)
    L.jpeg_std_error(err)

    @C.CFUNCTYPE(None, C.c_void_p)
    def error_exit(cinfo):
        code = C.c_int.from_address(C.c_void_p.from_address(cinfo).value + 40).value
        sys.stderr.write(f"libjpeg error, msg_code {code}\n")
        os._exit(3)
    C.c_void_p.from_address(C.addressof(err)).value = C.cast(error_exit, C.c_void_p).value
    _KEEP.append((err, error_exit))
    return err


def _rows(x):
    x = np.ascontiguousarray(x, dtype=np.uint16)
    return x, [C.c_void_p(x[r].ctypes.data) for r in range(x.shape[0])]


def encode12(x, quality):
    """uint16 [rows, cols] samples < 4096 -> a P = 12 stream (SOF1) from jpeg12_write_scanlines."""
    L = lib12()
    err = _error_manager()
    cinfo = C.create_string_buffer(1024)
    C.c_void_p.from_address(C.addressof(cinfo)).value = C.addressof(err)
    L.jpeg_CreateCompress(cinfo, 62, 520)
    out, size = C.c_void_p(), C.c_ulong()
    L.jpeg_mem_dest(cinfo, C.byref(out), C.byref(size))
    base = C.addressof(cinfo)
    x, rows = _rows(x)
    C.c_uint.from_address(base + 48).value = x.shape[1]
    C.c_uint.from_address(base + 52).value = x.shape[0]
    C.c_int.from_address(base + 56).value = 1
    C.c_int.from_address(base + 60).value = 1                      # JCS_GRAYSCALE
    L.jpeg_set_defaults(cinfo)
    C.c_int.from_address(base + 72).value = 12                     # data_precision (jpeg_set_defaults resets it to 8)
    L.jpeg_set_quality(cinfo, quality, 0)
    L.jpeg_start_compress(cinfo, 1)
    for r in rows:
        assert L.jpeg12_write_scanlines(cinfo, C.byref(r), 1) == 1
    L.jpeg_finish_compress(cinfo)
    data = C.string_at(out.value, size.value)
    L.jpeg_destroy_compress(cinfo)
    return data


def decode12(stream, rows, cols):
    """libjpeg-turbo's default decode of a P = 12 stream -> uint16 [rows, cols]."""
    L = lib12()
    err = _error_manager()
    cinfo = C.create_string_buffer(1024)
    C.c_void_p.from_address(C.addressof(cinfo)).value = C.addressof(err)
    L.jpeg_CreateDecompress(cinfo, 62, 632)
    L.jpeg_mem_src(cinfo, stream, len(stream))
    L.jpeg_read_header(cinfo, 1)
    L.jpeg_start_decompress(cinfo)
    out, ptrs = _rows(np.zeros((rows, cols), dtype=np.uint16))
    for r in ptrs:
        assert L.jpeg12_read_scanlines(cinfo, C.byref(r), 1) == 1
    L.jpeg_finish_decompress(cinfo)
    L.jpeg_destroy_decompress(cinfo)
    return out


def encode8(x, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(x, dtype=np.uint8)).save(b, format="JPEG", **kw)
    return b.getvalue()


def decode8(stream):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(stream))).astype(np.uint16)


def smooth(shape, P, seed):
    """A CT-like test image: an ellipse of textured tissue on an empty background, samples < 2^P."""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    yy, xx = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    body = ((yy - rows / 2) ** 2 / (rows * 0.4) ** 2 + (xx - cols / 2) ** 2 / (cols * 0.4) ** 2) < 1
    v = np.where(body, 0.27 + 0.05 * np.sin(xx / 3.0) + rng.normal(0, 0.02, shape), 0.01) * (1 << P)
    return np.clip(np.round(v), 0, (1 << P) - 1).astype(np.uint16)


def has_16bit_dqt(stream):
    i = stream.index(b"\xFF\xDB")
    return stream[i + 4] >> 4 == 1


def main():
    assert lib12(), "Pillow with a libjpeg-turbo 3.x that exports the 12-bit entry points is needed"
    rng = np.random.default_rng(20261019)
    p8 = {"64x64_q75": encode8(smooth((64, 64), 8, 1), quality=75),
          "37x51_q30": encode8(smooth((37, 51), 8, 2), quality=30),
          "noise_q100": encode8(rng.integers(0, 2, (40, 48)) * 255, quality=100),
          "optimize_q85": encode8(smooth((48, 56), 8, 3), quality=85, optimize=True)}
    _save("p8.npz", {k: (v, decode8(v)) for k, v in p8.items()})
    q = 30
    while not has_16bit_dqt(encode12(smooth((37, 51), 12, 5), q)):
        q -= 5
    x12 = {"24x40_q90": (smooth((24, 40), 12, 4), 90), f"37x51_q{q}_dqt16": (smooth((37, 51), 12, 5), q),
           "noise_q100": (rng.integers(0, 2, (40, 48)) * 4095, 100)}
    p12 = {}
    for name, (x, quality) in x12.items():
        s = encode12(x, quality)
        p12[name] = (s, decode12(s, *x.shape))
    _save("p12.npz", p12)
    sys.path.insert(0, os.path.join(ROOT, "body-and-organ-analysis_amd"))
    from boa_hip.synthetic import ct_phantom
    vol = ct_phantom((512, 512, 64)).transpose(2, 1, 0).astype(np.int64) + 1024
    ph = {}
    for z in (24, 40):
        s = encode12(vol[z].astype(np.uint16), 90)
        ph[f"512x512_ct_phantom_z{z}_q90"] = (s, decode12(s, 512, 512))
    _save("phantom12.npz", ph, digest=True)


def _save(name, items, digest=False):
    out = {"names": np.array(list(items))}
    for k, (stream, decoded) in items.items():
        out["stream_" + k] = np.frombuffer(stream, dtype=np.uint8)
        if digest:
            out["sha256_" + k] = np.array(hashlib.sha256(decoded.astype("<u2").tobytes()).hexdigest())
        else:
            out["decoded_" + k] = decoded.astype(np.uint16)
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path), "bytes;", ", ".join(f"{k}: {len(v[0])} B" for k, v in items.items()))


def probe():
    """Exit status 0 when the 12-bit entry points work with the struct sizes and offsets used above (a library of another
    layout ends the process through error_exit: callers run this in a child process before they rely on encode12 / decode12)."""
    if not lib12():
        return 1
    x = smooth((8, 16), 12, 0)
    s = encode12(x, 90)
    ok = s[:2] == b"\xFF\xD8" and b"\xFF\xC1" in s and decode12(s, 8, 16).shape == (8, 16) and decode8(encode8(x >> 4)).shape == (8, 16)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(probe() if sys.argv[1:] == ["--probe"] else main())
