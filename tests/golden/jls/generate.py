"""Generator of charls.npz and charls_phantom{0,1}.npz: JPEG-LS streams written by CharLS 2.2 (libcharls through ctypes), the codec
behind GDCM's JPEG-LS support, with a SPIFF header as CharLS writes it.
  charls.npz          the 4 x 4 example of T.87 Annex H.3 (its scan bytes are asserted to be the standard's); CT-like images
                      (flat air, noisy body) of 40 x 48 at 12 bit, 33 x 301 at 16 bit and 40 x 48 at 8 bit, each at NEAR 0 and 2;
                      one with an LSE segment (T1, T2, T3, RESET = 9, 30, 100, 31); one 32 x 40 of full-range 16-bit noise
  charls_phantom{0,1}.npz  the streams of slices 4 and 11 of the 512 x 512 x 16 boa_hip.synthetic.ct_phantom (stored = HU + 1024,
                      12 bit), which the tests draw again rather than read
Per case NAME: source_NAME, stream_NAME, decoded_NAME (CharLS's own decode: the source when NEAR = 0, within NEAR otherwise),
params_NAME = (bits, NEAR, MAXVAL, T1, T2, T3, RESET; zeros where no LSE was asked for).
Run: python tests/golden/jls/generate.py [path of libcharls.so]"""
import ctypes as C
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
H3 = np.array([[0, 0, 90, 74], [68, 50, 43, 205], [64, 145, 145, 145], [100, 145, 145, 145]], dtype=np.uint8)
PHANTOM_Z = (4, 11)
H3_SCAN = bytes.fromhex("c000006c80208e01c00000574000006ee6000001bc18000005d800009160")


class FrameInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bits_per_sample", C.c_int32), ("component_count", C.c_int32)]


class PcParameters(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("maximum_sample_value", "threshold1", "threshold2", "threshold3", "reset_value")]


def load(path=None):
    cands = [path] if path else sorted(glob.glob(os.path.join(sys.prefix, "lib", "libcharls.so*")) +
                                       glob.glob("/usr/lib/*/libcharls.so*"))
    assert cands, "libcharls.so not found: pass its path"
    lib = C.CDLL(cands[0])
    for name in ("charls_jpegls_encoder_create", "charls_jpegls_decoder_create"):
        getattr(lib, name).restype = C.c_void_p
    return lib


def _ok(rc, what):
    assert rc == 0, f"{what}: charls error {rc}"


def charls_encode(lib, img, bits, near=0, lse=None):
    img = np.ascontiguousarray(img, dtype=np.uint8 if bits <= 8 else np.uint16)
    enc = C.c_void_p(lib.charls_jpegls_encoder_create())
    fi = FrameInfo(img.shape[1], img.shape[0], bits, 1)
    _ok(lib.charls_jpegls_encoder_set_frame_info(enc, C.byref(fi)), "frame info")
    _ok(lib.charls_jpegls_encoder_set_near_lossless(enc, C.c_int32(near)), "near")
    if lse:
        pc = PcParameters(*lse)
        _ok(lib.charls_jpegls_encoder_set_preset_coding_parameters(enc, C.byref(pc)), "preset coding parameters")
    size = C.c_size_t()
    _ok(lib.charls_jpegls_encoder_get_estimated_destination_size(enc, C.byref(size)), "size")
    buf = C.create_string_buffer(size.value + 1024)
    _ok(lib.charls_jpegls_encoder_set_destination_buffer(enc, buf, C.c_size_t(len(buf))), "destination")
    _ok(lib.charls_jpegls_encoder_write_standard_spiff_header(enc, C.c_int32(8), C.c_int32(0), C.c_uint32(1), C.c_uint32(1)), "spiff")
    _ok(lib.charls_jpegls_encoder_encode_from_buffer(enc, img.ctypes.data_as(C.c_void_p), C.c_size_t(img.nbytes), C.c_uint32(0)),
        "encode")
    n = C.c_size_t()
    _ok(lib.charls_jpegls_encoder_get_bytes_written(enc, C.byref(n)), "bytes written")
    lib.charls_jpegls_encoder_destroy(enc)
    return buf.raw[:n.value]


def charls_decode(lib, stream):
    dec = C.c_void_p(lib.charls_jpegls_decoder_create())
    src = C.create_string_buffer(stream, len(stream))
    _ok(lib.charls_jpegls_decoder_set_source_buffer(dec, src, C.c_size_t(len(stream))), "source")
    _ok(lib.charls_jpegls_decoder_read_header(dec), "header")
    fi = FrameInfo()
    _ok(lib.charls_jpegls_decoder_get_frame_info(dec, C.byref(fi)), "frame info")
    out = np.zeros((fi.height, fi.width), dtype=np.uint8 if fi.bits_per_sample <= 8 else np.uint16)
    _ok(lib.charls_jpegls_decoder_decode_to_buffer(dec, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes), C.c_uint32(0)), "decode")
    lib.charls_jpegls_decoder_destroy(dec)
    return out


def ct_like(rows, cols, bits, rng):
    yy, xx = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    body = ((yy - rows / 2) ** 2 / (rows * 0.4) ** 2 + (xx - cols / 2) ** 2 / (cols * 0.4) ** 2) < 1
    hu = np.where(body, 40 + rng.normal(0, 12, body.shape), -1000)               # flat air (runs), noisy tissue
    v = np.clip(np.round(hu), -1024, 3071) + 1024                                 # 0 .. 4095
    return (v.astype(np.int64) << (bits - 12) if bits >= 12 else v.astype(np.int64) >> (12 - bits)).astype(np.uint16)


def phantom_slices():
    """uint16 [16, 512, 512]: the seeded phantom, stored = HU + 1024."""
    sys.path[:0] = [os.path.join(ROOT, "body-and-organ-analysis_amd")]
    from boa_hip.synthetic import ct_phantom
    return (ct_phantom((512, 512, 16)).transpose(2, 1, 0).astype(np.int32) + 1024).astype(np.uint16)


def case(lib, out, name, img, bits, near=0, lse=None):
    stream = charls_encode(lib, img, bits, near, lse)
    dec = charls_decode(lib, stream).astype(np.uint16)
    err = int(np.abs(dec.astype(np.int64) - img.astype(np.int64)).max())
    assert err <= near, f"{name}: CharLS round trip off by {err} at NEAR {near}"
    out[f"source_{name}"] = np.asarray(img, dtype=np.uint16)
    out[f"stream_{name}"] = np.frombuffer(stream, dtype=np.uint8)
    out[f"decoded_{name}"] = dec
    out[f"params_{name}"] = np.array([bits, near] + list(lse or (0, 0, 0, 0, 0)), dtype=np.int32)
    return len(stream)


def main():
    lib = load(sys.argv[1] if len(sys.argv) > 1 else None)
    rng = np.random.default_rng(20261019)
    out, total = {}, 0
    total += case(lib, out, "h3", H3, 8)
    s = out["stream_h3"].tobytes()
    assert s[s.index(b"\xFF\xDA") + 10:-2] == H3_SCAN and s[-2:] == b"\xFF\xD9", "CharLS does not reproduce T.87 H.3"
    for rows, cols, bits in ((40, 48, 12), (33, 301, 16), (40, 48, 8)):
        img = ct_like(rows, cols, bits, rng)
        for near in (0, 2):
            total += case(lib, out, f"ct{bits}_{rows}x{cols}_near{near}", img, bits, near)
    total += case(lib, out, "lse", ct_like(40, 48, 12, rng), 12, 0, (4095, 9, 30, 100, 31))
    total += case(lib, out, "noise16", rng.integers(0, 1 << 16, (32, 40)).astype(np.uint16), 16)
    np.savez_compressed(os.path.join(HERE, "charls.npz"), **out)
    print(f"charls.npz: {len(out)} arrays, {total} stream bytes")

    vol = phantom_slices()
    for i, z in enumerate(PHANTOM_Z):
        big = {}
        assert int(vol[z].max()) < 4096
        total = case(lib, big, "phantom", vol[z], 12)
        # (NEAR 0: CharLS decodes to the source, asserted above, and the source is phantom_slice(z): the stream alone is kept)
        del big["decoded_phantom"], big["source_phantom"]
        np.savez_compressed(os.path.join(HERE, f"charls_phantom{i}.npz"), **big)
        print(f"charls_phantom{i}.npz: {total} stream bytes")


if __name__ == "__main__":
    main()
