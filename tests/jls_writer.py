"""Test-only JPEG-LS (ITU-T T.87) encoder in plain Python and DICOM wrapper, written from the standard.  JPEG-LS encoding is
deterministic, so `encode_scan` is pinned byte for byte against CharLS (tests/golden/jls); `encode` wraps the scan in the markers
SOI, [LSE], SOF55, SOS, EOI.  `write_slice` / `write_series` put the stream into DICOM files on top of dicom_writer."""
import os
import struct

import numpy as np

from dicom_writer import write_slice as _write_native
import ljpeg_writer as _LW
from rle_writer import _set_bits_allocated, write_native_slice8
import jls_model as M


def golden_generator():
    """tests/golden/jls/generate.py as a module (under a name of its own: the golden folders each have a generate.py)."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jls", "generate.py")
    spec = importlib.util.spec_from_file_location("jls_golden_generate", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


JPEG_LS_LOSSLESS = "1.2.840.10008.1.2.4.80"
JPEG_LS_NEAR = "1.2.840.10008.1.2.4.81"


class _BitWriter:
    """Bits into bytes, most significant first; after a 0xFF byte the next byte takes 7 bits."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0          # pending bits (a Python int) and their count
        self.n = 0

    def put(self, value, k):
        self.acc = (self.acc << k) | (value & ((1 << k) - 1))
        self.n += k
        self._flush(False)

    def zeros_one(self, z):
        self.put(1, z + 1)

    def _flush(self, final):
        while True:
            width = 7 if (self.out and self.out[-1] == 0xFF) else 8
            if self.n < width:
                if not (final and self.n):
                    return
                self.acc <<= width - self.n            # the last byte: zero padded
                self.n = width
            self.out.append((self.acc >> (self.n - width)) & ((1 << width) - 1))
            self.n -= width
            self.acc &= (1 << self.n) - 1

    def finish(self):
        self._flush(True)
        if self.out and self.out[-1] == 0xFF:          # the scan may not end on 0xFF: a marker follows
            self.out.append(0)
        return bytes(self.out)


def _golomb(w, p, k, glimit, m):
    hi = m >> k
    if hi < glimit - p.qbpp - 1:
        w.zeros_one(hi)
        w.put(m, k)
    else:
        w.zeros_one(glimit - p.qbpp - 1)
        w.put(m - 1, p.qbpp)


def _quantise_error(e, p):
    if p.near == 0:
        return e
    return (p.near + e) // p.step if e > 0 else -((p.near - e) // p.step)


def _mod_range(e, p):
    if e < 0:
        e += p.range
    if e >= (p.range + 1) // 2:
        e -= p.range
    return e


def encode_scan(img, p: M.Params):
    """Samples [rows, cols] -> (scan bytes, reconstructed samples uint16): the source itself when NEAR = 0."""
    img = np.asarray(img).astype(np.int64)
    rows, cols = img.shape
    w = _BitWriter()
    A, B, C, N = [p.a0] * 367, [0] * 367, [0] * 367, [1] * 367
    rec = np.zeros((rows, cols), dtype=np.uint16)
    ri, corner = 0, 0
    prev = [0] * (cols + 1)
    near, reset, maxval, step = p.near, p.reset, p.maxval, p.step
    for r in range(rows):
        src = img[r].tolist()
        cur = [0] * (cols + 1)
        prev[cols] = prev[cols - 1]
        ra, rc, x = prev[0], corner, 0
        corner = prev[0]
        while x < cols:
            rb, rd = prev[x], prev[x + 1]
            d1, d2, d3 = rd - rb, rb - rc, rc - ra
            if abs(d1) <= near and abs(d2) <= near and abs(d3) <= near:
                x0 = x
                while x < cols and abs(src[x] - ra) <= near:
                    x += 1
                run = x - x0
                cur[x0:x] = [ra] * run
                while run >= 1 << M.J[ri]:
                    w.put(1, 1)
                    run -= 1 << M.J[ri]
                    if ri < 31:
                        ri += 1
                if x == cols:
                    if run:
                        w.put(1, 1)
                    break
                w.put(run, M.J[ri] + 1)
                rb = prev[x]
                t = 1 if abs(ra - rb) <= near else 0
                q = 365 + t
                s = 1 if (t or rb >= ra) else -1
                e = _mod_range(_quantise_error((src[x] - (ra if t else rb)) * s, p), p)
                temp = A[q] + ((N[q] >> 1) if t else 0)
                k = M.golomb_k(N[q], temp)
                if k == 0 and e > 0 and 2 * B[q] < N[q]:
                    mp = 1
                elif e < 0 and 2 * B[q] >= N[q]:
                    mp = 1
                elif e < 0 and k != 0:
                    mp = 1
                else:
                    mp = 0
                m = 2 * abs(e) - t - mp
                _golomb(w, p, k, p.limit - M.J[ri] - 1, m)
                if e < 0:
                    B[q] += 1
                A[q] += (m + 1 - t) >> 1
                if N[q] == reset:
                    A[q] >>= 1
                    B[q] >>= 1
                    N[q] >>= 1
                N[q] += 1
                rx = M.fix((ra if t else rb) + e * s * step, p)
                if ri > 0:
                    ri -= 1
            else:
                qs = 81 * M.quantise(d1, p) + 9 * M.quantise(d2, p) + M.quantise(d3, p)
                sign, q = (-1, -qs) if qs < 0 else (1, qs)
                px = min(ra, rb) if rc >= max(ra, rb) else max(ra, rb) if rc <= min(ra, rb) else ra + rb - rc
                px = min(max(px + sign * C[q], 0), maxval)
                e = _quantise_error((src[x] - px) * sign, p)
                rx = M.fix(px + sign * e * step, p)
                e = _mod_range(e, p)
                k = M.golomb_k(N[q], A[q])
                if near == 0 and k == 0 and 2 * B[q] <= -N[q]:
                    m = 2 * e + 1 if e >= 0 else -2 * (e + 1)
                else:
                    m = 2 * e if e >= 0 else -2 * e - 1
                _golomb(w, p, k, p.limit, m)
                B[q] += e * step
                A[q] += abs(e)
                if N[q] == reset:
                    A[q] >>= 1
                    B[q] >>= 1
                    N[q] >>= 1
                N[q] += 1
                if B[q] <= -N[q]:
                    B[q] += N[q]
                    if C[q] > -128:
                        C[q] -= 1
                    if B[q] <= -N[q]:
                        B[q] = -N[q] + 1
                elif B[q] > 0:
                    B[q] -= N[q]
                    if C[q] < 127:
                        C[q] += 1
                    if B[q] > 0:
                        B[q] = 0
            cur[x] = rx
            ra, rc = rx, rb
            x += 1
        rec[r] = cur[:cols]
        prev = cur
    return w.finish(), rec


def markers(rows, cols, bits, near=0, lse=None, *, app8=b"", components=1, ilv=0, pt=0, table=0, comp_id=1):
    """The marker segments in front of the scan.  lse: (MAXVAL, T1, T2, T3, RESET) or None."""
    out = b"\xFF\xD8"
    if app8:
        out += b"\xFF\xE8" + struct.pack(">H", 2 + len(app8)) + app8
    out += b"\xFF\xF7" + struct.pack(">HBHHB", 8 + 3 * components, bits, rows, cols, components)
    out += b"".join(struct.pack("BBB", comp_id + c, 0x11, 0) for c in range(components))
    if lse is not None:
        out += b"\xFF\xF8" + struct.pack(">HB5H", 13, 1, *lse)
    out += b"\xFF\xDA" + struct.pack(">HB", 6 + 2 * components, components)
    out += b"".join(struct.pack("BB", comp_id + c, table) for c in range(components))
    return out + struct.pack("BBB", near, ilv, pt)


def encode(img, bits, near=0, lse=None, **kw):
    """Samples -> a whole JPEG-LS stream (SOI .. EOI)."""
    img = np.asarray(img)
    p = M.Params(lse[0] or (1 << bits) - 1, near, *lse[1:]) if lse else M.Params((1 << bits) - 1, near)
    scan, _ = encode_scan(img, p)
    return markers(img.shape[0], img.shape[1], bits, near, lse, **kw) + scan + b"\xFF\xD9"


def write_slice(path, pixels, stream=None, *, bits_allocated=16, bits_stored=None, near=0, fragments=1, bot=False, **kw):
    """One JPEG-LS file: dicom_writer.write_slice with the JPEG-LS syntax (.80, or .81 where near > 0), its native PixelData
    replaced by the encapsulated `stream` (default: the stored bit patterns of `pixels` encoded at BitsStored precision)."""
    stored = bits_stored if bits_stored is not None else bits_allocated
    if stream is None:
        stream = encode(np.asarray(pixels).astype(np.int64) & ((1 << stored) - 1), stored, near)
    kw.setdefault("transfer_syntax", JPEG_LS_NEAR if near else JPEG_LS_LOSSLESS)
    _LW.write_compressed_slice(path, pixels, stream, fragments=fragments, bot=bot, bits_stored=stored, **kw)
    if bits_allocated != 16:
        with open(path, "rb") as f:
            buf = f.read()
        with open(path, "wb") as f:
            f.write(_set_bits_allocated(buf, bits_allocated))


def write_series(folder, volume_zyx_stored, *, compressed=True, bits_allocated=16, origin=(-100.0, -120.0, 50.0),
                 iop=(1, 0, 0, 0, 1, 0), dz=1.5, name="IM%04d.dcm", **kw):
    """A series of JPEG-LS slices (or, compressed=False, of native slices of the same BitsAllocated)."""
    os.makedirs(folder, exist_ok=True)
    iop_a = np.asarray(iop, dtype=float)
    normal = np.cross(iop_a[:3], iop_a[3:])
    paths = []
    for z in range(len(volume_zyx_stored)):
        p = os.path.join(folder, name % z)
        geo = dict(ipp=np.asarray(origin, dtype=float) + z * dz * normal, iop=iop, instance=z + 1)
        if compressed:
            write_slice(p, volume_zyx_stored[z], bits_allocated=bits_allocated, **geo, **kw)
        else:
            kw2 = {k: v for k, v in kw.items() if k != "near"}
            if bits_allocated == 8:
                write_native_slice8(p, volume_zyx_stored[z], **geo, **kw2)
            else:
                _write_native(p, volume_zyx_stored[z], **geo, **kw2)
        paths.append(p)
    return paths
