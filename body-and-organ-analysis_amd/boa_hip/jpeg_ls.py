"""JPEG-LS (ITU-T T.87) for DICOM CT: transfer syntaxes 1.2.840.10008.1.2.4.80 (lossless) and 1.2.840.10008.1.2.4.81
(near-lossless).  The reference reads these series through GDCM (BOA/compute/io.py:254-259), whose JPEG-LS codec is CharLS; here
the host reads the markers of every frame and the scans of the whole series are decoded in one batched HIP call
(csrc/jls.hip, `boa_jls_decode`).

A frame is SOI, any APPn (CharLS writes a SPIFF header in APP8) and COM, SOF55, an optional LSE of id 1 (MAXVAL, T1, T2, T3,
RESET), one SOS, the scan and EOI.  One component, no interleaving, no point transform, no mapping table and no restart interval
are read; everything else is refused by name.  Host side (this module, numpy only, no device): `parse_frame`, `build_batch`.
Device side: `decode_frames`; the device reads the stuffed bit stream itself.  The decoding rule (one rule for both kernels and the
tests' model): include/boa_hip.h, `boa_jls_decode`.
"""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

JPEG_LS_LOSSLESS = "1.2.840.10008.1.2.4.80"
JPEG_LS_NEAR = "1.2.840.10008.1.2.4.81"
SYNTAXES = (JPEG_LS_LOSSLESS, JPEG_LS_NEAR)

FRAME_WORDS = 16                                       # include/boa_hip.h: BOA_JLS_FRAME_WORDS
STATUS = {1: "scan truncated", 2: "invalid code in the scan"}
_LSE_NAMES = {2: "mapping table specification", 3: "mapping table continuation", 4: "oversize image dimensions"}


def _err(msg: str):
    from .dicom import DicomError
    return DicomError(msg)


def plausible_stream(data: bytes) -> bool:
    """The coarse test `dicom.read_file` applies to the PixelData of a JPEG-LS-syntax file: SOI, then SOF55 before any other
    SOF marker.  Everything finer is `parse_frame`'s."""
    buf = bytes(data[:65536])
    if buf[:2] != b"\xFF\xD8":
        return False
    pos = 2
    while pos + 4 <= len(buf) and buf[pos] == 0xFF:
        m = buf[pos + 1]
        if m == 0xF7:
            return True
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC) or m in (0xDA, 0xD9) or m < 0xC0:
            return False
        pos += 2 + struct.unpack_from(">H", buf, pos + 2)[0]
    return False


def _clamp_t(i: int, j: int, maxval: int) -> int:
    return j if (i > maxval or i < j) else i


def default_thresholds(maxval: int, near: int) -> Tuple[int, int, int]:
    """T.87 C.2.4.1.1.1 (csrc/jls_codes.h: jls_default_thresholds)."""
    if maxval >= 128:
        f = (min(maxval, 4095) + 128) // 256
        t1 = _clamp_t(f + 2 + 3 * near, near + 1, maxval)
        t2 = _clamp_t(f * 4 + 3 + 5 * near, t1, maxval)
        t3 = _clamp_t(f * 17 + 4 + 7 * near, t2, maxval)
    else:
        f = 256 // (maxval + 1)
        t1 = _clamp_t(max(2, 3 // f + 3 * near), near + 1, maxval)
        t2 = _clamp_t(max(3, 7 // f + 5 * near), t1, maxval)
        t3 = _clamp_t(max(4, 21 // f + 7 * near), t2, maxval)
    return t1, t2, t3


@dataclass
class Frame:
    """One parsed JPEG-LS frame."""
    name: str
    rows: int
    cols: int
    precision: int                 # P
    maxval: int                    # the coding parameters, defaults resolved
    near: int
    t1: int
    t2: int
    t3: int
    reset: int
    data: np.ndarray               # uint8: the scan's bytes, stuffing included, up to the marker that ends it


def parse_frame(data: bytes, *, rows: int, cols: int, bits_allocated: int = 16, bits_stored: Optional[int] = None,
                name: str = "") -> Frame:
    """The markers of one JPEG-LS frame.  Raises NotImplementedError for several components or an interleaved scan, LSE ids
    2 - 4, a mapping table, a restart interval and a point transform (each named), DicomError for anything else this reader does
    not accept."""
    buf = bytes(data)
    bits_stored = bits_allocated if bits_stored is None else bits_stored
    if buf[:2] != b"\xFF\xD8":
        raise _err(f"{name}: JPEG-LS frame does not start with SOI")
    pos = 2
    sof = None
    lse = (0, 0, 0, 0, 0)

    def segment():
        if pos + 2 > len(buf):
            raise _err(f"{name}: marker segment overruns the frame")
        ln = struct.unpack_from(">H", buf, pos)[0]
        if ln < 2 or pos + ln > len(buf):
            raise _err(f"{name}: marker segment of length {ln} overruns the frame")
        return buf[pos + 2:pos + ln], pos + ln

    while True:
        if pos >= len(buf) or buf[pos] != 0xFF:
            raise _err(f"{name}: expected a marker at byte {pos} (no SOS)" if sof else f"{name}: expected a marker at byte {pos} (no SOF55)")
        while pos < len(buf) and buf[pos] == 0xFF:
            pos += 1                               # (fill bytes)
        if pos >= len(buf):
            raise _err(f"{name}: frame ends inside a marker")
        m = buf[pos]
        pos += 1
        if m == 0xD9:
            raise _err(f"{name}: EOI before any scan (no SOS)")
        if 0xE0 <= m <= 0xEF or m == 0xFE:         # APPn (SPIFF: APP8), COM
            _, pos = segment()
        elif m == 0xF7:                            # SOF55
            body, pos = segment()
            if sof is not None:
                raise _err(f"{name}: more than one frame header")
            if len(body) < 6:
                raise _err(f"{name}: SOF55 segment truncated")
            p, y, x, nf = body[0], struct.unpack_from(">H", body, 1)[0], struct.unpack_from(">H", body, 3)[0], body[5]
            if len(body) != 6 + 3 * nf:
                raise _err(f"{name}: SOF55 segment of {len(body)} bytes for {nf} components")
            if nf != 1:
                raise NotImplementedError(f"{name}: JPEG-LS frame of {nf} components: only single-component frames are read")
            if not 2 <= p <= 16:
                raise _err(f"{name}: SOF55 precision {p} (2..16)")
            if y == 0 or x == 0:
                raise NotImplementedError(f"{name}: SOF55 with a zero dimension (oversize image dimensions, LSE id 4, or DNL) "
                                          "is not read")
            if (y, x) != (rows, cols):
                raise _err(f"{name}: SOF55 size {y} x {x} differs from Rows x Columns {rows} x {cols}")
            if p > bits_allocated or p < bits_stored:
                raise _err(f"{name}: SOF55 precision {p} outside BitsStored {bits_stored} .. BitsAllocated {bits_allocated}")
            sof = (p, body[6])
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise _err(f"{name}: SOF marker {m:02X} in a JPEG-LS frame (SOF55 expected)")
        elif m == 0xF8:                            # LSE
            body, pos = segment()
            if len(body) < 1:
                raise _err(f"{name}: LSE segment truncated")
            if body[0] in _LSE_NAMES:
                raise NotImplementedError(f"{name}: JPEG-LS LSE id {body[0]} ({_LSE_NAMES[body[0]]}) is not read")
            if body[0] != 1 or len(body) != 11:
                raise _err(f"{name}: LSE segment id {body[0]} of {len(body)} bytes")
            lse = struct.unpack_from(">5H", body, 1)
        elif m == 0xDD:                            # DRI
            body, pos = segment()
            if len(body) not in (2, 3, 4):
                raise _err(f"{name}: DRI segment of {len(body)} bytes")
            if int.from_bytes(body, "big"):
                raise NotImplementedError(f"{name}: JPEG-LS restart interval of {int.from_bytes(body, 'big')} lines (DRI) is not read")
        elif m == 0xDC:
            raise _err(f"{name}: DNL marker (number of lines defined after the scan) is not read")
        elif m == 0xDA:                            # SOS
            body, pos = segment()
            break
        else:
            raise _err(f"{name}: unexpected marker FF{m:02X} ahead of the scan")
    if sof is None:
        raise _err(f"{name}: scan before the frame header (no SOF55)")
    if len(body) < 1 or len(body) != 4 + 2 * body[0]:
        raise _err(f"{name}: SOS segment of {len(body)} bytes")
    near, ilv, pt = body[-3], body[-2], body[-1]
    if body[0] != 1 or ilv != 0:
        raise NotImplementedError(f"{name}: JPEG-LS scan of {body[0]} components, interleave mode {ilv}: only single-component, "
                                  "non-interleaved scans are read")
    if body[1] != sof[1]:
        raise _err(f"{name}: scan component {body[1]} is not the frame's component {sof[1]}")
    if body[2] != 0:
        raise NotImplementedError(f"{name}: JPEG-LS mapping table {body[2]} selected in SOS: mapping tables are not read")
    if pt != 0:
        raise NotImplementedError(f"{name}: JPEG-LS point transform {pt} is not read")
    # the coding parameters (T.87 C.2.4.1.1): a zero field of LSE stands for the default
    p = sof[0]
    maxval = lse[0] or (1 << p) - 1
    if maxval > (1 << p) - 1:
        raise _err(f"{name}: LSE MAXVAL {maxval} above the {p}-bit precision")
    if near > min(255, maxval // 2):
        raise _err(f"{name}: NEAR {near} above min(255, MAXVAL / 2) = {min(255, maxval // 2)}")
    d = default_thresholds(maxval, near)
    t1, t2, t3, reset = lse[1] or d[0], lse[2] or d[1], lse[3] or d[2], lse[4] or 64
    if not (near + 1 <= t1 <= maxval and t1 <= t2 <= maxval and t2 <= t3 <= maxval):
        raise _err(f"{name}: LSE thresholds T1 {t1}, T2 {t2}, T3 {t3} out of order or range (NEAR {near}, MAXVAL {maxval})")
    if not 3 <= reset <= max(255, maxval):
        raise _err(f"{name}: LSE RESET {reset} outside 3 .. {max(255, maxval)}")
    # the scan: up to the first marker, which must be EOI
    ecs = np.frombuffer(buf, dtype=np.uint8, offset=pos)
    term = np.flatnonzero((ecs[:-1] == 0xFF) & (ecs[1:] >= 0x80)) if len(ecs) >= 2 else ()
    if len(term) == 0:
        raise _err(f"{name}: JPEG-LS scan not terminated by a marker (EOI missing)")
    end = int(term[0])
    marker = int(ecs[end + 1])
    if marker == 0xDA:
        raise _err(f"{name}: more than one scan (only single-scan frames are read)")
    if marker == 0xDC:
        raise _err(f"{name}: DNL marker (number of lines defined after the scan) is not read")
    if marker != 0xD9:
        raise _err(f"{name}: marker FF{marker:02X} after the scan (EOI expected)")
    return Frame(name, rows, cols, p, maxval, near, t1, t2, t3, reset, ecs[:end])


def build_batch(frames: Sequence[Frame]) -> Tuple[np.ndarray, np.ndarray]:
    """Frames -> (data uint8: the scans, each starting on a 4-byte boundary and zero padded to one, frame table int32
    [n][FRAME_WORDS]) as `boa_jls_decode` takes them."""
    ftab = np.zeros((len(frames), FRAME_WORDS), dtype=np.int64)
    sizes = np.array([len(fr.data) for fr in frames], dtype=np.int64)
    padded = (sizes + 3) & ~3
    offs = np.concatenate([[0], np.cumsum(padded)])
    data = np.zeros(int(offs[-1]) + 8, dtype=np.uint8)
    for f, fr in enumerate(frames):
        off = int(offs[f])
        data[off:off + len(fr.data)] = fr.data
        ftab[f, :9] = [off & 0xFFFFFFFF, off >> 32, len(fr.data), fr.maxval, fr.near, fr.t1, fr.t2, fr.t3, fr.reset]
    return data, ftab.astype(np.uint32).view(np.int32)


def decode_frames(ctx, frames: Sequence[Frame], *, serial: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """Decode a batch of frames of one size on the device in one call -> (uint16 [n][rows][cols] samples, int32 status per frame:
    0 ok, else a key of STATUS; the samples of a failed frame are unspecified).  serial: the one-lane-per-frame reference
    decoder instead of the one-wave-per-frame one."""
    if not frames:
        raise ValueError("no frames")
    rows, cols = frames[0].rows, frames[0].cols
    if any((f.rows, f.cols) != (rows, cols) for f in frames):
        raise ValueError("the frames of one batch must have one size")
    data, ftab = build_batch(frames)
    return _decode_tables(ctx, data, ftab, rows, cols, serial=serial)


def _decode_tables(ctx, data: np.ndarray, ftab: np.ndarray, rows: int, cols: int, *, serial: bool = False):
    from . import _lib
    n = len(ftab)
    d_data = ctx.from_numpy(data)
    out = ctx.alloc(n * rows * cols * 2)
    status = np.zeros(n, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    ftab = np.ascontiguousarray(ftab)
    try:
        _lib.check(ctx.lib.boa_jls_decode(ctx.h, d_data.vp, data.nbytes, n, ftab.ctypes.data_as(ip), rows, cols, out.vp,
                                          status.ctypes.data_as(ip), 1 if serial else 0), "boa_jls_decode")
        px = out.download((n, rows, cols), np.uint16)
    finally:
        d_data.free()
        out.free()
    return px, status


def decode(ctx, frames: Sequence[Frame], **kw) -> np.ndarray:
    """`decode_frames`, raising DicomError naming the first file whose frame did not decode."""
    px, status = decode_frames(ctx, frames, **kw)
    bad = np.flatnonzero(status)
    if len(bad):
        f = frames[int(bad[0])]
        raise _err(f"{f.name}: JPEG-LS decode failed: {STATUS.get(int(status[bad[0]]), 'status %d' % status[bad[0]])}"
                   + (f" ({len(bad)} frames of the series failed)" if len(bad) > 1 else ""))
    return px
