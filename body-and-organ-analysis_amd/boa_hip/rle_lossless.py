"""RLE Lossless (DICOM PS3.5 Annex G) for DICOM CT: transfer syntax 1.2.840.10008.1.2.5.  The reference reads these series through
GDCM (BOA/compute/io.py:254-259); here the host reads the 64-byte RLE header of every frame and the PackBits streams of the whole
series are decoded in one batched HIP call (csrc/rle.hip, `boa_rle_decode`).

A frame is a header (a little-endian uint32 segment count and 15 uint32 segment offsets) and one segment per byte plane of the
samples, the most significant plane first; a segment is a PackBits stream over the plane's rows.  Host side (this module, numpy
only, no device): `parse_frame`, `build_batch`.  Device side: `decode_frames`.  The decoding rule (one rule for both kernels and
the tests' model): include/boa_hip.h, `boa_rle_decode`.
"""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

RLE_LOSSLESS = "1.2.840.10008.1.2.5"
SYNTAXES = (RLE_LOSSLESS,)

HEADER_BYTES, FRAME_WORDS = 64, 8                      # include/boa_hip.h: BOA_RLE_FRAME_WORDS
STATUS = {1: "segment truncated"}


def _err(msg: str):
    from .dicom import DicomError
    return DicomError(msg)


def plausible_header(data: bytes) -> bool:
    """The coarse test `dicom.read_file` applies to the PixelData of an RLE-syntax file: at least a header, a segment count in
    1 .. 15, the first segment right behind the header.  Everything finer is `parse_frame`'s."""
    if len(data) < HEADER_BYTES:
        return False
    count, first = struct.unpack_from("<II", data, 0)
    return 1 <= count <= 15 and first == HEADER_BYTES


@dataclass
class Frame:
    """One parsed RLE frame."""
    name: str
    rows: int
    cols: int
    data: np.ndarray               # uint8: the whole frame, header included
    bounds: List[Tuple[int, int]]  # per segment (= byte plane, most significant first): first byte, end byte in `data`


def parse_frame(data: bytes, *, rows: int, cols: int, bits_allocated: int = 16, bits_stored: Optional[int] = None,
                name: str = "") -> Frame:
    """The RLE header of one frame.  Raises NotImplementedError for a segment count other than BitsAllocated / 8 of an 8- or
    16-bit image (named), DicomError for anything else this reader does not accept."""
    buf = bytes(data)
    if len(buf) < HEADER_BYTES:
        raise _err(f"{name}: RLE frame of {len(buf)} bytes is shorter than its {HEADER_BYTES}-byte header")
    count, *offsets = struct.unpack_from("<16I", buf, 0)
    if not 1 <= count <= 15:
        raise _err(f"{name}: RLE header with {count} segments (1..15)")
    if bits_allocated not in (8, 16) or count != bits_allocated // 8:
        raise NotImplementedError(f"{name}: RLE frame of {count} segments with BitsAllocated {bits_allocated}: only one segment per "
                                  "byte of an 8- or 16-bit single-sample image is read")
    if offsets[0] != HEADER_BYTES:
        raise _err(f"{name}: first RLE segment at offset {offsets[0]}, {HEADER_BYTES} expected")
    used = offsets[:count]
    for k in range(1, count):
        if used[k] <= used[k - 1]:
            raise _err(f"{name}: RLE segment offsets are not increasing ({used[k - 1]}, {used[k]})")
    if used[-1] >= len(buf):
        raise _err(f"{name}: RLE segment offset {used[-1]} is outside the {len(buf)}-byte frame")
    ends = used[1:] + [len(buf)]
    return Frame(name, rows, cols, np.frombuffer(buf, dtype=np.uint8), list(zip(used, ends)))


def build_batch(frames: Sequence[Frame]) -> Tuple[np.ndarray, np.ndarray]:
    """Frames -> (data uint8: the frames back to back, frame table int32 [n][FRAME_WORDS]) as `boa_rle_decode` takes them."""
    ftab = np.zeros((len(frames), FRAME_WORDS), dtype=np.int64)
    off = 0
    for f, fr in enumerate(frames):
        ftab[f, :4] = [off & 0xFFFFFFFF, off >> 32, len(fr.data), len(fr.bounds)]
        ftab[f, 4:4 + 2 * len(fr.bounds)] = np.asarray(fr.bounds).ravel()
        off += len(fr.data)
    data = np.concatenate([fr.data for fr in frames])
    return data, ftab.astype(np.uint32).view(np.int32)


def decode_frames(ctx, frames: Sequence[Frame], *, serial: bool = False, chunk_bytes: int = 1024) -> Tuple[np.ndarray, np.ndarray]:
    """Decode a batch of frames of one size on the device in one call -> (uint16 [n][rows][cols] stored bit patterns, int32 status
    per frame: 0 ok, else a key of STATUS; the samples of a failed frame are unspecified).  serial: the one-lane-per-segment
    reference decoder; chunk_bytes: the chunk size of the parallel decoder, a power of two in 256 .. 4096."""
    if not frames:
        raise ValueError("no frames")
    rows, cols = frames[0].rows, frames[0].cols
    if any((f.rows, f.cols) != (rows, cols) for f in frames):
        raise ValueError("the frames of one batch must have one size")
    data, ftab = build_batch(frames)
    return _decode_tables(ctx, data, ftab, rows, cols, serial=serial, chunk_bytes=chunk_bytes)


def _decode_tables(ctx, data: np.ndarray, ftab: np.ndarray, rows: int, cols: int, *, serial: bool = False, chunk_bytes: int = 1024):
    from . import _lib
    n = len(ftab)
    d_data = ctx.from_numpy(data)
    out = ctx.alloc(n * rows * cols * 2)
    status = np.zeros(n, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    ftab = np.ascontiguousarray(ftab)
    try:
        _lib.check(ctx.lib.boa_rle_decode(ctx.h, d_data.vp, data.nbytes, n, ftab.ctypes.data_as(ip), rows, cols, int(chunk_bytes),
                                          out.vp, status.ctypes.data_as(ip), 1 if serial else 0), "boa_rle_decode")
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
        raise _err(f"{f.name}: RLE Lossless decode failed: {STATUS.get(int(status[bad[0]]), 'status %d' % status[bad[0]])}"
                   + (f" ({len(bad)} frames of the series failed)" if len(bad) > 1 else ""))
    return px
