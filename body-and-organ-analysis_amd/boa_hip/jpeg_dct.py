"""Lossy DCT JPEG (ITU T.81 sequential DCT, Huffman) for DICOM CT: transfer syntaxes 1.2.840.10008.1.2.4.50 (baseline, Process 1,
8-bit) and 1.2.840.10008.1.2.4.51 (extended, Process 2 & 4, 8- or 12-bit).  The reference reads these series through GDCM's
bundled libjpeg (BOA/compute/io.py:254-259); here the host parses the encapsulated PixelData and the markers, and the entropy
decode, the dequantisation and the inverse DCT of the whole series run in one batched HIP call (csrc/jpeg_dct.hip,
`boa_jdct_decode`).  The IDCT is not normative in T.81: the pixels are those of libjpeg's default decode (JDCT_ISLOW), bit for bit.

Host side (this module, numpy only, no device): `parse_frame` (the markers of one frame: SOI, APPn / COM, DQT, DHT, SOF0 / SOF1,
DRI, one SOS, EOI; everything else is refused by name), the removal of the byte stuffing and of the RSTn markers and the
expansion of the Huffman tables (both shared with jpeg_lossless).  Device side: `decode_frames`.
"""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .jpeg_lossless import _SOF_NAMES, _err, _segments, expand_table

JPEG_BASELINE = "1.2.840.10008.1.2.4.50"        # Process 1, 8-bit
JPEG_EXTENDED = "1.2.840.10008.1.2.4.51"        # Process 2 & 4, 8- or 12-bit
SYNTAXES = (JPEG_BASELINE, JPEG_EXTENDED)

FRAME_WORDS = 16                                # include/boa_hip.h: BOA_JD_FRAME_WORDS
STATUS = {1: "entropy-coded data truncated", 2: "invalid Huffman code", 3: "zero run past the end of a block",
          4: "SSSS beyond the sample precision", 5: "trailing data after the last block"}

# natural (row-major) index of the coefficient at zig-zag position k (T.81 figure A.6)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])


def plausible_stream(frame: bytes) -> bool:
    """SOI, then SOF0 or SOF1 ahead of any other frame header: what `dicom.read_file` asks of a file under these syntaxes
    before it calls its PixelData a DCT JPEG stream (the markers themselves are `parse_frame`'s)."""
    b = bytes(frame)
    if b[:2] != b"\xFF\xD8":
        return False
    pos = 2
    while pos + 4 <= len(b) and b[pos] == 0xFF:
        m = b[pos + 1]
        if m == 0xFF:                                # fill byte
            pos += 1
            continue
        if m in (0xC0, 0xC1):
            return True
        if m in _SOF_NAMES or m == 0xC3 or m in (0xDA, 0xD9):
            return False
        pos += 2 + struct.unpack_from(">H", b, pos + 2)[0]
    return False


@dataclass
class Frame:
    """One parsed sequential DCT frame."""
    name: str
    rows: int
    cols: int
    precision: int                 # P: 8 or 12
    restart: int                   # restart interval in blocks, 0 = none
    qtable: bytes                  # the component's quantisation table: 64 little-endian uint16 in natural order
    dc: Tuple[bytes, bytes]        # the scan's DC table: (16 code counts, SSSS values)
    ac: Tuple[bytes, bytes]        # the scan's AC table: (16 code counts, RRRRSSSS values)
    data: np.ndarray               # uint8: entropy-coded data with the stuffing and the RSTn markers removed
    seg_bounds: np.ndarray         # int64 [n_seg + 1]: byte offsets in `data` where each restart interval starts, then the end

    @property
    def n_blocks(self) -> int:
        return -(-self.rows // 8) * -(-self.cols // 8)


def _check_table(tc: int, counts: bytes, values: bytes, name: str) -> None:
    code = 0
    for length in range(1, 17):
        code += counts[length - 1]
        if code > (1 << length):
            raise _err(f"{name}: Huffman table code counts exceed {length}-bit codes")
        code <<= 1
    if len(set(values)) != len(values):
        raise _err(f"{name}: Huffman table lists a value twice")
    if tc == 0 and any(v > 15 for v in values):
        raise _err(f"{name}: DC Huffman table holds SSSS values above 15")
    if tc == 1 and any((v & 15) == 0 and (v >> 4) not in (0, 15) for v in values):
        raise _err(f"{name}: AC Huffman table holds EOBn run codes (progressive JPEG's)")


def parse_frame(data: bytes, *, rows: int, cols: int, bits_allocated: int = 16, bits_stored: Optional[int] = None,
                name: str = "") -> Frame:
    """The markers of one sequential DCT frame.  Raises NotImplementedError for the other coding processes, several components
    and several scans (named), DicomError for anything else this reader does not accept."""
    buf = bytes(data)
    bits_stored = bits_allocated if bits_stored is None else bits_stored
    if buf[:2] != b"\xFF\xD8":
        raise _err(f"{name}: compressed frame does not start with SOI")
    pos = 2
    huff: Dict[Tuple[int, int], Tuple[bytes, bytes]] = {}
    quant: Dict[int, bytes] = {}
    sof = None
    restart = 0

    def segment():
        if pos + 2 > len(buf):
            raise _err(f"{name}: marker segment overruns the frame")
        ln = struct.unpack_from(">H", buf, pos)[0]
        if ln < 2 or pos + ln > len(buf):
            raise _err(f"{name}: marker segment of length {ln} overruns the frame")
        return buf[pos + 2:pos + ln], pos + ln

    while True:
        if pos >= len(buf) or buf[pos] != 0xFF:
            raise _err(f"{name}: expected a marker at byte {pos}")
        while pos < len(buf) and buf[pos] == 0xFF:
            pos += 1                               # (fill bytes)
        if pos >= len(buf):
            raise _err(f"{name}: frame ends inside a marker")
        m = buf[pos]
        pos += 1
        if m == 0xD9:
            raise _err(f"{name}: EOI before any scan")
        if 0xE0 <= m <= 0xEF or m == 0xFE:         # APPn, COM
            _, pos = segment()
        elif m == 0xDB:                            # DQT: possibly several tables
            body, pos = segment()
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                if pq > 1 or tq > 3:
                    raise _err(f"{name}: DQT precision {pq} / id {tq}")
                n = 64 * (1 + pq)
                if k + 1 + n > len(body):
                    raise _err(f"{name}: DQT segment truncated")
                q = np.frombuffer(body, dtype=">u2" if pq else np.uint8, count=64, offset=k + 1)
                if (q == 0).any():
                    raise _err(f"{name}: DQT table {tq} holds a zero")
                nat = np.zeros(64, dtype="<u2")
                nat[ZIGZAG] = q
                quant[tq] = nat.tobytes()
                k += 1 + n
        elif m == 0xC4:                            # DHT: possibly several tables
            body, pos = segment()
            k = 0
            while k < len(body):
                if k + 17 > len(body):
                    raise _err(f"{name}: DHT segment truncated")
                tc, th = body[k] >> 4, body[k] & 15
                counts = body[k + 1:k + 17]
                n = sum(counts)
                if k + 17 + n > len(body):
                    raise _err(f"{name}: DHT segment truncated")
                if tc > 1 or th > 3 or n > 256:
                    raise _err(f"{name}: DHT class {tc} / id {th} with {n} codes")
                huff[(tc, th)] = (bytes(counts), bytes(body[k + 17:k + 17 + n]))
                k += 17 + n
        elif m in (0xC0, 0xC1):                    # SOF0, SOF1
            body, pos = segment()
            if sof is not None:
                raise _err(f"{name}: more than one frame header")
            if len(body) < 6:
                raise _err(f"{name}: SOF{m - 0xC0} segment truncated")
            p, y, x, nf = body[0], struct.unpack_from(">H", body, 1)[0], struct.unpack_from(">H", body, 3)[0], body[5]
            if len(body) != 6 + 3 * nf or nf == 0:
                raise _err(f"{name}: SOF{m - 0xC0} segment of {len(body)} bytes for {nf} components")
            if nf != 1:
                raise NotImplementedError(f"{name}: JPEG frame with {nf} components: only single-component (MONOCHROME2) "
                                          "frames are read")
            if p not in ((8,) if m == 0xC0 else (8, 12)):
                raise _err(f"{name}: SOF{m - 0xC0} precision {p} ({'8' if m == 0xC0 else '8 or 12'})")
            if y == 0:
                raise _err(f"{name}: SOF{m - 0xC0} with 0 lines (number of lines defined by DNL is not read)")
            if (y, x) != (rows, cols):
                raise _err(f"{name}: SOF{m - 0xC0} size {y} x {x} differs from Rows x Columns {rows} x {cols}")
            if p > bits_allocated or p < bits_stored:
                raise _err(f"{name}: SOF{m - 0xC0} precision {p} outside BitsStored {bits_stored} .. BitsAllocated {bits_allocated}")
            if body[7] != 0x11:
                raise _err(f"{name}: sampling factors {body[7] >> 4} x {body[7] & 15} of a single component (1 x 1)")
            sof = (p, body[6], body[8], m - 0xC0)
        elif m in _SOF_NAMES or m == 0xC3:
            what = _SOF_NAMES.get(m, "lossless (Huffman)")
            raise NotImplementedError(f"{name}: JPEG {what} (SOF marker {m:02X}): only sequential DCT with Huffman coding "
                                      "(SOF0, SOF1) is read under this transfer syntax")
        elif m == 0xDD:                            # DRI
            body, pos = segment()
            if len(body) != 2:
                raise _err(f"{name}: DRI segment of {len(body)} bytes")
            restart = struct.unpack(">H", body)[0]
        elif m == 0xDC:
            raise _err(f"{name}: DNL marker (number of lines defined after the scan) is not read")
        elif m == 0xDA:                            # SOS
            body, pos = segment()
            break
        else:
            raise _err(f"{name}: unexpected marker FF{m:02X} ahead of the scan")
    if sof is None:
        raise _err(f"{name}: scan before the frame header (no SOF0 / SOF1)")
    if len(body) < 1 or body[0] != 1 or len(body) != 6:
        raise _err(f"{name}: scan with {body[0] if body else 0} components (one is read)")
    cs, td, ta, ss, se, ahal = body[1], body[2] >> 4, body[2] & 15, body[3], body[4], body[5]
    if cs != sof[1]:
        raise _err(f"{name}: scan component {cs} is not the frame's component {sof[1]}")
    if (ss, se, ahal) != (0, 63, 0):
        raise _err(f"{name}: scan parameters Ss {ss}, Se {se}, Ah {ahal >> 4}, Al {ahal & 15} (sequential: 0, 63, 0, 0)")
    if sof[3] == 0 and (td > 1 or ta > 1):
        raise _err(f"{name}: baseline scan uses Huffman tables {td} / {ta} (0 or 1)")
    if (0, td) not in huff or (1, ta) not in huff:
        raise _err(f"{name}: the scan uses Huffman tables DC {td} / AC {ta}, which no DHT defined")
    if sof[2] not in quant:
        raise _err(f"{name}: the component uses quantisation table {sof[2]}, which no DQT defined")
    _check_table(0, *huff[(0, td)], name)
    _check_table(1, *huff[(1, ta)], name)
    ecs = np.frombuffer(buf, dtype=np.uint8, offset=pos)
    unstuffed, bounds, term = _segments(ecs, name)
    marker = int(ecs[term + 1])
    if marker == 0xDA or marker in (0xC4, 0xDB, 0xDD):
        raise NotImplementedError(f"{name}: more than one scan (only single-scan frames are read)")
    if marker == 0xDC:
        raise _err(f"{name}: DNL marker (number of lines defined after the scan) is not read")
    if marker != 0xD9:
        raise _err(f"{name}: marker FF{marker:02X} after the scan (EOI expected)")
    n_blocks = -(-rows // 8) * -(-cols // 8)
    n_seg = -(-n_blocks // restart) if restart else 1
    if len(bounds) - 1 != n_seg:
        raise _err(f"{name}: {len(bounds) - 1} restart intervals, {n_seg} expected for {n_blocks} blocks")
    return Frame(name, rows, cols, sof[0], restart if restart < n_blocks else 0, quant[sof[2]], huff[(0, td)], huff[(1, ta)],
                 unstuffed, bounds)


def build_batch(frames: Sequence[Frame], subseq_bytes: int = 128):
    """Frames -> (data uint8, frame table, segment table, subsequence table, expanded Huffman tables, quantisation tables) as
    `boa_jdct_decode` takes them."""
    if subseq_bytes < 4:
        raise ValueError(f"subseq_bytes {subseq_bytes} < 4")
    hkeys: Dict[Tuple[bytes, bytes], int] = {}
    qkeys: Dict[bytes, int] = {}
    tabs: List[np.ndarray] = []
    parts, ftab, segs, subs = [], np.zeros((len(frames), FRAME_WORDS), dtype=np.int64), [], []
    off = n_seg = n_sub = 0
    for f, fr in enumerate(frames):
        for key in (fr.dc, fr.ac):
            if key not in hkeys:
                hkeys[key] = len(tabs)
                tabs.append(expand_table(*key))
        q = qkeys.setdefault(fr.qtable, len(qkeys))
        b = fr.seg_bounds
        lo, hi = b[:-1], b[1:]
        nsub = np.maximum(1, -(-(hi - lo) // subseq_bytes))
        first = n_sub + np.concatenate([[0], np.cumsum(nsub)[:-1]])
        k = np.arange(int(nsub.sum())) - np.repeat(first - n_sub, nsub)
        seg_idx = np.repeat(np.arange(len(lo)) + n_seg, nsub)
        subs.append(np.stack([np.repeat(lo, nsub) + k * subseq_bytes, seg_idx], axis=1))
        R = fr.restart or fr.n_blocks
        segs.append(np.stack([lo, hi, np.arange(len(lo)) * R, first], axis=1))
        ftab[f, :12] = [off & 0xFFFFFFFF, off >> 32, len(fr.data), fr.precision, fr.restart, hkeys[fr.dc], hkeys[fr.ac], q, n_seg,
                        len(lo), n_sub, int(nsub.sum())]
        padded = (len(fr.data) + 3) & ~3
        parts.append(fr.data)
        if padded > len(fr.data):
            parts.append(np.zeros(padded - len(fr.data), dtype=np.uint8))
        off += padded
        n_seg += len(lo)
        n_sub += int(nsub.sum())
    data = np.concatenate(parts + [np.zeros(8, dtype=np.uint8)])
    qt = np.stack([np.frombuffer(k, dtype="<u2") for k in qkeys]).astype(np.uint16)
    return (data, ftab.astype(np.uint32).view(np.int32), np.concatenate(segs).astype(np.int32),
            np.concatenate(subs).astype(np.int32), np.stack(tabs), qt)


def decode_frames(ctx, frames: Sequence[Frame], *, serial: bool = False, subseq_bytes: int = 128) -> Tuple[np.ndarray, np.ndarray]:
    """Decode a batch of frames of one size on the device in one call -> (uint16 [n][rows][cols] samples, int32 status per
    frame: 0 ok, else a key of STATUS).  serial: the one-lane-per-frame reference entropy decoder; subseq_bytes: the size of the
    subsequences of the parallel decoder (small values force many resynchronisations)."""
    from . import _lib
    if not frames:
        raise ValueError("no frames")
    rows, cols = frames[0].rows, frames[0].cols
    if any((f.rows, f.cols) != (rows, cols) for f in frames):
        raise ValueError("the frames of one batch must have one size")
    data, ftab, segs, subs, tabs, qt = build_batch(frames, subseq_bytes)
    d_data = ctx.from_numpy(data)
    out = ctx.alloc(len(frames) * rows * cols * 2)
    status = np.zeros(len(frames), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    tabs, qt = np.ascontiguousarray(tabs), np.ascontiguousarray(qt)
    try:
        _lib.check(ctx.lib.boa_jdct_decode(
            ctx.h, d_data.vp, data.nbytes, len(frames), ftab.ctypes.data_as(ip), rows, cols, len(segs), segs.ctypes.data_as(ip),
            len(subs), subs.ctypes.data_as(ip), len(tabs), tabs.ctypes.data_as(C.POINTER(C.c_uint32)), len(qt),
            qt.ctypes.data_as(C.POINTER(C.c_uint16)), out.vp, status.ctypes.data_as(ip), 1 if serial else 0), "boa_jdct_decode")
        px = out.download((len(frames), rows, cols), np.uint16)
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
        raise _err(f"{f.name}: JPEG decode failed: {STATUS.get(int(status[bad[0]]), 'status %d' % status[bad[0]])}"
                   + (f" ({len(bad)} frames of the series failed)" if len(bad) > 1 else ""))
    return px
