"""JPEG Lossless, Process 14 (ITU T.81 Annex H) for DICOM CT: transfer syntaxes 1.2.840.10008.1.2.4.57 (any predictor) and
1.2.840.10008.1.2.4.70 (first-order prediction, selection value 1).  The reference reads these series through GDCM
(BOA/compute/io.py:254-259); here the host parses the encapsulated PixelData and the markers, and the entropy decode and the
reconstruction of the whole series run in one batched HIP call (csrc/jpeg_ll.hip, `boa_ljpeg_decode`).

Host side (this module, numpy only, no device): `read_encapsulated` (PS3.5 A.4 fragments of one frame), `parse_frame` (the
markers of one frame: SOI, APPn / COM, DHT, SOF3, DRI, one SOS, EOI; everything else is refused by name), the removal of the
byte stuffing and of the RSTn markers, and the expansion of the Huffman tables into lookup form.  Device side: `decode_frames`.
"""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

JPEG_LOSSLESS = "1.2.840.10008.1.2.4.57"        # Process 14, any predictor
JPEG_LOSSLESS_SV1 = "1.2.840.10008.1.2.4.70"    # Process 14, selection value 1
SYNTAXES = (JPEG_LOSSLESS, JPEG_LOSSLESS_SV1)

FRAME_WORDS, TABLE_WORDS, LOOKUP_BITS = 16, 384, 9     # include/boa_hip.h: BOA_LJ_FRAME_WORDS, BOA_LJ_TABLE_WORDS, jpeg_ll.hip LB
STATUS = {1: "entropy-coded data truncated", 2: "invalid Huffman code", 3: "trailing garbage after the last sample"}

# SOFn markers of the other coding processes (T.81 table B.1) and JPEG-LS (T.87): refused by name
_SOF_NAMES = {0xC0: "baseline sequential DCT", 0xC1: "extended sequential DCT (Huffman)", 0xC2: "progressive DCT (Huffman)",
              0xC5: "differential sequential DCT (Huffman)", 0xC6: "differential progressive DCT (Huffman)",
              0xC7: "differential lossless (Huffman)", 0xC9: "extended sequential DCT (arithmetic)",
              0xCA: "progressive DCT (arithmetic)", 0xCB: "lossless (arithmetic)", 0xCD: "differential sequential DCT (arithmetic)",
              0xCE: "differential progressive DCT (arithmetic)", 0xCF: "differential lossless (arithmetic)", 0xF7: "JPEG-LS"}


def _err(msg: str):
    from .dicom import DicomError
    return DicomError(msg)


class CompressedFrame(bytes):
    """The bytes of one compressed frame (the concatenated fragments of an encapsulated PixelData), tagged with the file's
    transfer syntax, which names the codec: what `dicom.read_file` returns as PixelData for a JPEG Lossless, JPEG-LS,
    JPEG 2000, RLE Lossless or DCT JPEG file."""
    transfer_syntax: str = ""


def read_encapsulated(buf: bytes, pos: int, name: str = "") -> Tuple[bytes, int]:
    """PS3.5 A.4: the value of an undefined-length PixelData starting at `pos` (after its header) -> (frame bytes, position after
    the sequence delimiter).  Item 1 is the Basic Offset Table (possibly empty); the fragments up to (FFFE,E0DD) are one frame."""
    items: List[bytes] = []
    while True:
        if pos + 8 > len(buf):
            raise _err(f"{name}: encapsulated PixelData ends without a sequence delimiter")
        g, e, length = struct.unpack_from("<HHI", buf, pos)
        pos += 8
        if (g, e) == (0xFFFE, 0xE0DD):
            break
        if (g, e) != (0xFFFE, 0xE000):
            raise _err(f"{name}: unexpected tag ({g:04X},{e:04X}) in encapsulated PixelData")
        if length == 0xFFFFFFFF or pos + length > len(buf):
            raise _err(f"{name}: encapsulated PixelData item of length {length:#x} overruns the file")
        items.append(buf[pos:pos + length])
        pos += length
    if not items:
        raise _err(f"{name}: encapsulated PixelData without a Basic Offset Table item")
    bot, frags = items[0], items[1:]
    if len(bot) > 4:
        raise NotImplementedError(f"{name}: a Basic Offset Table of {len(bot) // 4} frames: multi-frame objects are not read")
    if not frags:
        raise _err(f"{name}: encapsulated PixelData holds no fragment")
    return b"".join(frags), pos


@dataclass
class Frame:
    """One parsed Process-14 frame."""
    name: str
    rows: int
    cols: int
    precision: int                 # P
    pt: int                        # point transform (Al)
    predictor: int                 # selection value Ss, 1..7
    restart_rows: int              # 0 = no restart interval
    counts: bytes                  # the scan's DHT table: 16 code counts
    values: bytes                  # and its SSSS values
    data: np.ndarray               # uint8: entropy-coded data with the stuffing and the RSTn markers removed
    seg_bounds: np.ndarray         # int64 [n_seg + 1]: byte offsets in `data` where each restart interval starts, then the end


def _segments(ecs: np.ndarray, name: str) -> Tuple[np.ndarray, np.ndarray, int]:
    """Entropy-coded data starting at ecs[0] -> (un-stuffed bytes, interval bounds, index of the terminating marker's FF)."""
    if len(ecs) < 2:
        raise _err(f"{name}: entropy-coded segment not terminated by a marker")
    ff = np.flatnonzero(ecs[:-1] == 0xFF)
    nxt = ecs[ff + 1]
    rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    term = np.flatnonzero((nxt != 0x00) & (nxt != 0xFF) & ~rst)
    if len(term) == 0:
        raise _err(f"{name}: entropy-coded segment not terminated by a marker (EOI missing)")
    end = int(ff[term[0]])
    inside = ff < end
    ff, nxt, rst = ff[inside], nxt[inside], rst[inside]
    keep = np.ones(end, dtype=bool)
    keep[ff[nxt == 0x00] + 1] = False              # FF 00 -> FF
    keep[ff[nxt == 0xFF]] = False                  # fill bytes ahead of a marker
    rpos = ff[rst]
    keep[rpos] = False
    keep[rpos + 1] = False
    seq = nxt[rst].astype(np.int64) - 0xD0
    if (seq != np.arange(len(seq)) % 8).any():
        raise _err(f"{name}: restart markers out of sequence")
    before = np.concatenate([[0], np.cumsum(keep)])    # kept bytes ahead of each position
    bounds = np.concatenate([[0], before[rpos], [before[-1]]]).astype(np.int64)
    return ecs[:end][keep], bounds, end


def parse_frame(data: bytes, *, rows: int, cols: int, bits_allocated: int = 16, bits_stored: Optional[int] = None,
                name: str = "") -> Frame:
    """The markers of one JPEG Lossless frame.  Raises NotImplementedError for the other coding processes (named) and a
    restart interval that is not a whole number of rows, DicomError for anything else this reader does not accept."""
    buf = bytes(data)
    bits_stored = bits_allocated if bits_stored is None else bits_stored
    if buf[:2] != b"\xFF\xD8":
        raise _err(f"{name}: compressed frame does not start with SOI")
    pos = 2
    tables: Dict[int, Tuple[bytes, bytes]] = {}
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
                if tc != 0 or th > 3:
                    raise _err(f"{name}: DHT class {tc} / id {th} (lossless scans use DC-class tables 0-3)")
                tables[th] = (bytes(counts), bytes(body[k + 17:k + 17 + n]))
                k += 17 + n
        elif m == 0xC3:                            # SOF3
            body, pos = segment()
            if sof is not None:
                raise _err(f"{name}: more than one frame header")
            if len(body) < 6:
                raise _err(f"{name}: SOF3 segment truncated")
            p, y, x, nf = body[0], struct.unpack_from(">H", body, 1)[0], struct.unpack_from(">H", body, 3)[0], body[5]
            if nf != 1 or len(body) != 6 + 3 * nf:
                raise _err(f"{name}: SOF3 with {nf} components (one is read)")
            if not 2 <= p <= 16:
                raise _err(f"{name}: SOF3 precision {p} (2..16)")
            if y == 0:
                raise _err(f"{name}: SOF3 with 0 lines (number of lines defined by DNL is not read)")
            if (y, x) != (rows, cols):
                raise _err(f"{name}: SOF3 size {y} x {x} differs from Rows x Columns {rows} x {cols}")
            if p > bits_allocated or p < bits_stored:
                raise _err(f"{name}: SOF3 precision {p} outside BitsStored {bits_stored} .. BitsAllocated {bits_allocated}")
            sof = (p, body[6])
        elif m in _SOF_NAMES:
            raise NotImplementedError(f"{name}: JPEG {_SOF_NAMES[m]} (SOF marker {m:02X}): only lossless Process 14 "
                                      "(SOF3, Huffman) is read")
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
        raise _err(f"{name}: scan before the frame header (no SOF3)")
    if len(body) < 1 or body[0] != 1 or len(body) != 6:
        raise _err(f"{name}: scan with {body[0] if body else 0} components (one is read)")
    cs, td, ss, se, ahal = body[1], body[2] >> 4, body[3], body[4], body[5]
    if cs != sof[1]:
        raise _err(f"{name}: scan component {cs} is not the frame's component {sof[1]}")
    if not 1 <= ss <= 7 or se != 0 or (ahal >> 4) != 0:
        raise _err(f"{name}: scan parameters Ss {ss}, Se {se}, Ah {ahal >> 4} (lossless: predictor 1-7, 0, 0)")
    pt = ahal & 15
    if pt >= sof[0]:
        raise _err(f"{name}: point transform {pt} >= precision {sof[0]}")
    if td not in tables:
        raise _err(f"{name}: the scan uses Huffman table {td}, which no DHT defined")
    counts, values = tables[td]
    _check_table(counts, values, name)
    if restart and restart % cols:
        raise NotImplementedError(f"{name}: restart interval of {restart} samples is not a whole number of {cols}-sample rows")
    restart_rows = restart // cols
    ecs = np.frombuffer(buf, dtype=np.uint8, offset=pos)
    unstuffed, bounds, term = _segments(ecs, name)
    marker = int(ecs[term + 1])
    if marker == 0xDA:
        raise _err(f"{name}: more than one scan (only single-scan frames are read)")
    if marker == 0xDC:
        raise _err(f"{name}: DNL marker (number of lines defined after the scan) is not read")
    if marker != 0xD9:
        raise _err(f"{name}: marker FF{marker:02X} after the scan (EOI expected)")
    n_seg = -(-rows // restart_rows) if restart_rows else 1
    if len(bounds) - 1 != n_seg:
        raise _err(f"{name}: {len(bounds) - 1} restart intervals, {n_seg} expected for {rows} rows")
    return Frame(name, rows, cols, sof[0], pt, ss, restart_rows if restart_rows < rows else 0, counts, values, unstuffed,
                 bounds)


def _check_table(counts: bytes, values: bytes, name: str) -> None:
    if any(v > 16 for v in values):
        raise _err(f"{name}: Huffman table holds SSSS values above 16")
    code = 0
    for length in range(1, 17):
        code += counts[length - 1]
        if code > (1 << length):
            raise _err(f"{name}: Huffman table code counts exceed {length}-bit codes")
        code <<= 1


def expand_table(counts: bytes, values: bytes) -> np.ndarray:
    """A DHT table -> uint32 [TABLE_WORDS] lookup form (layout: include/boa_hip.h, boa_ljpeg_decode)."""
    look = np.zeros(1 << LOOKUP_BITS, dtype=np.uint16)
    maxcode = np.full(18, -1, dtype=np.int32)
    valoff = np.zeros(18, dtype=np.int32)
    code = k = 0
    for length in range(1, 17):
        n = counts[length - 1]
        if n:
            valoff[length] = k - code
            maxcode[length] = code + n - 1
        for _ in range(n):
            if length <= LOOKUP_BITS:
                sh = LOOKUP_BITS - length
                look[code << sh:(code + 1) << sh] = (length << 8) | values[k]
            code += 1
            k += 1
        code <<= 1
    hv = np.zeros(256, dtype=np.uint8)
    hv[:len(values)] = np.frombuffer(values, dtype=np.uint8)
    out = np.zeros(TABLE_WORDS, dtype=np.uint32)
    out[:256] = look.view(np.uint32)
    out[256:274] = maxcode.view(np.uint32)
    out[274:292] = valoff.view(np.uint32)
    out[292:356] = hv.view(np.uint32)
    return out


def build_batch(frames: Sequence[Frame], subseq_bytes: int = 128):
    """Frames -> (data uint8, frame table, segment table, subsequence table, expanded tables) as `boa_ljpeg_decode` takes them."""
    if subseq_bytes < 4:
        raise ValueError(f"subseq_bytes {subseq_bytes} < 4")
    keys: Dict[Tuple[bytes, bytes], int] = {}
    tabs: List[np.ndarray] = []
    parts, ftab, segs, subs = [], np.zeros((len(frames), FRAME_WORDS), dtype=np.int64), [], []
    off = n_seg = n_sub = 0
    for f, fr in enumerate(frames):
        key = (fr.counts, fr.values)
        if key not in keys:
            keys[key] = len(tabs)
            tabs.append(expand_table(*key))
        b = fr.seg_bounds
        lo, hi = b[:-1], b[1:]
        nsub = np.maximum(1, -(-(hi - lo) // subseq_bytes))
        first = n_sub + np.concatenate([[0], np.cumsum(nsub)[:-1]])
        k = np.arange(int(nsub.sum())) - np.repeat(first - n_sub, nsub)
        seg_idx = np.repeat(np.arange(len(lo)) + n_seg, nsub)
        subs.append(np.stack([np.repeat(lo, nsub) + k * subseq_bytes, seg_idx], axis=1))
        R = fr.restart_rows or fr.rows
        segs.append(np.stack([lo, hi, np.arange(len(lo)) * R, first], axis=1))
        ftab[f, :14] = [off & 0xFFFFFFFF, off >> 32, len(fr.data), fr.rows, fr.cols, fr.precision, fr.pt, fr.predictor,
                        fr.restart_rows, keys[key], n_seg, len(lo), n_sub, int(nsub.sum())]
        padded = (len(fr.data) + 3) & ~3
        parts.append(fr.data)
        if padded > len(fr.data):
            parts.append(np.zeros(padded - len(fr.data), dtype=np.uint8))
        off += padded
        n_seg += len(lo)
        n_sub += int(nsub.sum())
    data = np.concatenate(parts + [np.zeros(8, dtype=np.uint8)])
    return (data, ftab.astype(np.uint32).view(np.int32),
            np.concatenate(segs).astype(np.int32), np.concatenate(subs).astype(np.int32), np.stack(tabs))


def decode_frames(ctx, frames: Sequence[Frame], *, serial: bool = False, subseq_bytes: int = 128) -> Tuple[np.ndarray, np.ndarray]:
    """Decode a batch of frames of one size on the device in one call -> (uint16 [n][rows][cols] stored bit patterns, int32
    status per frame: 0 ok, else a key of STATUS).  serial: the one-lane-per-frame reference decoder; subseq_bytes: the size of
    the subsequences of the parallel decoder (small values force many resynchronisations)."""
    from . import _lib
    if not frames:
        raise ValueError("no frames")
    rows, cols = frames[0].rows, frames[0].cols
    if any((f.rows, f.cols) != (rows, cols) for f in frames):
        raise ValueError("the frames of one batch must have one size")
    data, ftab, segs, subs, tabs = build_batch(frames, subseq_bytes)
    d_data = ctx.from_numpy(data)
    out = ctx.alloc(len(frames) * rows * cols * 2)
    status = np.zeros(len(frames), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    tabs = np.ascontiguousarray(tabs)
    _lib.check(ctx.lib.boa_ljpeg_decode(
        ctx.h, d_data.vp, data.nbytes, len(frames), ftab.ctypes.data_as(ip), len(segs), segs.ctypes.data_as(ip), len(subs),
        subs.ctypes.data_as(ip), len(tabs), tabs.ctypes.data_as(C.POINTER(C.c_uint32)), out.vp, status.ctypes.data_as(ip),
        1 if serial else 0), "boa_ljpeg_decode")
    px = out.download((len(frames), rows, cols), np.uint16)
    d_data.free()
    out.free()
    return px, status


def decode(ctx, frames: Sequence[Frame], **kw) -> np.ndarray:
    """`decode_frames`, raising DicomError naming the first file whose frame did not decode."""
    px, status = decode_frames(ctx, frames, **kw)
    bad = np.flatnonzero(status)
    if len(bad):
        f = frames[int(bad[0])]
        raise _err(f"{f.name}: JPEG Lossless decode failed: {STATUS.get(int(status[bad[0]]), 'status %d' % status[bad[0]])}"
                   + (f" ({len(bad)} frames of the series failed)" if len(bad) > 1 else ""))
    return px
