"""Test-only RLE Lossless (DICOM PS3.5 Annex G) encoder, decoder model and DICOM wrapper, written from the standard.

Encoder: `encode_segment` (one byte plane -> one PackBits stream, in several styles a conforming or a merely tolerated encoder
may produce), `encode_frame` (header, segments most significant plane first, even padding).  Model of the decoding rule that
boa_hip's kernels follow (include/boa_hip.h, boa_rle_decode): `decode_segment`, `decode_frame`.  Model of the three chunk phases
of csrc/rle.hip, each by the plain walk and independent of the pointer doubling there: `chunk_map`, `chain`, `chunk_runs`,
`chunked_decode`.  Pinned against libtiff's PackBits encoder (through Pillow): tests/golden/rle/."""
import os
import struct

import numpy as np

from dicom_writer import write_slice as _write_native
import ljpeg_writer as _LW

RLE_LOSSLESS = "1.2.840.10008.1.2.5"
MODES = ("rows", "literal", "dense", "crossing", "noops")
NOT_LIVE = -1
T_DEAD, T_EXIT_SHIFT, T_COUNT_MASK = 0x80000000, 20, 0xFFFFF


# ------------------------------------------------------------------------------------------------ encoder
def _greedy(b: bytes):
    """Greedy PackBits tokens of one byte string: runs of two or more equal bytes become repeat controls (at most 128 each),
    the rest literal controls (at most 128 each).  No 0x80 is written."""
    a = np.frombuffer(b, dtype=np.uint8)
    if len(a) == 0:
        return []
    cut = np.flatnonzero(np.diff(a)) + 1
    starts = np.concatenate([[0], cut])
    lengths = np.diff(np.concatenate([starts, [len(a)]]))
    out, lit = [], bytearray()

    def flush():
        for i in range(0, len(lit), 128):
            piece = bytes(lit[i:i + 128])
            out.append(bytes([len(piece) - 1]) + piece)
        lit.clear()

    for s, n in zip(starts.tolist(), lengths.tolist()):
        v = b[s]
        if n == 1:
            lit.append(v)
            continue
        flush()
        while n >= 2:
            k = min(n, 128)
            if n - k == 1:                       # (leave two for the last repeat rather than a single byte)
                k -= 1
            out.append(bytes([257 - k, v]))
            n -= k
        if n:
            lit.append(v)
    flush()
    return out


def tokens(plane, mode="rows"):
    """The control tokens (control byte with its operands) of one byte plane [rows, cols] in the given style:
    rows      greedy, each row on its own: what Annex G asks of an encoder
    literal   literal runs of 128 bytes only (the last one shorter), across the row ends
    dense     one-byte literals and two-byte repeats only: the most controls per stream byte
    crossing  greedy over the whole plane: runs cross the row ends (forbidden for encoders, accepted by decoders)"""
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    flat = plane.tobytes()
    if mode == "rows":
        return [t for r in range(plane.shape[0]) for t in _greedy(plane[r].tobytes())]
    if mode == "crossing":
        return _greedy(flat)
    if mode == "literal":
        return [bytes([len(flat[i:i + 128]) - 1]) + flat[i:i + 128] for i in range(0, len(flat), 128)]
    if mode == "dense":
        out, i = [], 0
        while i < len(flat):
            if i + 1 < len(flat) and flat[i] == flat[i + 1]:
                out.append(bytes([255, flat[i]]))
                i += 2
            else:
                out.append(bytes([0, flat[i]]))
                i += 1
        return out
    raise ValueError(mode)


def encode_segment(plane, mode="rows", *, k=0, at=()):
    """One byte plane -> one segment.  mode: see `tokens`; "noops": the "rows" tokens with `k` 0x80 bytes inserted in front of
    each of the token indices `at` (default: the first, a middle and the last token)."""
    if mode != "noops":
        return b"".join(tokens(plane, mode))
    toks = tokens(plane, "rows")
    at = set(at) if len(at) else {0, len(toks) // 2, len(toks) - 1}
    return b"".join((b"\x80" * (k or 3) if i in at else b"") + t for i, t in enumerate(toks))


def planes_of(px, bits_allocated=16):
    """Stored values [rows, cols] -> the byte planes, most significant first."""
    px = np.asarray(px).astype(np.int64) & ((1 << bits_allocated) - 1)
    return [((px >> s) & 0xFF).astype(np.uint8) for s in range(bits_allocated - 8, -1, -8)]


def frame_of(segments):
    """Segments -> an RLE frame: the 64-byte header and the segments, each padded to an even length."""
    header, body = [len(segments)], b""
    for s in segments:
        header.append(64 + len(body))
        body += s + (b"\0" if len(s) % 2 else b"")
    return struct.pack("<16I", *(header + [0] * (16 - len(header)))) + body


def encode_frame(px, bits_allocated=16, mode="rows", **kw):
    return frame_of([encode_segment(p, mode, **kw) for p in planes_of(px, bits_allocated)])


# ------------------------------------------------------------------------------------------------ the decoding rule
def step(c):
    """Control byte -> (bytes consumed, bytes produced)."""
    return (c + 2, c + 1) if c < 128 else (2, 257 - c) if c > 128 else (1, 0)


def decode_segment(seg: bytes, wanted: int):
    """-> (the up to `wanted` bytes produced, status 0 / 1 = truncated)."""
    out, p = bytearray(), 0
    while len(out) < wanted and p < len(seg):
        adv, cnt = step(seg[p])
        if p + adv > len(seg):
            break
        out += seg[p + 1:p + adv] if seg[p] < 128 else seg[p + 1:p + 2] * cnt
        p += adv
    return bytes(out[:wanted]), int(len(out) < wanted)


def segments_of(frame: bytes):
    count, *off = struct.unpack_from("<16I", frame, 0)
    ends = off[1:count] + [len(frame)]
    return [frame[a:b] for a, b in zip(off[:count], ends)]


def decode_frame(frame: bytes, rows: int, cols: int):
    """-> (uint16 [rows, cols], status); the samples of a failed frame are whatever was produced, zero filled."""
    px, status = np.zeros(rows * cols, dtype=np.uint16), 0
    for seg in segments_of(frame):
        got, st = decode_segment(seg, rows * cols)
        plane = np.zeros(rows * cols, dtype=np.uint16)
        plane[:len(got)] = np.frombuffer(got, dtype=np.uint8)
        px = (px << 8) | plane
        status |= st
    return px.reshape(rows, cols), status


# ------------------------------------------------------------------------------------------------ the three chunk phases
def n_chunks(seg, cb):
    return -(-len(seg) // cb)


def chunk_map(seg: bytes, cb: int, k: int):
    """The 129 table words of chunk k: for every entry offset the bytes produced up to the chunk's end and the exit offset into
    the next chunk, or T_DEAD where a control's operands overrun the segment."""
    start = k * cb
    ln = min(cb, len(seg) - start)
    words = []
    for e in range(129):
        p, cnt, dead = e, 0, False
        while p < ln:
            adv, out = step(seg[start + p])
            if start + p + adv > len(seg):
                dead = True
                break
            p += adv
            cnt += out
        words.append(T_DEAD | cnt if dead else cnt | ((p - ln) << T_EXIT_SHIFT))
    return words


def chain(tables, wanted: int):
    """-> (total, entry per chunk (NOT_LIVE behind the end), output base per chunk)."""
    total, e, live, entries, bases = 0, 0, True, [], []
    for t in tables:
        live = live and total < wanted
        entries.append(e if live else NOT_LIVE)
        bases.append(total if live else 0)
        if not live:
            continue
        w = t[e]
        total += w & T_COUNT_MASK
        if w & T_DEAD:
            live = False
        e = (w >> T_EXIT_SHIFT) & 0xFF
    return total, entries, bases


def chunk_runs(seg: bytes, cb: int, k: int, e: int):
    """[(position in the chunk, offset in the chunk's output)] of the controls on the chain from entry e that produce bytes."""
    start = k * cb
    ln = min(cb, len(seg) - start)
    p, off, runs = e, 0, []
    while p < ln:
        adv, out = step(seg[start + p])
        if start + p + adv > len(seg):
            break
        if out:
            runs.append((p, off))
        p += adv
        off += out
    return runs


def chunked_decode(seg: bytes, cb: int, wanted: int):
    """The three phases strung together -> (bytes, status): equal to decode_segment by construction of the phases."""
    tables = [chunk_map(seg, cb, k) for k in range(n_chunks(seg, cb))]
    total, entries, bases = chain(tables, wanted)
    out = bytearray(wanted)
    for k, (e, base) in enumerate(zip(entries, bases)):
        if e == NOT_LIVE:
            continue
        for p, off in chunk_runs(seg, cb, k, e):
            c = seg[k * cb + p]
            adv, cnt = step(c)
            body = seg[k * cb + p + 1:k * cb + p + adv] if c < 128 else seg[k * cb + p + 1:k * cb + p + 2] * cnt
            room = max(0, wanted - (base + off))
            out[base + off:base + off + min(cnt, room)] = body[:room]
    return bytes(out[:min(total, wanted)]), int(total < wanted)


def fnv(b: bytes) -> int:
    h = 1469598103934665603
    for v in b:
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


# ------------------------------------------------------------------------------------------------ DICOM files
def _set_bits_allocated(buf: bytes, bits: int) -> bytes:
    tag = struct.pack("<HH2sH", 0x0028, 0x0100, b"US", 2)
    i = buf.index(tag)
    return buf[:i + 8] + struct.pack("<H", bits) + buf[i + 10:]


def write_slice(path, pixels, frame=None, *, bits_allocated=16, mode="rows", fragments=1, bot=False, **kw):
    """One RLE Lossless file: dicom_writer.write_slice with the RLE syntax, its native PixelData replaced by the encapsulated
    `frame` (default: `encode_frame(pixels, bits_allocated, mode)`); BitsAllocated 8 is patched into the written element."""
    if frame is None:
        frame = encode_frame(pixels, bits_allocated, mode)
    if bits_allocated == 8:
        kw.setdefault("bits_stored", 8)
    _LW.write_compressed_slice(path, pixels, frame, transfer_syntax=RLE_LOSSLESS, fragments=fragments, bot=bot, **kw)
    if bits_allocated != 16:
        with open(path, "rb") as f:
            buf = f.read()
        with open(path, "wb") as f:
            f.write(_set_bits_allocated(buf, bits_allocated))


def write_native_slice8(path, pixels, **kw):
    """An uncompressed 8-bit slice: dicom_writer.write_slice, its 16-bit PixelData replaced and BitsAllocated patched."""
    px = np.asarray(pixels)
    kw.setdefault("bits_stored", 8)
    _write_native(path, px, **kw)
    with open(path, "rb") as f:
        buf = f.read()
    cut = 12 + px.size * 2
    assert buf[-cut:-cut + 4] == struct.pack("<HH", 0x7FE0, 0x0010)
    body = px.astype("i1" if kw.get("signed") else "u1").tobytes()
    body += b"\0" * (len(body) % 2)
    with open(path, "wb") as f:
        f.write(_set_bits_allocated(buf[:-cut], 8) + struct.pack("<HH2sHI", 0x7FE0, 0x0010, b"OB", 0, len(body)) + body)


def write_series(folder, volume_zyx_stored, *, compressed=True, bits_allocated=16, origin=(-100.0, -120.0, 50.0),
                 iop=(1, 0, 0, 0, 1, 0), dz=1.5, name="IM%04d.dcm", mode="rows", **kw):
    """A series of RLE Lossless slices (or, compressed=False, of native slices of the same BitsAllocated): slice z at
    origin + z * dz * normal."""
    os.makedirs(folder, exist_ok=True)
    iop_a = np.asarray(iop, dtype=float)
    normal = np.cross(iop_a[:3], iop_a[3:])
    paths = []
    for z in range(len(volume_zyx_stored)):
        p = os.path.join(folder, name % z)
        geo = dict(ipp=np.asarray(origin, dtype=float) + z * dz * normal, iop=iop, instance=z + 1)
        if compressed:
            write_slice(p, volume_zyx_stored[z], bits_allocated=bits_allocated, mode=mode, **geo, **kw)
        elif bits_allocated == 8:
            write_native_slice8(p, volume_zyx_stored[z], **geo, **kw)
        else:
            _write_native(p, volume_zyx_stored[z], **geo, **kw)
        paths.append(p)
    return paths


# ------------------------------------------------------------------------------------------------ streams built on purpose
def _literal(data: bytes) -> bytes:
    assert 1 <= len(data) <= 128
    return bytes([len(data) - 1]) + data


def boundary_cases(cb=256, seed=5):
    """{name: (segment, wanted bytes)}: single segments (= 8-bit frames of 1 x wanted) whose controls sit on purpose against the
    boundaries of chunks of `cb` bytes, and malformed ones.  The expected output and status are `decode_segment`'s."""
    rng = np.random.default_rng(seed)
    noise = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()   # noqa: E731

    def upto(n):
        """Literal tokens of exactly n stream bytes."""
        out = b""
        while n - len(out) > 130:
            out += _literal(noise(128))
        rest = n - len(out)
        if rest > 129:
            out += _literal(noise(60))
            rest = n - len(out)
        return out + (_literal(noise(rest - 1)) if rest >= 2 else b"\x80" * rest)

    tail = _literal(noise(77)) + bytes([257 - 9, 3]) + _literal(noise(128))
    cases = {}
    for name, seg in {
        "c127_on_last_byte": upto(cb - 1) + _literal(noise(128)) + tail,           # the next chunk is entered at offset 128
        "repeat_on_last_byte": upto(cb - 1) + bytes([257 - 100, 0xAB]) + tail,     # its operand is the next chunk's first byte
        "ends_on_boundary": upto(2 * cb),
        "noop_flood": _literal(noise(40)) + b"\x80" * (2 * cb + 100) + tail,       # whole chunks that produce nothing
        "noops_then_end": tail + b"\x80" * 700,
        "dense": encode_segment(np.frombuffer(noise(3 * cb) + bytes(cb), dtype=np.uint8).reshape(4, cb), "dense"),
    }.items():
        assert len(upto(cb - 1)) == cb - 1 and len(upto(2 * cb)) == 2 * cb
        cases[name] = (seg, len(decode_segment(seg, 1 << 30)[0]))
    body = upto(3 * cb - 17)
    n = len(decode_segment(body, 1 << 30)[0])
    cases["last_run_clipped"] = (body + bytes([257 - 128, 0x5A]), n + 5)          # a 128-byte repeat crosses the wanted count
    cases["trailing_pad"] = (body + b"\0", n)
    cases["trailing_garbage"] = (body + noise(300) + bytes([127, 1, 2]), n)       # ignored, overrunning control included
    cases["cut_short"] = (body[:len(body) // 2], n)                               # status 1
    cases["operand_overrun"] = (body[:cb + 40] + bytes([100]) + noise(20), n)     # a literal control that wants 101 bytes: status 1
    cases["repeat_without_operand"] = (upto(cb) + bytes([200]), 10 * cb)          # the control is the segment's last byte: status 1
    cases["empty_after_header"] = (b"\x80", 4)                                    # nothing produced: status 1
    return cases
