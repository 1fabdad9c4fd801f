"""Test-only JPEG Lossless encoder (ITU T.81 Process 14, one component, Huffman) and DICOM wrapper, written from the standard:
vectorised numpy (a 512 x 512 slice in tens of milliseconds), any predictor 1-7, point transform, P = 2..16, optional restart
intervals of whole rows, optimal Huffman tables (T.81 K.2 with the K.3 16-bit limit) so that codes of up to 16 bits occur.
Pinned against libjpeg-turbo (through Pillow) at P = 8: tests/test_ljpeg_writer_cpu.py and tests/golden/ljpeg/."""
import os
import struct

import numpy as np

from dicom_writer import write_slice

JPEG_LOSSLESS = "1.2.840.10008.1.2.4.57"
JPEG_LOSSLESS_SV1 = "1.2.840.10008.1.2.4.70"


def differences(x, *, precision, predictor=1, pt=0, restart_rows=0):
    """x: [rows, cols] samples (< 2^P) -> T.81 H.1.2 differences modulo 2^16 (uint16 patterns) of the point-transformed samples."""
    x = np.asarray(x).astype(np.int64) >> pt
    rows, cols = x.shape
    ra, rb, rc = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    ra[:, 1:], rb[1:, :], rc[1:, 1:] = x[:, :-1], x[:-1, :], x[:-1, :-1]
    px = {1: ra, 2: rb, 3: rc, 4: ra + rb - rc, 5: ra + ((rb - rc) >> 1), 6: rb + ((ra - rc) >> 1), 7: (ra + rb) >> 1}[predictor].copy()
    first = np.arange(rows) % (restart_rows or rows) == 0
    px[first, 1:] = ra[first, 1:]
    px[~first, 0] = rb[~first, 0]
    px[first, 0] = 1 << (precision - pt - 1)
    return (x - px) & 0xFFFF


def categories(d):
    """uint16 difference patterns -> (SSSS, extra-bit values)."""
    d = np.asarray(d).astype(np.int64)
    v = np.where(d >= 32768, d - 65536, d)            # -32768 .. 32767; -32768 is SSSS 16 (no extra bits)
    a = np.abs(v)
    s = np.zeros(a.shape, dtype=np.int64)
    nz = a > 0
    s[nz] = np.floor(np.log2(a[nz])).astype(np.int64) + 1
    extra = np.where(v >= 0, v, v + (1 << np.minimum(s, 62)) - 1)
    extra = np.where(s >= 16, 0, extra)
    return s, extra


def optimal_table(freq):
    """T.81 K.2 (Figure K.1 code sizes, K.3 Adjust_BITS to 16 bits, Sort_input): SSSS frequencies (17) -> (counts[16], values)."""
    f = [int(v) for v in freq] + [1]                  # symbol 17 = the reserved code point (no code of all 1 bits)
    n = len(f)
    size, others = [0] * n, [-1] * n
    while True:
        cand = [v for v in range(n) if f[v] > 0]
        if len(cand) < 2:
            break
        v1 = min(cand, key=lambda v: (f[v], -v))
        v2 = min((v for v in cand if v != v1), key=lambda v: (f[v], -v))
        f[v1] += f[v2]
        f[v2] = 0
        size[v1] += 1
        while others[v1] != -1:
            v1 = others[v1]
            size[v1] += 1
        others[v1] = v2
        size[v2] += 1
        while others[v2] != -1:
            v2 = others[v2]
            size[v2] += 1
    bits = [0] * 33
    for v in range(n):
        if size[v]:
            bits[size[v]] += 1
    i = 32
    while i > 16:
        if bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        else:
            i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                      # the reserved code point goes
    values = [v for v in sorted(range(n - 1), key=lambda v: (size[v], v)) if size[v] > 0]
    return bytes(bits[1:17]), bytes(values)


def canonical_codes(counts, values):
    """T.81 C.2: (counts, values) -> {SSSS: (code, length)}."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _pack(lengths, vals):
    """Codewords (MSB first) -> bytes, padded with 1 bits, FF stuffed with 00."""
    lengths = np.asarray(lengths, dtype=np.int64)
    total = int(lengths.sum())
    starts = np.cumsum(lengths) - lengths
    idx = np.repeat(np.arange(len(lengths)), lengths)
    k = np.arange(total) - starts[idx]
    bits = ((np.asarray(vals, dtype=np.uint64)[idx] >> (lengths[idx] - 1 - k).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    bits = np.concatenate([bits, np.ones((-total) % 8, dtype=np.uint8)])
    b = np.packbits(bits)
    ff = b == 0xFF
    out = np.repeat(b, 1 + ff.astype(np.int64))
    pos = np.arange(len(b)) + np.cumsum(ff) - ff
    out[pos[ff] + 1] = 0
    return out.tobytes()


def encode(pixels, *, precision, predictor=1, pt=0, restart_rows=0, table=None, table_id=0, extra_tables=()):
    """pixels: [rows, cols] samples < 2^precision -> one JPEG Lossless frame (SOI .. EOI).  table: (counts, values) to use
    instead of the optimal one; extra_tables: further (id, counts, values) DHT entries written but not used by the scan."""
    x = np.asarray(pixels)
    rows, cols = x.shape
    assert 2 <= precision <= 16 and 0 <= pt < precision and 1 <= predictor <= 7
    assert int(x.max(initial=0)) < (1 << precision) and int(x.min(initial=0)) >= 0
    d = differences(x, precision=precision, predictor=predictor, pt=pt, restart_rows=restart_rows)
    s, extra = categories(d)
    if table is None:
        table = optimal_table(np.bincount(s.ravel(), minlength=17))
    counts, values = table
    codes = canonical_codes(counts, values)
    code = np.zeros(17, dtype=np.int64)
    clen = np.zeros(17, dtype=np.int64)
    for v, (c, ln) in codes.items():
        code[v], clen[v] = c, ln
    assert all(int(v) in codes for v in np.unique(s)), "table lacks a category"
    nbits = np.where(s >= 16, 0, s)
    lengths = clen[s] + nbits
    vals = (code[s] << nbits) | extra
    R = restart_rows or rows
    ecs = b""
    for k, r0 in enumerate(range(0, rows, R)):
        if k:
            ecs += bytes([0xFF, 0xD0 + (k - 1) % 8])
        ecs += _pack(lengths[r0:r0 + R].ravel(), vals[r0:r0 + R].ravel())
    seg = lambda m, body: bytes([0xFF, m]) + struct.pack(">H", len(body) + 2) + body   # noqa: E731
    dht = b"".join(bytes([t]) + bytes(c) + bytes(v) for t, c, v in [(table_id, counts, values)] + list(extra_tables))
    out = b"\xFF\xD8" + seg(0xC4, dht)
    out += seg(0xC3, struct.pack(">BHHB", precision, rows, cols, 1) + bytes([1, 0x11, 0]))
    if restart_rows:
        out += seg(0xDD, struct.pack(">H", restart_rows * cols))
    out += seg(0xDA, bytes([1, 1, table_id << 4, predictor, 0, pt]))
    return out + ecs + b"\xFF\xD9"


def encapsulate(frame: bytes, *, fragments=1, bot=False) -> bytes:
    """PS3.5 A.4: an undefined-length (7FE0,0010) OB with a Basic Offset Table item (empty, or one offset) and the frame in
    `fragments` even-length fragments, then the sequence delimiter."""
    if len(frame) % 2:
        frame += b"\0"
    n = len(frame) // 2
    cuts = [2 * (n * i // fragments) for i in range(fragments + 1)]
    out = struct.pack("<HH2sHI", 0x7FE0, 0x0010, b"OB", 0, 0xFFFFFFFF)
    out += struct.pack("<HHI", 0xFFFE, 0xE000, 4 if bot else 0) + (struct.pack("<I", 0) if bot else b"")
    for a, b in zip(cuts[:-1], cuts[1:]):
        out += struct.pack("<HHI", 0xFFFE, 0xE000, b - a) + frame[a:b]
    return out + struct.pack("<HHI", 0xFFFE, 0xE0DD, 0)


def write_compressed_slice(path, pixels, stream, *, transfer_syntax=JPEG_LOSSLESS_SV1, fragments=1, bot=False, **kw):
    """dicom_writer.write_slice with the given syntax, its native PixelData (the file's last element) replaced by the
    encapsulated `stream`."""
    write_slice(path, pixels, transfer_syntax=transfer_syntax, **kw)
    with open(path, "rb") as f:
        buf = f.read()
    cut = 12 + np.asarray(pixels).size * 2
    assert buf[-cut:-cut + 4] == struct.pack("<HH", 0x7FE0, 0x0010)
    with open(path, "wb") as f:
        f.write(buf[:-cut] + encapsulate(stream, fragments=fragments, bot=bot))


def stored_pattern(pixels, bits_stored):
    """Stored values (signed or not) -> the unsigned BitsStored-bit samples a Process-14 encoder codes."""
    return np.asarray(pixels).astype(np.int64) & ((1 << bits_stored) - 1)


def write_compressed_series(folder, volume_zyx_stored, *, origin=(-100.0, -120.0, 50.0), iop=(1, 0, 0, 0, 1, 0), dz=1.5,
                            transfer_syntax=JPEG_LOSSLESS_SV1, predictor=1, pt=0, restart_rows=0, bits_stored=16,
                            name="IM%04d.dcm", **kw):
    """dicom_writer.write_series for JPEG Lossless: slice z at origin + z * dz * normal, P = bits_stored."""
    os.makedirs(folder, exist_ok=True)
    iop_a = np.asarray(iop, dtype=float)
    normal = np.cross(iop_a[:3], iop_a[3:])
    paths = []
    for z in range(len(volume_zyx_stored)):
        px = volume_zyx_stored[z]
        stream = encode(stored_pattern(px, bits_stored), precision=bits_stored, predictor=predictor, pt=pt,
                        restart_rows=restart_rows)
        p = os.path.join(folder, name % z)
        write_compressed_slice(p, px, stream, transfer_syntax=transfer_syntax, ipp=np.asarray(origin, dtype=float) + z * dz * normal,
                               iop=iop, instance=z + 1, bits_stored=bits_stored, **kw)
        paths.append(p)
    return paths
