"""JPEG 2000 (ITU T.800, one component, one tile) for DICOM CT: transfer syntaxes 1.2.840.10008.1.2.4.90 (lossless only) and
1.2.840.10008.1.2.4.91, holding the reversible 5/3 transform or the irreversible 9/7 transform with scalar quantisation (derived
or expounded); the stream decides, not the transfer syntax.  A reversible .91 stream may be lossy too: its layers stop code blocks
before their last coding pass.  Such blocks are reconstructed as OpenJPEG reconstructs them (every coefficient at the midpoint of
what its undecoded bit-planes leave open), and a 9/7 stream is dequantised, transformed and rounded in OpenJPEG's float32
arithmetic (csrc/j2k_dwt97.h), so the pixels equal the reference's in every case.  The reference reads these
series through GDCM / OpenJPEG (BOA/compute/io.py:254-259); here the host parses the codestream and runs tier-2, and tier-1 and
the inverse wavelet transform of the whole series run in one batched HIP call (csrc/j2k.hip, `boa_j2k_decode`).

Host side (this module, numpy only, no device): `parse_frame` reads the main and tile-part headers (SIZ, COD / COC, QCD / QCC;
COM, TLM, PLM, PLT, CRG skipped; everything this reader does not decode is refused by name) and walks the packets in progression
order (T.800 Annex B: tag trees, pass counts, Lblock and lengths), giving a flat table of code blocks whose contributions are
concatenated across layers.  Device side: `decode_frames`.
"""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

J2K_LOSSLESS = "1.2.840.10008.1.2.4.90"     # JPEG 2000 Image Compression (Lossless Only)
J2K = "1.2.840.10008.1.2.4.91"              # JPEG 2000 Image Compression (reversible or irreversible)
SYNTAXES = (J2K_LOSSLESS, J2K)

# include/boa_hip.h: BOA_J2K_FRAME_WORDS, BOA_J2K_F_*, BOA_J2K_BLOCK_WORDS, BOA_J2K_B_*
FRAME_WORDS, BLOCK_WORDS = 12, 12
STATUS = {1: "invalid code-block data (more coding passes than bit-planes, or magnitudes beyond 30 bits)"}
ORIENT = {"LL": 0, "HL": 1, "LH": 2, "HH": 3}

_PROGRESSIONS = ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL")
_CBLK_STYLE = ((0x01, "selective arithmetic coding bypass (BYPASS)"), (0x02, "context reset on each pass (RESET)"),
               (0x04, "termination on each pass (TERMALL)"), (0x08, "vertically causal context (VCAUSAL)"),
               (0x10, "predictable termination (PTERM)"), (0x20, "segmentation symbols (SEGSYM)"))
_JP2_SIGNATURE = b"\x00\x00\x00\x0cjP  \r\n\x87\n"


def _err(msg: str):
    from .dicom import DicomError
    return DicomError(msg)


@dataclass
class Frame:
    """One parsed JPEG 2000 frame: the code-block table of its only tile-component and the blocks' concatenated data."""
    name: str
    rows: int
    cols: int
    precision: int                 # P, 1..16
    signed: bool
    levels: int                    # decomposition levels NL
    blocks: np.ndarray             # int64 [n][8]: orientation, x0, y0 (Mallat position), w, h, bit-planes, passes, bytes
    data: bytes                    # the blocks' data, block after block, in table order
    transform: int = 1             # 1 reversible 5/3, 0 irreversible 9/7 (the COD / COC field)
    band: Optional[np.ndarray] = None       # int64 [n]: the block's subband, 0 LL, 1 + 3 (r - 1) + (0 HL, 1 LH, 2 HH) of resolution r
    band_mb: Optional[np.ndarray] = None    # int64 [3 NL + 1]: magnitude bit-planes M_b = G + eps_b - 1 of every subband
    steps: Optional[np.ndarray] = None      # float32 [3 NL + 1], 9/7 only: step_b = (1 + mu_b / 2048) 2^(P - eps_b)


@dataclass
class _Coding:
    levels: int
    xcb: int
    ycb: int
    style: int
    transform: int
    precincts: List[Tuple[int, int]]   # (PPx, PPy) per resolution


class _Reader:
    """Big-endian fields of a marker segment; running past its end is a DicomError naming the segment."""

    def __init__(self, body: bytes, what: str, name: str):
        self.b, self.p, self.what, self.name = body, 0, what, name

    def take(self, fmt: str):
        n = struct.calcsize(fmt)
        if self.p + n > len(self.b):
            raise _err(f"{self.name}: {self.what} marker segment truncated")
        v = struct.unpack_from(fmt, self.b, self.p)
        self.p += n
        return v if len(v) > 1 else v[0]


def unwrap_jp2(buf: bytes, name: str = "") -> bytes:
    """A JP2 file (ISO 15444-1 Annex I) -> the contents of its contiguous codestream box ('jp2c'); a bare codestream is returned
    unchanged."""
    if not buf.startswith(_JP2_SIGNATURE):
        return buf
    pos = 0
    while pos + 8 <= len(buf):
        lbox, tbox = struct.unpack_from(">I4s", buf, pos)
        head = 8
        if lbox == 1:
            if pos + 16 > len(buf):
                break
            lbox, head = struct.unpack_from(">Q", buf, pos + 8)[0], 16
        end = len(buf) if lbox == 0 else pos + lbox
        if lbox != 0 and (lbox < head or end > len(buf)):
            raise _err(f"{name}: JP2 box {tbox!r} of length {lbox} overruns the frame")
        if tbox == b"jp2c":
            return buf[pos + head:end]
        pos = end
    raise _err(f"{name}: JP2 file without a contiguous codestream box (jp2c)")


def _cod_params(r: _Reader, scod_precincts: bool, name: str) -> _Coding:
    levels, xcb, ycb, style, transform = r.take(">BBBBB")
    if levels > 32:
        raise _err(f"{name}: {levels} decomposition levels (at most 32)")
    if transform not in (0, 1):
        raise _err(f"{name}: wavelet transform {transform} (0 = 9/7, 1 = 5/3)")
    if xcb > 8 or ycb > 8 or xcb + ycb > 8:
        raise _err(f"{name}: code-block size exponents {xcb + 2}, {ycb + 2} (each 2..10, sum at most 12)")
    for bit, what in _CBLK_STYLE:
        if style & bit:
            raise NotImplementedError(f"{name}: code-block style {what} is not read")
    if style & ~0x3F:
        raise _err(f"{name}: code-block style {style:#x}")
    if scod_precincts:
        pp = []
        for k in range(levels + 1):
            v = r.take(">B")
            pp.append((v & 15, v >> 4))
            if k > 0 and (v & 15 == 0 or v >> 4 == 0):
                raise _err(f"{name}: precinct size exponent 0 at resolution {k}")
    else:
        pp = [(15, 15)] * (levels + 1)
    if r.p != len(r.b):
        raise _err(f"{name}: {r.what} marker segment of {len(r.b) + 2} bytes, {r.p + 2} expected")
    return _Coding(levels, xcb + 2, ycb + 2, style, transform, pp)


def _quant(r: _Reader, name: str) -> Tuple[int, int, List[int]]:
    """Sqcd / Sqcc and what follows -> (style, guard bits, values): style 0 an exponent per subband, style 1 (derived) the one
    16-bit eps << 11 | mu of the LL band, style 2 (expounded) one such value per subband."""
    sq = r.take(">B")
    style, guard = sq & 31, sq >> 5
    if style not in (0, 1, 2):
        raise _err(f"{name}: quantisation style {style}")
    if style == 0:
        return style, guard, [b >> 3 for b in r.b[r.p:]]
    if style == 1:
        return style, guard, [r.take(">H")]
    vals = []
    while r.p < len(r.b):
        vals.append(r.take(">H"))
    return style, guard, vals


def _check_pair(transform: int, style: int, name: str):
    """The wavelet transform and the quantisation style that hold for the component have to belong together: 5/3 without
    quantisation, 9/7 with scalar quantisation."""
    if transform == 0 and style == 0:
        raise NotImplementedError(f"{name}: irreversible 9/7 wavelet transform without scalar quantisation: lossy JPEG 2000 is not "
                                  "read in this form")
    if transform == 1 and style != 0:
        raise NotImplementedError(f"{name}: scalar quantisation ({'derived' if style == 1 else 'expounded'}) with the reversible "
                                  "5/3 transform is not read")


def _band_table(levels: int, style: int, vals: List[int], precision: int, name: str):
    """-> (eps_b per subband, step_b float32 per subband or None without quantisation); subbands LL, then HL LH HH of
    resolutions 1 .. NL.  Derived quantisation (T.800 E-5): eps_b = eps_0 - (r - 1) from resolution 2 on (never below 0, as
    OpenJPEG has it), mu_b = mu_0."""
    nb = 3 * levels + 1
    if style == 1:
        e0, mu = vals[0] >> 11, vals[0] & 0x7FF
        exps = [e0] + [max(0, e0 - (r - 1)) for r in range(1, levels + 1) for _ in range(3)]
        mants = [mu] * nb
    else:
        if len(vals) < nb:
            raise _err(f"{name}: QCD/QCC holds {len(vals)} {'exponents' if style == 0 else 'step sizes'}, {nb} subbands")
        if style == 0:
            return list(vals[:nb]), None
        exps, mants = [v >> 11 for v in vals[:nb]], [v & 0x7FF for v in vals[:nb]]
    steps = np.array([(1.0 + m / 2048.0) * 2.0 ** (precision - e) for e, m in zip(exps, mants)], dtype=np.float32)
    return exps, steps


def _tag_tree(w: int, h: int):
    """A tag tree over w x h leaves: (value, low, parent index) lists, leaves first; values start at 'unknown' (a large value)."""
    dims = [(w, h)]
    while dims[-1] != (1, 1):
        dims.append(((dims[-1][0] + 1) // 2, (dims[-1][1] + 1) // 2))
    off = [0]
    for a, b in dims:
        off.append(off[-1] + a * b)
    parent = [-1] * off[-1]
    for lv in range(len(dims) - 1):
        a, _ = dims[lv]
        pa = dims[lv + 1][0]
        for i in range(off[lv + 1] - off[lv]):
            y, x = divmod(i, a)
            parent[off[lv] + i] = off[lv + 1] + (y // 2) * pa + x // 2
    n = off[-1]
    return [1 << 30] * n, [0] * n, parent


class _Bits:
    """Packet-header bits (T.800 B.10.1): MSB first; a byte after 0xFF carries 7 bits."""
    __slots__ = ("b", "pos", "end", "buf", "ct", "name")

    def __init__(self, b: bytes, pos: int, end: int, name: str):
        self.b, self.pos, self.end, self.buf, self.ct, self.name = b, pos, end, 0, 0, name

    def bit(self) -> int:
        if self.ct == 0:
            if self.pos >= self.end:
                raise _err(f"{self.name}: packet header runs past the end of the tile")
            self.ct = 7 if self.buf == 0xFF else 8
            self.buf = self.b[self.pos]
            self.pos += 1
        self.ct -= 1
        return (self.buf >> self.ct) & 1

    def bits(self, n: int) -> int:
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def align(self) -> int:
        """End of the header: a header whose last byte is 0xFF is followed by one more (stuffing) byte.  -> the body's start."""
        if self.ct >= 0 and self.buf == 0xFF:
            if self.pos >= self.end:
                raise _err(f"{self.name}: packet header runs past the end of the tile")
            self.pos += 1
        return self.pos


def _tag_decode(tree, leaf: int, threshold: int, br: _Bits) -> bool:
    """T.800 B.10.2: decode the tag tree along the path to `leaf` up to `threshold`; -> leaf value < threshold."""
    value, low, parent = tree
    path = []
    n = leaf
    while n >= 0:
        path.append(n)
        n = parent[n]
    lo = 0
    for n in reversed(path):
        if lo > low[n]:
            low[n] = lo
        else:
            lo = low[n]
        while lo < threshold and lo < value[n]:
            if br.bit():
                value[n] = lo
            else:
                lo += 1
        low[n] = lo
    return value[leaf] < threshold


def _ceil_shift(v: int, s: int) -> int:
    return (v + (1 << s) - 1) >> s


def _tier2(tile: bytes, W: int, H: int, cod: _Coding, nlayers: int, prog: int, guard: int, exps: List[int],
           name: str) -> Tuple[np.ndarray, bytes, np.ndarray]:
    NL = cod.levels
    blocks: List[list] = []           # orient, x0, y0, w, h, Mb, then: included, zbp, passes, lblock, chunks, subband
    precincts: Dict[Tuple[int, int], list] = {}
    order = []                        # (y, x, r, p) sort keys of the precincts on the reference grid
    for r in range(NL + 1):
        d = NL - r
        wr, hr = _ceil_shift(W, d), _ceil_shift(H, d)
        ppx, ppy = cod.precincts[r]
        if r == 0:
            xcb, ycb = min(cod.xcb, ppx), min(cod.ycb, ppy)
            bands = [(0, 0, 0, wr, hr, 0, ppx, ppy)]
        else:
            wl, hl = _ceil_shift(W, d + 1), _ceil_shift(H, d + 1)
            xcb, ycb = min(cod.xcb, ppx - 1), min(cod.ycb, ppy - 1)
            bands = [(o, x0, y0, bw, bh, 3 * (r - 1) + k, ppx - 1, ppy - 1) for k, (o, x0, y0, bw, bh) in enumerate(
                [(1, wl, 0, wr - wl, hl), (2, 0, hl, wl, hr - hl), (3, wl, hl, wr - wl, hr - hl)], start=1)]
        npx, npy = _ceil_shift(wr, ppx), _ceil_shift(hr, ppy)
        for py in range(npy):
            for px in range(npx):
                entry = []
                for o, bx, by, bw, bh, sb, pbx, pby in bands:
                    x0, x1 = min(px << pbx, bw), min((px + 1) << pbx, bw)
                    y0, y1 = min(py << pby, bh), min((py + 1) << pby, bh)
                    if x1 <= x0 or y1 <= y0:
                        continue
                    cx0, cx1 = x0 >> xcb, _ceil_shift(x1, xcb)
                    cy0, cy1 = y0 >> ycb, _ceil_shift(y1, ycb)
                    ids = []
                    for cy in range(cy0, cy1):
                        for cx in range(cx0, cx1):
                            ax, ay = cx << xcb, cy << ycb
                            ids.append(len(blocks))
                            blocks.append([o, bx + ax, by + ay, min(ax + (1 << xcb), bw) - ax, min(ay + (1 << ycb), bh) - ay,
                                           guard + exps[sb] - 1, False, 0, 0, 3, [], sb])
                    entry.append((ids, _tag_tree(cx1 - cx0, cy1 - cy0), _tag_tree(cx1 - cx0, cy1 - cy0)))
                precincts[(r, py * npx + px)] = entry
                order.append(((py << (ppy + d)), (px << (ppx + d)), r, py * npx + px))
    keys = list(precincts)
    if prog in (0, 1):                # LRCP, RLCP
        packets = ([(l, k) for l in range(nlayers) for k in keys] if prog == 0 else
                   [(l, k) for r in range(NL + 1) for l in range(nlayers) for k in keys if k[0] == r])
    elif prog == 2:                   # RPCL: resolution, then position (precincts in raster order), then layer
        packets = [(l, k) for k in keys for l in range(nlayers)]
    else:                             # PCRL, CPRL (one component): position on the reference grid, resolution, layer
        packets = [(l, (r, p)) for _, _, r, p in sorted(order) for l in range(nlayers)]
    pos, end = 0, len(tile)
    for layer, key in packets:
        if pos >= end:
            raise _err(f"{name}: packet (layer {layer}, resolution {key[0]}, precinct {key[1]}) starts past the end of the tile")
        br = _Bits(tile, pos, end, name)
        contrib = []
        if br.bit():
            for ids, incl, zbp in precincts[key]:
                for leaf, i in enumerate(ids):
                    b = blocks[i]
                    if not b[6]:
                        if not _tag_decode(incl, leaf, layer + 1, br):
                            continue
                        t = 0
                        while not _tag_decode(zbp, leaf, t + 1, br):
                            t += 1
                            if t > 64:
                                raise _err(f"{name}: zero bit-plane count out of range")
                        b[6], b[7] = True, t
                    elif not br.bit():
                        continue
                    if not br.bit():
                        n = 1
                    elif not br.bit():
                        n = 2
                    else:
                        n = br.bits(2)
                        if n < 3:
                            n += 3
                        else:
                            n = br.bits(5)
                            n = 6 + n if n < 31 else 37 + br.bits(7)
                    while br.bit():
                        b[9] += 1
                        if b[9] > 32:
                            raise _err(f"{name}: Lblock out of range")
                    contrib.append((i, n, br.bits(b[9] + n.bit_length() - 1)))
        pos = br.align()
        for i, n, ln in contrib:
            if pos + ln > end:
                raise _err(f"{name}: packet data runs past the end of the tile")
            b = blocks[i]
            b[8] += n
            b[10].append(tile[pos:pos + ln])
            pos += ln
    table = np.zeros((len(blocks), 8), dtype=np.int64)
    datas = []
    for k, b in enumerate(blocks):
        data = b"".join(b[10])
        nbp = b[5] - b[7] if b[6] else 0
        if b[6] and nbp < 0:
            raise _err(f"{name}: {b[7]} zero bit-planes above the {b[5]} of the subband")
        if b[8] > 164 * nlayers:
            raise _err(f"{name}: {b[8]} coding passes in one code block")
        table[k] = (b[0], b[1], b[2], b[3], b[4], nbp, b[8], len(data))
        datas.append(data)
    return table, b"".join(datas), np.array([b[11] for b in blocks], dtype=np.int64)


def parse_frame(data: bytes, *, rows: int, cols: int, bits_allocated: int = 16, bits_stored: Optional[int] = None,
                name: str = "") -> Frame:
    """One JPEG 2000 frame (a bare codestream, or a JP2 file whose 'jp2c' box is taken) -> its code-block table.  Raises
    NotImplementedError for what this reader does not decode (named: 9/7 without scalar quantisation and 5/3 with it, several
    tiles / components, sub-sampling, code-block styles, SOP / EPH, POC, PPM, PPT, RGN), DicomError for malformed or
    inconsistent data.  The stream decides between the reversible 5/3 and the irreversible 9/7, not the transfer syntax."""
    buf = unwrap_jp2(bytes(data), name)
    if buf[:2] != b"\xFF\x4F":
        raise _err(f"{name}: compressed frame does not start with a JPEG 2000 SOC marker")
    pos = 2
    siz = None
    cod = coc = qcd = qcc = None
    scod = 0

    def segment(p):
        if p + 4 > len(buf):
            raise _err(f"{name}: marker segment overruns the frame")
        m, ln = struct.unpack_from(">HH", buf, p)
        if ln < 2 or p + 2 + ln > len(buf):
            raise _err(f"{name}: marker segment FF{m & 0xFF:02X} of length {ln} overruns the frame")
        return m, buf[p + 4:p + 2 + ln], p + 2 + ln

    def header_marker(m, body, main):
        nonlocal cod, coc, qcd, qcc, scod
        if m == 0xFF52:                                  # COD
            r = _Reader(body, "COD", name)
            scod, prog, nlay, mct = r.take(">BBHB")
            if scod & 2:
                raise NotImplementedError(f"{name}: SOP markers (start of packet) are not read")
            if scod & 4:
                raise NotImplementedError(f"{name}: EPH markers (end of packet header) are not read")
            if scod & ~7:
                raise _err(f"{name}: COD style {scod:#x}")
            if mct:
                raise NotImplementedError(f"{name}: multiple component transformation (MCT) is not read")
            if prog > 4:
                raise _err(f"{name}: progression order {prog}")
            if nlay == 0:
                raise _err(f"{name}: COD with 0 layers")
            cod = (prog, nlay, _cod_params(r, bool(scod & 1), name))
            coc = None if not main else coc
        elif m == 0xFF53:                                # COC
            r = _Reader(body, "COC", name)
            c, s = r.take(">BB")
            if c != 0:
                raise _err(f"{name}: COC for component {c} of a one-component image")
            coc = _cod_params(r, bool(s & 1), name)
        elif m == 0xFF5C:                                # QCD
            qcd = _quant(_Reader(body, "QCD", name), name)
            qcc = None if not main else qcc
        elif m == 0xFF5D:                                # QCC
            r = _Reader(body, "QCC", name)
            if r.take(">B") != 0:
                raise _err(f"{name}: QCC for a component other than 0")
            qcc = _quant(r, name)
        elif m == 0xFF5E:
            raise NotImplementedError(f"{name}: region of interest (RGN marker) is not read")
        elif m == 0xFF5F:
            raise NotImplementedError(f"{name}: progression order change (POC marker) is not read")
        elif m == 0xFF60:
            raise NotImplementedError(f"{name}: packed packet headers in the main header (PPM marker) are not read")
        elif m == 0xFF61:
            raise NotImplementedError(f"{name}: packed packet headers in a tile-part header (PPT marker) are not read")
        elif m in (0xFF64, 0xFF55, 0xFF57, 0xFF63) and main:   # COM, TLM, PLM, CRG
            pass
        elif m in (0xFF64, 0xFF58) and not main:         # COM, PLT
            pass
        else:
            raise _err(f"{name}: unexpected marker {m:04X} in the {'main' if main else 'tile-part'} header")

    while True:                                          # main header
        m, body, nxt = segment(pos)
        if m == 0xFF90:                                  # SOT
            break
        if m == 0xFF51:                                  # SIZ
            r = _Reader(body, "SIZ", name)
            _rsiz, X, Y, XO, YO, XT, YT, XTO, YTO, nc = r.take(">HIIIIIIIIH")
            if nc != 1:
                raise NotImplementedError(f"{name}: {nc} image components (Csiz): only one component is read")
            ssiz, xr, yr = r.take(">BBB")
            if XO or YO or XTO or YTO:
                raise NotImplementedError(f"{name}: non-zero image or tile origin is not read")
            if (xr, yr) != (1, 1):
                raise NotImplementedError(f"{name}: component sub-sampling {xr} x {yr} is not read")
            if XT < X or YT < Y:
                raise NotImplementedError(f"{name}: several tiles ({XT} x {YT} tiles of a {X} x {Y} image) are not read")
            prec = (ssiz & 0x7F) + 1
            if prec > 16:
                raise _err(f"{name}: SIZ precision {prec} (1..16)")
            if (Y, X) != (rows, cols):
                raise _err(f"{name}: SIZ size {Y} x {X} differs from Rows x Columns {rows} x {cols}")
            if prec > bits_allocated:
                raise _err(f"{name}: SIZ precision {prec} above BitsAllocated {bits_allocated}")
            siz = (prec, bool(ssiz & 0x80))
        else:
            if siz is None:
                raise _err(f"{name}: marker {m:04X} ahead of SIZ")
            header_marker(m, body, True)
        pos = nxt
    if siz is None or cod is None or qcd is None:
        raise _err(f"{name}: main header without {'SIZ' if siz is None else 'COD' if cod is None else 'QCD'}")
    _check_pair((coc or cod[2]).transform, (qcc or qcd)[0], name)      # the pair that holds once the whole main header is known
    parts = []
    first = True
    while True:                                          # tile-parts
        m, body, nxt = segment(pos)
        if m != 0xFF90:
            raise _err(f"{name}: marker {m:04X} where a tile-part (SOT) or EOC was expected")
        r = _Reader(body, "SOT", name)
        isot, psot, _tp, _tn = r.take(">HIBB")
        if isot != 0:
            raise _err(f"{name}: tile index {isot} in a one-tile image")
        p = nxt
        while True:
            if p + 2 > len(buf):
                raise _err(f"{name}: tile-part header overruns the frame")
            m = struct.unpack_from(">H", buf, p)[0]
            if m == 0xFF93:                              # SOD
                p += 2
                break
            m, body, p = segment(p)
            if not first and m in (0xFF52, 0xFF53, 0xFF5C, 0xFF5D):
                raise _err(f"{name}: marker {m:04X} in a tile-part header after the first")
            header_marker(m, body, False)
        if psot == 0:
            if buf[-2:] != b"\xFF\xD9":
                raise _err(f"{name}: a tile-part running to the end of the codestream, without EOC")
            parts.append(buf[p:len(buf) - 2])
            break
        tp_end = pos + psot
        if tp_end < p or tp_end > len(buf):
            raise _err(f"{name}: tile-part of {psot} bytes overruns the frame")
        parts.append(buf[p:tp_end])
        pos = tp_end
        first = False
        if pos + 2 <= len(buf) and buf[pos:pos + 2] == b"\xFF\xD9":
            break
        if pos >= len(buf):
            raise _err(f"{name}: codestream ends without EOC")
    prog, nlayers, coding = cod
    coding = coc or coding
    style, guard, vals = qcc or qcd
    _check_pair(coding.transform, style, name)                        # (a tile-part header may have replaced either)
    exps, steps = _band_table(coding.levels, style, vals, siz[0], name)
    table, bdata, band = _tier2(b"".join(parts), cols, rows, coding, nlayers, prog, guard, exps, name)
    return Frame(name, rows, cols, siz[0], siz[1], coding.levels, table, bdata, coding.transform, band,
                 guard + np.array(exps, dtype=np.int64) - 1, steps)


def build_batch(frames: Sequence[Frame]):
    """Frames -> (data uint8, frame table int32 [n][FRAME_WORDS], block table int32 [m][BLOCK_WORDS]) as `boa_j2k_decode` takes
    them; the outputs are packed frame after frame (uint16 rows x cols each)."""
    ftab = np.zeros((len(frames), FRAME_WORDS), dtype=np.int64)
    btabs, parts = [], []
    off = out = nb = 0
    for f, fr in enumerate(frames):
        n = len(fr.blocks)
        ftab[f, :10] = [out & 0xFFFFFFFF, out >> 32, fr.rows, fr.cols, fr.levels, fr.precision, int(fr.signed), nb, n, fr.transform]
        b = np.zeros((n, BLOCK_WORDS), dtype=np.int64)
        if fr.transform == 0:                            # BOA_J2K_B_STEP: the float32 bits of 0.5f * step_b
            b[:, 11] = (np.float32(0.5) * fr.steps[fr.band]).astype(np.float32).view(np.uint32)
        lens = fr.blocks[:, 7]
        starts = off + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
        b[:, 0] = f
        b[:, 1:8] = fr.blocks[:, :7]
        b[:, 8] = starts & 0xFFFFFFFF
        b[:, 9] = starts >> 32
        b[:, 10] = lens
        btabs.append(b)
        parts.append(np.frombuffer(fr.data, dtype=np.uint8))
        off += len(fr.data)
        out += fr.rows * fr.cols
        nb += n
    data = np.concatenate(parts + [np.zeros(4, dtype=np.uint8)])
    blocks = np.concatenate(btabs) if nb else np.zeros((0, BLOCK_WORDS), dtype=np.int64)
    return data, ftab.astype(np.uint32).view(np.int32), blocks.astype(np.uint32).view(np.int32)


def decode_frames(ctx, frames: Sequence[Frame]) -> Tuple[List[np.ndarray], np.ndarray]:
    """Decode a batch of frames (any sizes) on the device in one call -> ([uint16 rows x cols] per frame, samples modulo 2^16;
    int32 status per frame: 0 ok, else a key of STATUS)."""
    from . import _lib
    if not frames:
        raise ValueError("no frames")
    data, ftab, btab = build_batch(frames)
    total = sum(f.rows * f.cols for f in frames)
    d_data = ctx.from_numpy(data)
    out = ctx.alloc(total * 2)
    status = np.zeros(len(frames), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    btab = np.ascontiguousarray(btab)
    _lib.check(ctx.lib.boa_j2k_decode(ctx.h, d_data.vp, data.nbytes, len(frames), ftab.ctypes.data_as(ip), len(btab),
                                      btab.ctypes.data_as(ip), out.vp, status.ctypes.data_as(ip)), "boa_j2k_decode")
    flat = out.download((total,), np.uint16)
    d_data.free()
    out.free()
    px, o = [], 0
    for f in frames:
        px.append(flat[o:o + f.rows * f.cols].reshape(f.rows, f.cols))
        o += f.rows * f.cols
    return px, status


def decode(ctx, frames: Sequence[Frame]) -> np.ndarray:
    """`decode_frames` for frames of one size -> uint16 [n][rows][cols], raising DicomError naming the first file whose frame did
    not decode."""
    if any((f.rows, f.cols) != (frames[0].rows, frames[0].cols) for f in frames):
        raise ValueError("the frames of one series must have one size")
    px, status = decode_frames(ctx, frames)
    bad = np.flatnonzero(status)
    if len(bad):
        f = frames[int(bad[0])]
        raise _err(f"{f.name}: JPEG 2000 decode failed: {STATUS.get(int(status[bad[0]]), 'status %d' % status[bad[0]])}"
                   + (f" ({len(bad)} frames of the series failed)" if len(bad) > 1 else ""))
    return np.stack(px)
