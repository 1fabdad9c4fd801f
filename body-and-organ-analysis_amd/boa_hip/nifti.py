"""Minimal NIfTI-1 single-file (.nii / .nii.gz) reader and writer for the folder contract of the path (SURVEY 8b
"File contract"; 8f rank 3).  Implements the published NIfTI-1.1 header layout (348-byte header, 4-byte extender,
extensions, data at vox_offset) -- enough for what the reference does with nibabel on this path:
  * `nib.load(p).get_fdata()` / `.affine` / `.header.get_zooms()`: data scaled by scl_slope/scl_inter, best affine =
    sform (sform_code > 0) else qform (qform_code > 0) else pixdim-only;
  * `new_header = img_in_orig.header.copy(); new_header.set_data_dtype(np.uint8)` + label-table XML extension
    (ecode 0) + `nib.save` (TS/nnunet.py:723-726; TS/nifti_ext_header.py:12-42).
nibabel itself is absent in this image; files written here were round-tripped through this reader only (PARITY
UNPINNED vs nibabel's byte-level output; the header fields follow the standard)."""
from __future__ import annotations

import gzip
import os
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

_DT = {2: np.uint8, 4: np.int16, 8: np.int32, 16: np.float32, 64: np.float64, 256: np.int8, 512: np.uint16,
       768: np.uint32, 1024: np.int64, 1280: np.uint64}
_DT_INV = {np.dtype(v): k for k, v in _DT.items()}
_HDR = "<i10s18sihcB8h3f4h8f3fhBB4f2i80s24s2h3f3f12f16s4s"   # little-endian layout, 348 bytes
assert struct.calcsize(_HDR) == 348


@dataclass
class NiftiHeader:
    raw: bytes                                   # the 348 header bytes as read (little-endian normalised)
    dim: Tuple[int, ...]
    datatype: int
    pixdim: Tuple[float, ...]
    vox_offset: float
    scl_slope: float
    scl_inter: float
    qform_code: int
    sform_code: int
    quatern: Tuple[float, float, float]
    qoffset: Tuple[float, float, float]
    srow: np.ndarray
    extensions: List[Tuple[int, bytes]] = field(default_factory=list)

    def get_zooms(self) -> Tuple[float, ...]:
        return tuple(np.float32(v) for v in self.pixdim[1:1 + self.dim[0]])

    def get_data_shape(self) -> Tuple[int, ...]:
        return tuple(self.dim[1:1 + self.dim[0]])

    def get_data_dtype(self):
        return np.dtype(_DT[self.datatype])


def _qform(h: NiftiHeader) -> np.ndarray:
    b, c, d = (float(v) for v in h.quatern)
    a2 = 1.0 - (b * b + c * c + d * d)
    a = np.sqrt(a2) if a2 > 0 else 0.0
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c]])
    qfac = -1.0 if h.pixdim[0] < 0 else 1.0
    zooms = np.array([h.pixdim[1], h.pixdim[2], h.pixdim[3] * qfac], dtype=np.float64)
    aff = np.eye(4)
    aff[:3, :3] = R * zooms
    aff[:3, 3] = h.qoffset
    return aff


def best_affine(h: NiftiHeader) -> np.ndarray:
    if h.sform_code > 0:
        aff = np.eye(4)
        aff[:3, :] = h.srow
        return aff
    if h.qform_code > 0:
        return _qform(h)
    # neither code set: nibabel's base affine (shape_zoom_affine with the Analyze / NIfTI default x_flip=True):
    # diag(-zx, zy, zz) with the volume centre at the world origin
    zooms = np.array([-h.pixdim[1], h.pixdim[2], h.pixdim[3]], dtype=np.float64)
    aff = np.diag([zooms[0], zooms[1], zooms[2], 1.0])
    shape = np.array(h.dim[1:4], dtype=np.float64)
    aff[:3, 3] = -(shape - 1) / 2.0 * zooms
    return aff


def _open(path, mode):
    return gzip.open(path, mode) if str(path).endswith(".gz") else open(path, mode)


def _member_table(raw) -> Optional[list]:
    """[(deflate start, deflate end, uncompressed size)] of a gzip file whose EVERY member carries this module's FEXTRA index
    subfield (written by write_gzip_members), else None.  Walking the members costs a few header reads, no inflation."""
    mv = memoryview(raw)
    out, off, n = [], 0, len(mv)
    while off < n:
        if n - off < 28 or mv[off] != 0x1F or mv[off + 1] != 0x8B or mv[off + 2] != 8 or mv[off + 3] != 4:
            return None
        xlen = mv[off + 10] | (mv[off + 11] << 8)
        if xlen != 8 or bytes(mv[off + 12:off + 16]) != b"BO\x04\x00":
            return None
        total = struct.unpack("<I", mv[off + 16:off + 20])[0]
        if total < 28 or off + total > n:
            return None
        out.append((off + 20, off + total - 8, struct.unpack("<I", mv[off + total - 4:off + total])[0]))
        off += total
    return out or None


READ_THREADS = int(os.environ.get("BOA_READ_THREADS", "0")) or min(8, os.cpu_count() or 1)


LOAD_DEVICE_ENV = "BOA_LOAD_DEVICE"


def load_context(ctx):
    """`ctx` for the readers of the file-level callers (compute_all_models, compute_measurements, the BCA file readers): the
    context with $BOA_LOAD_DEVICE = 1, which sends their .nii.gz inputs through the device inflate, else None (default off:
    DESIGN 4.10)."""
    return ctx if os.environ.get(LOAD_DEVICE_ENV) == "1" else None


def gzip_header_end(raw, off: int = 0) -> Optional[int]:
    """The offset of the deflate body of the gzip member that starts at `off` (RFC 1952 section 2.3: the fixed ten bytes, then
    FEXTRA, FNAME, FCOMMENT and FHCRC as FLG says; FTEXT changes nothing), or None where that is no complete deflate member header
    (bad magic, a method other than 8, a reserved flag bit, a field that runs past the end, an FHCRC that does not match)."""
    import zlib
    mv = memoryview(raw)
    n = len(mv)
    if n - off < 10 or mv[off] != 0x1F or mv[off + 1] != 0x8B or mv[off + 2] != 8:
        return None
    flg = mv[off + 3]
    if flg & 0xE0:
        return None
    at = off + 10
    if flg & 4:
        if at + 2 > n:
            return None
        at += 2 + (mv[at] | (mv[at + 1] << 8))
        if at > n:
            return None
    for bit in (8, 16):
        if flg & bit:
            while at < n and mv[at] != 0:
                at += 1
            if at >= n:
                return None
            at += 1
    if flg & 2:
        if at + 2 > n or (zlib.crc32(mv[off:at]) & 0xFFFF) != (mv[at] | (mv[at + 1] << 8)):
            return None
        at += 2
    return at


def _gzip_streams(raw) -> Optional[list]:
    """[(deflate start, deflate end, payload size, CRC-32)] for the device inflate: the members of this module's index, or the one
    member of a foreign file (whether it is the only one shows when its final block ends: a second member is trailing data to the
    decoder).  ISIZE is the size modulo 2^32; it is taken as the size, and a stream that counts differently goes to the host."""
    mv = memoryview(raw)
    tab = _member_table(raw)
    if tab:
        return [(lo, hi, size, struct.unpack("<I", mv[hi:hi + 4])[0]) for lo, hi, size in tab]
    body = gzip_header_end(raw)
    if body is None or len(mv) - body < 8 + 1:
        return None
    crc, isize = struct.unpack("<II", mv[len(mv) - 8:])
    return [(body, len(mv) - 8, isize, crc)]


def device_inflate(ctx, raw, *, chunk_bytes: Optional[int] = None):
    """The payload of the gzip file `raw` (bytes-like) inflated on the device with `boa_inflate_streams` (csrc/inflate.hip):
    -> (uint8 array, info).  Only the file's bytes go up and the payload comes down.  info: "chunks", "candidates" (block starts
    the find pass accepted), "rejected" (those the chain check dropped), "rounds" (repair rounds), "live", "streams", "status"
    (one name per stream, "ok" = decoded and equal to the trailer's CRC-32 and size), "ms" (device-event times of find, count,
    store, windows, resolve) and "host": True where the device did not decode the file -- a container this path does not take
    (status []), or a status other than ok -- in which case the array is None and the caller inflates on the host.
    `chunk_bytes`: compressed bytes per chunk (default boa_inflate_default_chunk(), 64 KiB)."""
    import ctypes as C
    from . import _lib
    info = {"chunks": 0, "candidates": 0, "rejected": 0, "rounds": 0, "live": 0, "streams": 0, "status": [], "ms": {}, "host": True}
    streams = _gzip_streams(raw)
    if not streams:
        return None, info
    n = len(streams)
    total = sum(s[2] for s in streams)
    u64 = C.c_uint64 * n
    offs, lens, sizes = u64(*[s[0] for s in streams]), u64(*[s[1] - s[0] for s in streams]), u64(*[s[2] for s in streams])
    crcs = (C.c_uint32 * n)(*[s[3] for s in streams])
    status, words, ms = (C.c_int * n)(), (C.c_uint64 * _lib.BOA_INF_INFO_WORDS)(), (C.c_float * _lib.BOA_INF_MS_WORDS)()
    chunk_bytes = int(chunk_bytes) if chunk_bytes else int(ctx.lib.boa_inflate_default_chunk())
    src = ctx.from_numpy(np.frombuffer(raw, dtype=np.uint8))
    out = ctx.alloc(max(total, 16))
    try:
        _lib.check(ctx.lib.boa_inflate_streams(ctx.h, src.vp, len(raw), n, offs, lens, sizes, crcs, chunk_bytes, out.vp, total, status,
                                               words, ms), "boa_inflate_streams")
        info.update(chunks=int(words[0]), candidates=int(words[1]), rejected=int(words[2]), rounds=int(words[3]), live=int(words[4]),
                    streams=n, status=[_lib.BOA_INF_STATUS[s] for s in status],
                    ms=dict(zip(("find", "count", "store", "windows", "resolve"), (float(v) for v in ms))))
        if any(status):
            return None, info
        info["host"] = False
        return (out.download((total,), np.uint8) if total else np.zeros(0, np.uint8)), info
    finally:
        src.free()
        out.free()


def read_bytes(path, threads: Optional[int] = None, ctx=None) -> bytes:
    """The decompressed content of `path`.  A .gz file written by this module (indexed members) is inflated on `threads` cores
    (zlib releases the GIL): a 512^3 label volume in 0.15 s instead of 0.6 s; any other gzip stream takes the ordinary
    sequential path (a deflate stream has no entry points -- files of other writers are parallelised across FILES, load_many).
    With `ctx` (a device Context) an indexed or a single-member .gz file is inflated on the device (device_inflate); whatever the
    device does not decode -- another container, a damaged stream -- takes the host path above and raises what it raises."""
    if not str(path).endswith(".gz"):
        with open(path, "rb") as f:
            return f.read()
    threads = READ_THREADS if threads is None else int(threads)
    with open(path, "rb") as f:
        raw = f.read()
    if ctx is not None:
        data, info = device_inflate(ctx, raw)
        if not info["host"]:
            return data
    tab = _member_table(raw) if threads > 1 else None
    if not tab or len(tab) == 1:
        return gzip.decompress(raw)
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    offs = np.concatenate([[0], np.cumsum([t[2] for t in tab])]).astype(np.int64)
    out = bytearray(int(offs[-1]))
    omv, rmv = memoryview(out), memoryview(raw)

    def inflate(i):
        lo, hi, size = tab[i]
        d = zlib.decompress(rmv[lo:hi], -15, size)
        if len(d) != size or (zlib.crc32(d) & 0xFFFFFFFF) != struct.unpack("<I", rmv[hi:hi + 4])[0]:
            raise ValueError(f"{path}: gzip member {i} is corrupt")
        omv[int(offs[i]):int(offs[i]) + size] = d

    with ThreadPoolExecutor(max_workers=min(threads, len(tab))) as ex:
        list(ex.map(inflate, range(len(tab))))
    return out


def load_many(paths, threads: Optional[int] = None) -> list:
    """[load(p) for p in paths] with the files read and inflated concurrently (the reference reads the CT and up to seven
    segmentation volumes per task one after the other, NN/imageio/nibabel_reader_writer.py:38-90, BOA/compute/measurements.py)."""
    from concurrent.futures import ThreadPoolExecutor
    paths = list(paths)
    threads = READ_THREADS if threads is None else int(threads)
    if threads <= 1 or len(paths) <= 1:
        return [load(p) for p in paths]
    inner = max(1, threads // len(paths))
    with ThreadPoolExecutor(max_workers=min(threads, len(paths))) as ex:
        return list(ex.map(lambda p: load(p, threads=inner), paths))


def load(path, threads: Optional[int] = None, ctx=None) -> Tuple[np.ndarray, np.ndarray, NiftiHeader]:
    """-> (raw data array in file axis order and dtype, affine (4,4) float64, header).  `get_fdata` = fdata(...).  `ctx`: see
    read_bytes."""
    blob = read_bytes(path, threads, ctx)
    if len(blob) < 352:
        raise ValueError(f"{path}: not a NIfTI-1 file")
    endian = "<"
    if struct.unpack("<i", blob[:4])[0] != 348:
        if struct.unpack(">i", blob[:4])[0] != 348:
            raise ValueError(f"{path}: sizeof_hdr != 348")
        endian = ">"
    v = struct.unpack(endian + _HDR[1:], blob[:348])
    magic = v[-1]
    if magic[:3] not in (b"n+1", b"ni1"):
        raise ValueError(f"{path}: bad magic {magic!r}")
    if magic[:3] == b"ni1":
        raise ValueError(f"{path}: two-file NIfTI (.hdr/.img) is not supported")
    dim = v[7:15]
    datatype = v[19]
    pixdim = v[22:30]
    vox_offset, scl_slope, scl_inter = v[30], v[31], v[32]
    qform_code, sform_code = v[44], v[45]
    quatern, qoffset = v[46:49], v[49:52]
    srow = np.array(v[52:64], dtype=np.float64).reshape(3, 4)
    if datatype not in _DT:
        raise TypeError(f"{path}: unsupported NIfTI datatype code {datatype}")
    raw_le = struct.pack(_HDR, *v)
    h = NiftiHeader(raw_le, tuple(int(d) for d in dim), int(datatype), tuple(float(p) for p in pixdim), float(vox_offset),
                    float(scl_slope), float(scl_inter), int(qform_code), int(sform_code), tuple(quatern), tuple(qoffset), srow)
    off = 352
    if blob[348] != 0:                       # extensions present
        while off + 8 <= int(vox_offset):
            esize, ecode = struct.unpack(endian + "ii", blob[off:off + 8])
            if esize < 8:
                break
            h.extensions.append((ecode, bytes(blob[off + 8:off + esize])))
            off += esize
    shape = h.get_data_shape()
    dt = np.dtype(_DT[datatype]).newbyteorder(endian)
    n = int(np.prod(shape))
    data = np.frombuffer(blob, dtype=dt, count=n, offset=int(vox_offset)).reshape(shape, order="F")
    return data.astype(dt.newbyteorder("=")), best_affine(h), h


def is_scaled(h: NiftiHeader) -> bool:
    """True when get_fdata() would apply scl_slope / scl_inter."""
    s, i = h.scl_slope, h.scl_inter
    return bool(np.isfinite(s) and s != 0 and not (s == 1.0 and (i == 0 or not np.isfinite(i))))


def fdata(data: np.ndarray, h: NiftiHeader) -> np.ndarray:
    """nibabel's get_fdata(): float64 with scl_slope / scl_inter applied when they are set."""
    out = data.astype(np.float64)
    s, i = h.scl_slope, h.scl_inter
    if np.isfinite(s) and s != 0 and not (s == 1.0 and (i == 0 or not np.isfinite(i))):
        out = out * s + (i if np.isfinite(i) else 0.0)
    return out


def label_xml(label_map: Dict[int, str]) -> bytes:
    """TS/nifti_ext_header.py:12-42 (the CaretExtension label table written into the extended header)."""
    colors = [[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255], [255, 128, 0],
              [255, 0, 128], [128, 255, 128], [0, 128, 255], [128, 128, 128], [185, 170, 155]]
    pre = ('<?xml version="1.0" encoding="UTF-8"?> <CaretExtension>  <Date><![CDATA[2013-07-14T05:45:09]]></Date>   '
           '<VolumeInformation Index="0">   <LabelTable>')
    body = ""
    for k, name in label_map.items():
        r, g, b = colors[k % len(colors)]
        body += f'<Label Key="{k}" Red="{r / 255}" Green="{g / 255}" Blue="{b / 255}" Alpha="1"><![CDATA[{name}]]></Label>\n'
    post = ('  </LabelTable>  <StudyMetaDataLinkSet>  </StudyMetaDataLinkSet>  <VolumeType><![CDATA[Label]]></VolumeType>   '
            '</VolumeInformation></CaretExtension>')
    return bytes(pre + "\n" + body + "\n" + post + "\n              ", "utf-8")


def parse_label_xml(content: bytes) -> Dict[int, str]:
    import re
    return {int(k): v for k, v in re.findall(r'<Label Key="(\d+)"[^>]*><!\[CDATA\[(.*?)\]\]></Label>',
                                             content.decode("utf-8", "replace"))}


SAVE_THREADS = int(os.environ.get("BOA_SAVE_THREADS", "0")) or min(8, os.cpu_count() or 1)   # nr_thr_saving of the reference
_GZ_BLOCK = 4 << 20


def gzip_member(body, crc32: int, size: int) -> bytes:
    """One gzip member (RFC 1952) around a raw deflate stream `body` of `size` payload bytes with CRC-32 `crc32`: the container
    of write_gzip_members, whichever encoder made the body (zlib there, the device encoder in device_deflate)."""
    total = 20 + len(body) + 8
    head = b"\x1f\x8b\x08\x04" + b"\x00\x00\x00\x00" + b"\x00\xff" + b"\x08\x00" + b"BO\x04\x00" + struct.pack("<I", total)
    return head + bytes(body) + struct.pack("<II", crc32 & 0xFFFFFFFF, size & 0xFFFFFFFF)


def write_wrapped_members(f, members):
    """Write (body, crc32, size) triples as consecutive gzip members."""
    for body, crc, size in members:
        f.write(gzip_member(body, crc, size))


def device_deflate(ctx, src, n: int, row_bytes: int = 0, member_bytes: int = 0, *, near_bytes: int = 1, dynamic: bool = False):
    """Deflate `n` payload bytes that are on the device (`src`: a c_void_p / address, bytes in file order) with
    `boa_deflate_members2` (csrc/deflate.hip): -> [(body, crc32, size)] per member of `member_bytes` (default: the 4 MiB of
    write_gzip_members).  Only the compressed bytes and the offset / CRC tables are downloaded.  `near_bytes` (1 .. 16): the short
    candidate distance, the item size of the voxels (other than 1 only with `dynamic`); `dynamic`: blocks may carry their own Huffman codes (smaller, and what makes
    an int16 CT compress at all); the defaults give the fixed-code streams of `boa_deflate_members`."""
    import ctypes as C
    from . import _lib
    member_bytes = int(member_bytes) or _GZ_BLOCK
    n = int(n)
    cap = int(ctx.lib.boa_deflate_bound(n, member_bytes))
    if cap == 0:
        raise ValueError(f"device_deflate: {n} bytes in members of {member_bytes}")
    n_mem = max(1, -(-n // member_bytes))
    offs, crcs = (C.c_size_t * (n_mem + 1))(), (C.c_uint32 * n_mem)()
    out = ctx.alloc(cap)
    try:
        src = src if isinstance(src, C.c_void_p) else C.c_void_p(src)
        flags = _lib.BOA_DEFLATE_DYNAMIC if dynamic else 0
        _lib.check(ctx.lib.boa_deflate_members2(ctx.h, src, n, member_bytes, int(row_bytes), int(near_bytes), flags, out.vp, cap, offs, crcs),
                   "boa_deflate_members2")
        comp = memoryview(out.download((int(offs[n_mem]),), np.uint8)) if offs[n_mem] else memoryview(b"")
    finally:
        out.free()
    return [(comp[offs[m]:offs[m + 1]], int(crcs[m]), min(member_bytes, n - m * member_bytes)) for m in range(n_mem)]


def _device_body(ctx, data):
    """(buffer to free or None, address, bytes, row bytes) of `data` in file order on the device: a DevArray whose view is already
    in file order (x fastest) is used in place, any other one is reordered there; a numpy array is uploaded."""
    from .devarray import DevArray
    if isinstance(data, DevArray):
        x, y, _ = data.shape
        if data.strides == (1, x, x * y):
            return None, data.buf.ptr + data.offset * data.dtype.itemsize, data.size * data.dtype.itemsize, x * data.dtype.itemsize
        v = data.transpose((2, 1, 0)).contiguous(force_copy=True)
        return v.buf, v.buf.ptr, v.size * v.dtype.itemsize, x * data.dtype.itemsize
    body = np.asfortranarray(data).reshape(-1, order="F")
    row = (data.shape[0] if data.ndim else 1) * data.dtype.itemsize
    if body.nbytes == 0:
        return None, None, 0, row
    buf = ctx.from_numpy(body)
    return buf, buf.ptr, body.nbytes, row


SAVE_DEVICE_ENV = "BOA_SAVE_DEVICE"


def save_volume(path, data, affine, ctx=None, **kw):
    """`save` for the file-level callers (compute_all_models, the ct_pfav writer, get_image_info): with $BOA_SAVE_DEVICE = 1 the
    uint8 volumes of a `.gz` path go through the device encoder with its fixed codes, with $BOA_SAVE_DEVICE = 2 the uint8 and the
    int16 volumes with dynamic codes (default off: DESIGN 4.9); everything else, and everything without the switch, takes the CPU
    path (a DevArray is downloaded first)."""
    from .devarray import DevArray
    mode = os.environ.get(SAVE_DEVICE_ENV)
    dtypes = {"1": (np.uint8,), "2": (np.uint8, np.int16)}.get(mode, ())
    if ctx is not None and np.dtype(data.dtype) in dtypes and str(path).endswith(".gz"):
        return save(path, data, affine, ctx=ctx, dynamic=mode == "2", **kw)
    return save(path, data.download() if isinstance(data, DevArray) else data, affine, **kw)


def write_gzip_members(f, payload, compresslevel: int = 1, threads: int = 1, block: int = _GZ_BLOCK):
    """`payload` (bytes-like) as a gzip stream of independently compressed members (RFC 1952 section 2.2: a gzip file is a
    series of members; gzip.open, zlib's gzread -- SimpleITK, nibabel -- and `gunzip` read them as one stream; each member
    carries its own length in a FEXTRA subfield so that read_bytes can inflate them in parallel too), the members
    deflated in parallel: zlib releases the GIL, so a 512^3 label volume (134 MB) compresses on `threads` cores instead of
    one (pigz's scheme without its shared dictionary; level 1 like nibabel's default, so the ratio loss is a fraction of a
    percent).  The reference saves its volumes from `nr_thr_saving` worker processes instead (TS/nnunet.py:705-724)."""
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    mv = memoryview(payload).cast("B")

    def member(lo):
        # raw deflate + a hand-made gzip wrapper whose FEXTRA field (RFC 1952 2.3.1.1, subfield id "BO") holds the member's total
        # length -- BGZF's idea: a reader that knows the field hops from member to member and inflates them in parallel
        # (read_bytes); every other gzip reader skips it
        piece = mv[lo:lo + block]
        c = zlib.compressobj(compresslevel, zlib.DEFLATED, -15)
        return gzip_member(c.compress(piece) + c.flush(), zlib.crc32(piece), len(piece))

    starts = list(range(0, len(mv), block)) or [0]
    if threads <= 1 or len(starts) == 1:
        for lo in starts:
            f.write(member(lo))
        return
    with ThreadPoolExecutor(max_workers=min(threads, len(starts))) as ex:
        for part in ex.map(member, starts):
            f.write(part)


def quatern_from_affine(affine: np.ndarray) -> Tuple[Tuple[float, float, float], Tuple[float, float, float], float]:
    """(quatern b c d, qoffset, qfac) of an affine whose 3 x 3 part is rotation x positive zooms (x an optional flip of the third
    axis): the NIfTI-1.1 standard's matrix -> quaternion recipe (`nifti_mat44_to_quatern`), the inverse of `_qform`."""
    A = np.asarray(affine, dtype=np.float64)
    R = A[:3, :3] / np.sqrt(np.sum(A[:3, :3] ** 2, axis=0))[None, :]
    qfac = 1.0
    if np.linalg.det(R) < 0:
        R = R.copy()
        R[:, 2] = -R[:, 2]
        qfac = -1.0
    r11, r12, r13, r21, r22, r23, r31, r32, r33 = R.reshape(-1)
    a = r11 + r22 + r33 + 1.0
    if a > 0.5:
        a = 0.5 * np.sqrt(a)
        b, c, d = 0.25 * (r32 - r23) / a, 0.25 * (r13 - r31) / a, 0.25 * (r21 - r12) / a
    else:
        xd, yd, zd = 1.0 + r11 - (r22 + r33), 1.0 + r22 - (r11 + r33), 1.0 + r33 - (r11 + r22)
        if xd > 1.0:
            b = 0.5 * np.sqrt(xd)
            c, d, a = 0.25 * (r12 + r21) / b, 0.25 * (r13 + r31) / b, 0.25 * (r32 - r23) / b
        elif yd > 1.0:
            c = 0.5 * np.sqrt(yd)
            b, d, a = 0.25 * (r12 + r21) / c, 0.25 * (r23 + r32) / c, 0.25 * (r13 - r31) / c
        else:
            d = 0.5 * np.sqrt(zd)
            b, c, a = 0.25 * (r13 + r31) / d, 0.25 * (r23 + r32) / d, 0.25 * (r21 - r12) / d
        if a < 0.0:
            b, c, d = -b, -c, -d
    return (float(b), float(c), float(d)), tuple(float(x) for x in A[:3, 3]), qfac


def _file_head(shape, dtype, affine, like, extensions, form_codes) -> bytes:
    """The bytes in front of the data body of `save`: the 348-byte header, the extender and the extensions."""
    dtype = np.dtype(dtype)
    ndim = len(shape)
    if dtype not in _DT_INV:
        raise TypeError(f"unsupported dtype {dtype}")
    affine = np.asarray(affine, dtype=np.float64)
    v = list(struct.unpack(_HDR, like.raw)) if like is not None else list(struct.unpack(_HDR, b"\0" * 348))
    v[0] = 348
    dim = [ndim] + list(shape) + [1] * (7 - ndim)
    v[7:15] = dim
    v[19] = _DT_INV[dtype]
    v[20] = dtype.itemsize * 8
    zooms = np.sqrt(np.sum(affine[:3, :3] ** 2, axis=0))
    if like is None:
        v[22:30] = [1.0, float(zooms[0]), float(zooms[1]), float(zooms[2]), 1.0, 1.0, 1.0, 1.0]
        v[35] = 2 | 8                          # xyzt_units: mm, sec
        v[44], v[45] = 0, 2                    # qform unknown, sform aligned (what nibabel writes for a bare affine)
    v[31], v[32] = float("nan"), float("nan")   # nibabel writes nan slope/inter for unscaled data
    v[52:64] = [float(x) for x in affine[:3, :].reshape(-1)]
    if like is not None and like.sform_code == 0:
        v[45] = 2
    if form_codes is not None:                 # (qform_code, sform_code) with the quaternion of `affine` (what ITK's NIfTI writer stores)
        quat, qoff, qfac = quatern_from_affine(affine)
        v[44], v[45] = int(form_codes[0]), int(form_codes[1])
        v[46:49] = list(quat)
        v[49:52] = list(qoff)
        v[22] = qfac
    exts = list(extensions or [])
    ext_blob = b""
    for ecode, content in exts:
        esize = 8 + len(content)
        pad = (-esize) % 16
        ext_blob += struct.pack("<ii", esize + pad, ecode) + content + b"\0" * pad
    v[30] = float(352 + len(ext_blob))
    v[-1] = b"n+1\0"
    hdr = struct.pack(_HDR, *v)
    return hdr + bytes([1 if exts else 0, 0, 0, 0]) + ext_blob


def save(path, data: np.ndarray, affine: np.ndarray, like: Optional[NiftiHeader] = None,
         extensions: Optional[List[Tuple[int, bytes]]] = None, compresslevel: int = 1, threads: Optional[int] = None,
         form_codes: Optional[Tuple[int, int]] = None, ctx=None, dynamic: bool = False):
    """Write `data` (file axis order); `.gz` paths are deflated on `threads` cores (default SAVE_THREADS).  With `ctx` (a device
    Context) the data body of a `.gz` path is deflated on the device instead (device_deflate; same member container, so read_bytes
    inflates it in parallel as well), from a numpy array after an upload or from a 3-D DevArray without a download; the header and
    the extensions stay on the CPU path.  `dynamic` (with `ctx`): dynamic Huffman codes, the near distance = the item size.  `like`: header to copy (pixdim units, descrip, q/s-form codes ... as
    `img_in_orig.header.copy()` keeps them); datatype/bitpix/dim/vox_offset and the affine fields are set from the
    arguments; scl_slope/inter are reset (label volumes are stored unscaled).  `form_codes`: also store the affine as a qform."""
    on_device = ctx is not None and str(path).endswith(".gz")
    if on_device:
        from .devarray import DevArray
    if not (on_device and isinstance(data, DevArray)):   # (a DevArray is taken as it is)
        data = np.asarray(data)
    head = _file_head(data.shape, data.dtype, affine, like, extensions, form_codes)
    if on_device:
        buf, addr, nbytes, row = _device_body(ctx, data)
        try:
            if dynamic:
                members = device_deflate(ctx, addr, nbytes, row, near_bytes=min(16, data.dtype.itemsize), dynamic=True)
            else:
                members = device_deflate(ctx, addr, nbytes, row)
        finally:
            if buf is not None:
                buf.free()
        with open(path, "wb") as f:
            write_gzip_members(f, head, compresslevel, 1)
            write_wrapped_members(f, members)
        return
    body = np.asfortranarray(data).reshape(-1, order="F")          # (a view when `data` is already F-ordered)
    with open(path, "wb") as f:
        if str(path).endswith(".gz"):
            write_gzip_members(f, head, compresslevel, 1)
            write_gzip_members(f, body, compresslevel, SAVE_THREADS if threads is None else int(threads))
        else:
            f.write(head)
            f.write(body.tobytes())


def label_member_presence(ctx, src, n: int, member_bytes: int = 0) -> np.ndarray:
    """bool [members][256]: label k occurs in member m of the `n` label bytes on the device at `src` (a c_void_p / address),
    from one pass of `boa_label_member_presence` (csrc/label_masks.hip).  Members as in device_deflate."""
    import ctypes as C
    from . import _lib
    member_bytes = int(member_bytes) or _GZ_BLOCK
    n = int(n)
    n_mem = max(1, -(-n // member_bytes))
    bits = np.zeros((n_mem, 8), dtype="<u4")
    src = src if isinstance(src, C.c_void_p) else C.c_void_p(src)
    _lib.check(ctx.lib.boa_label_member_presence(ctx.h, src, n, member_bytes, bits.ctypes.data_as(C.POINTER(C.c_uint32))),
               "boa_label_member_presence")
    return np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little").astype(bool)


def pair_capacity(ctx, n: int, member_bytes: int, pair_members) -> int:
    """The output bytes `boa_deflate_label_pairs` asks for: every listed member stored (5 bytes per 16 KiB block, at least one)."""
    total = 0
    for m in pair_members:
        length = max(0, min(member_bytes, n - int(m) * member_bytes))
        total += int(ctx.lib.boa_deflate_bound(length, max(length, 1)))
    return total


def device_deflate_label_pairs(ctx, src, n: int, pairs, row_bytes: int = 0, member_bytes: int = 0, *, dynamic: bool = False, info=None):
    """The members of binary masks of the `n` label bytes on the device at `src`, without the masks: `pairs` = [(label, member)]
    -> [(body, crc32, size)] of the payload (labels == label) over that member, what device_deflate gives for it on the mask
    (`boa_deflate_label_pairs`, csrc/deflate.hip).  `info` (a dict): seconds spent in "encode" and "download" are added to it."""
    import ctypes as C
    import time
    from . import _lib
    member_bytes = int(member_bytes) or _GZ_BLOCK
    n, pairs = int(n), list(pairs)
    n_mem = max(1, -(-n // member_bytes))
    if not pairs:
        return []
    if any(not (0 <= int(k) <= 255 and 0 <= int(m) < n_mem) for k, m in pairs):
        raise ValueError(f"device_deflate_label_pairs: a pair outside labels 0 .. 255 x members 0 .. {n_mem - 1}")
    lab = (C.c_uint8 * len(pairs))(*[int(k) for k, _ in pairs])
    mem = (C.c_uint32 * len(pairs))(*[int(m) for _, m in pairs])
    cap = pair_capacity(ctx, n, member_bytes, (m for _, m in pairs))
    offs, crcs = (C.c_size_t * (len(pairs) + 1))(), (C.c_uint32 * len(pairs))()
    out = ctx.alloc(max(cap, 1))
    try:
        src = src if isinstance(src, C.c_void_p) else C.c_void_p(src)
        t0 = time.perf_counter()
        _lib.check(ctx.lib.boa_deflate_label_pairs(ctx.h, src, n, member_bytes, int(row_bytes), _lib.BOA_DEFLATE_DYNAMIC if dynamic else 0,
                                                   lab, mem, len(pairs), out.vp, cap, offs, crcs), "boa_deflate_label_pairs")
        t1 = time.perf_counter()
        comp = memoryview(out.download((int(offs[len(pairs)]),), np.uint8)) if offs[len(pairs)] else memoryview(b"")
        t2 = time.perf_counter()
    finally:
        out.free()
    if info is not None:
        info["encode"] = info.get("encode", 0.0) + t1 - t0
        info["download"] = info.get("download", 0.0) + t2 - t1
    return [(comp[offs[p]:offs[p + 1]], int(crcs[p]), max(0, min(member_bytes, n - int(m) * member_bytes))) for p, (_, m) in enumerate(pairs)]


def save_label_masks(folder, labels, affine, names: Dict[int, str], ctx, like: Optional[NiftiHeader] = None, dynamic: bool = False,
                     group_bytes: int = 1 << 30, info=None):
    """`<folder>/<name>.nii.gz` for every (k, name) of `names`: the uint8 mask (labels == k), each file byte for byte what
    `save(path, mask, affine, like=like, ctx=ctx, dynamic=dynamic)` writes -- TotalSegmentator's one-file-per-structure output
    (TS/nnunet.py:782-802) -- without a mask ever being made: `labels` (a uint8 DevArray or numpy volume, file axis order) is put
    on the device as `_device_body` does, one pass finds the (label, member) pairs that hold a voxel (label_member_presence), only
    those are encoded (device_deflate_label_pairs, in groups of at most `group_bytes` of payload, which bounds the workspace), and
    every other pair is the all-zero member, encoded once per member length.  A structure without a voxel gets an all-zero file, as
    the reference writes.  `info` (a dict) receives "pairs", "present", "compressed_bytes" and the seconds of "presence", "encode",
    "download" and "write"."""
    import io
    import time
    from .devarray import DevArray
    if not isinstance(labels, DevArray):
        labels = np.asarray(labels)
    if np.dtype(labels.dtype) != np.uint8 or len(labels.shape) != 3:
        raise TypeError(f"save_label_masks: a 3-D uint8 label volume is required, got {labels.dtype} {tuple(labels.shape)}")
    names = {int(k): str(v) for k, v in names.items()}
    if any(not 0 <= k <= 255 for k in names):
        raise ValueError("save_label_masks: label ids must be 0 .. 255")
    group_bytes = int(group_bytes)
    if group_bytes < 1:
        raise ValueError(f"save_label_masks: group_bytes {group_bytes}")
    folder = os.fspath(folder)
    stats = info if info is not None else {}
    head_gz = io.BytesIO()
    write_gzip_members(head_gz, _file_head(tuple(labels.shape), np.uint8, affine, like, None, None), 1, 1)
    mb = _GZ_BLOCK
    buf, addr, n, row = _device_body(ctx, labels)
    try:
        n_mem = max(1, -(-n // mb))
        length = [max(0, min(mb, n - m * mb)) for m in range(n_mem)]
        t0 = time.perf_counter()
        present = label_member_presence(ctx, addr, n, mb)
        stats["presence"] = time.perf_counter() - t0
        todo = [(k, m) for k in names for m in range(n_mem) if present[m, k]]
        members = {}
        lo = 0
        while lo < len(todo):                                  # groups of whole pairs, at least one
            hi, total = lo + 1, length[todo[lo][1]]
            while hi < len(todo) and total + length[todo[hi][1]] <= group_bytes:
                total += length[todo[hi][1]]
                hi += 1
            for pair, (body, crc, size) in zip(todo[lo:hi], device_deflate_label_pairs(ctx, addr, n, todo[lo:hi], row, mb, dynamic=dynamic, info=stats)):
                members[pair] = (bytes(body), crc, size)
            lo = hi
        zero = {}                                              # the all-zero member of every member length that an absent pair has
        for size in sorted({length[m] for k in names for m in range(n_mem) if not present[m, k]}):
            z = ctx.zeros(max(size, 1))
            try:
                (body, crc, _), = device_deflate(ctx, z.ptr, size, row, max(size, 1), dynamic=dynamic)
                zero[size] = (bytes(body), crc, size)
            finally:
                z.free()
    finally:
        if buf is not None:
            buf.free()
    t0 = time.perf_counter()
    written = 0
    for k, name in names.items():
        with open(os.path.join(folder, f"{name}.nii.gz"), "wb") as f:
            f.write(head_gz.getbuffer())
            write_wrapped_members(f, (members.get((k, m)) or zero[length[m]] for m in range(n_mem)))
            written += f.tell()
    stats.update(write=time.perf_counter() - t0, pairs=len(names) * n_mem, present=len(todo), compressed_bytes=written)
