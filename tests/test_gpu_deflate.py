"""The device deflate encoder (csrc/deflate.hip, `boa_deflate_members`) against zlib and gzip: every member must inflate on its
own to its slice of the payload, the CRC-32s must be zlib's, the sizes must stay within bounds derived from the format, and
`nifti.save(..., ctx=ctx)` / `compute_all_models` under BOA_SAVE_DEVICE=1 must write files that decompress to the bytes of the
CPU path."""
import ctypes as C
import functools
import gzip
import json
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 3, 257, 258, 259, 16383, 16384, 16385)
ROWS = (0, 7, 192, 32768, 32769)
IMG_W = 300


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.compute.inference import get_context
    return get_context("gpu")


def _prefix_image():
    """Rows of IMG_W random bytes; row k + 1 repeats the first L = 3 .. 258 bytes of row k and differs at byte L (then two rows that
    repeat it whole): a match of every length at distance IMG_W."""
    rng = np.random.default_rng(11)
    rows = [rng.integers(0, 256, IMG_W, dtype=np.uint8)]
    for L in range(3, 259):
        r = rng.integers(0, 256, IMG_W, dtype=np.uint8)
        r[:L] = rows[-1][:L]
        r[L] = rows[-1][L] ^ 0x55
        r[-1] = rows[-1][-1] ^ 0xAA          # (no match may begin in the row before)
        rows.append(r)
    rows += [rows[-1].copy(), rows[-1].copy()]
    return np.concatenate(rows)


def _cycle(a, n):
    return np.resize(a, n) if n else np.zeros(0, np.uint8)


def _regions_like(n):
    """Runs of 255 (body_regions' "ignore" value) and of small labels, with single bytes >= 144 between them."""
    rng = np.random.default_rng(5)
    vals = rng.choice(np.array([0, 1, 2, 11, 143, 144, 200, 255, 255, 255], np.uint8), n // 8 + 2)
    lens = rng.choice(np.array([1, 1, 2, 3, 4, 17, 60, 300]), n // 8 + 2)
    return np.repeat(vals, lens)[:n]


CONTENTS = {
    "zeros": lambda n: np.zeros(n, np.uint8),
    "all255": lambda n: np.full(n, 255, np.uint8),
    "alternating": lambda n: (np.arange(n) & 1).astype(np.uint8),
    "random": lambda n: np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8),
    "random0to3": lambda n: np.random.default_rng(2).integers(0, 4, n, dtype=np.uint8),
    "prefix_image": lambda n: _cycle(_prefix_image(), n),
    "regions_like": _regions_like,
}


def _deflate(ctx, payload, member_bytes, row_bytes, shift=0):
    """[(body, crc32, size)] per member through the Python binding; `shift`: bytes of padding in front (an unaligned source)."""
    from boa_hip import nifti
    buf = ctx.from_numpy(np.concatenate([np.zeros(shift, np.uint8), payload]))
    try:
        return nifti.device_deflate(ctx, buf.ptr + shift, len(payload), row_bytes, member_bytes)
    finally:
        buf.free()


def _check(members, payload, member_bytes):
    from boa_hip import nifti
    raw = payload.tobytes()
    assert len(members) == max(1, -(-len(raw) // member_bytes))
    for m, (body, crc, size) in enumerate(members):
        piece = raw[m * member_bytes:m * member_bytes + size]
        assert size == len(piece)
        d = zlib.decompressobj(-15)              # raw deflate with an empty window: a distance before the member's start fails
        got = d.decompress(bytes(body)) + d.flush()
        assert d.eof and d.unused_data == b"", f"member {m}: stream not finished at its end"
        assert got == piece, f"member {m} of {len(members)}"
        assert crc == zlib.crc32(piece), f"member {m}: CRC-32"
    assert gzip.decompress(b"".join(nifti.gzip_member(*t) for t in members)) == raw      # CRC-32 and ISIZE of every member


def _body_size(members):
    return sum(len(b) for b, _, _ in members)


@pytest.mark.parametrize("content", sorted(CONTENTS))
def test_round_trip_single_member(ctx, content):
    for n in SIZES:
        payload = CONTENTS[content](n)
        for row in ROWS + ((2,) if content == "alternating" else ()):
            _check(_deflate(ctx, payload, 4 << 20, row), payload, 4 << 20)
    if content == "zeros":
        assert bytes(_deflate(ctx, CONTENTS[content](0), 4 << 20, 0)[0][0]) == b"\x03\x00"     # the empty final fixed block


@pytest.mark.parametrize("content", sorted(CONTENTS))
def test_round_trip_ragged_members(ctx, content):
    """member_bytes = 40 000, n = 3 x 40 000 + 1: three members of two full blocks and a ragged one, and a member of one byte.
    Also an odd member size and a source that is not 16-byte aligned (the byte-wise load)."""
    n = 3 * 40_000 + 1
    payload = CONTENTS[content](n)
    for row in ROWS + ((2,) if content == "alternating" else ()):
        members = _deflate(ctx, payload, 40_000, row)
        _check(members, payload, 40_000)
        if row == 32769:
            assert [bytes(b) for b, _, _ in members] == [bytes(b) for b, _, _ in _deflate(ctx, payload, 40_000, 0)]
    _check(_deflate(ctx, payload, 40_001, 192), payload, 40_001)
    _check(_deflate(ctx, payload, 40_000, 7, shift=3), payload, 40_000)


def _fixed_block_symbols(body):
    """Length symbols and distances of a raw deflate stream of fixed-Huffman and stored blocks (RFC 1951 3.2.4 - 3.2.6)."""
    big, pos = int.from_bytes(body, "little"), 0
    lbase = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    lext = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    dbase = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
    dext = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]

    def take(k):
        nonlocal pos
        v = (big >> pos) & ((1 << k) - 1)
        pos += k
        return v

    def code(k, have=0, v=0):            # Huffman codes arrive most significant bit first
        for _ in range(k - have):
            v = (v << 1) | take(1)
        return v

    syms, lengths, dists, final = set(), [], set(), 0
    while not final:
        final, btype = take(1), take(2)
        if btype == 0:
            pos = (pos + 7) & ~7
            ln = take(16)
            assert take(16) == ln ^ 0xFFFF
            pos += 8 * ln
            continue
        assert btype == 1
        while True:
            c = code(7)
            if c <= 23:
                sym = 256 + c
            else:
                c = code(8, 7, c)
                if 0x30 <= c <= 0xBF:
                    continue                                  # literal 0 .. 143
                if 0xC0 <= c <= 0xC7:
                    sym = 280 + c - 0xC0
                else:
                    assert 0x190 <= code(9, 8, c) <= 0x1FF      # literal 144 .. 255
                    continue
            if sym == 256:
                break
            syms.add(sym)
            lengths.append(lbase[sym - 257] + take(lext[sym - 257]))
            dc = code(5)
            dists.add(dbase[dc] + take(dext[dc]))
    assert (pos + 7) // 8 == len(body)
    return syms, lengths, dists


def test_every_length_code_and_full_matches(ctx):
    """The prefix image at its own row distance: all 29 length codes 257 .. 285 with their extra bits, nothing but the two distances;
    and a run of zeros is a chain of full 258-byte matches."""
    img = _prefix_image()
    members = _deflate(ctx, img, 4 << 20, IMG_W)
    _check(members, img, 4 << 20)
    syms, lengths, dists = _fixed_block_symbols(bytes(members[0][0]))
    assert syms == set(range(257, 286))
    # every prefix length occurs as a match length, except where a 16 KiB block edge cuts the prefix in two
    whole = {L for L in range(3, 259) if ((L - 2) * IMG_W) // 16384 == ((L - 2) * IMG_W + L - 1) // 16384}
    assert len(whole) >= 250 and whole <= set(lengths)
    assert dists <= {1, IMG_W} and IMG_W in dists
    zeros = np.zeros(3 * 16384, np.uint8)
    members = _deflate(ctx, zeros, 4 << 20, 192)
    syms, lengths, dists = _fixed_block_symbols(bytes(members[0][0]))
    # the member's first block has one literal in front; the others start with a match into the block before
    assert lengths.count(258) == 3 * (16384 // 258) and dists == {1}


def test_deterministic(ctx):
    from boa_hip import synthetic
    payload = np.asfortranarray(synthetic.label_phantom_regions((96, 80, 64))).reshape(-1, order="F")
    a = _deflate(ctx, payload, 100_000, 96)
    b = _deflate(ctx, payload, 100_000, 96)
    assert [(bytes(x), c, s) for x, c, s in a] == [(bytes(x), c, s) for x, c, s in b]
    _check(a, payload, 100_000)


def test_size_zeros_and_random(ctx):
    n = 1 << 20
    z = _deflate(ctx, np.zeros(n, np.uint8), 4 << 20, 0)
    print("zeros:", n, "->", _body_size(z))
    # 13 bits per 258 bytes + 4 bytes of alignment per 16 KiB block: n / 149
    assert _body_size(z) <= n // 100
    for mb in (4 << 20, 300_000):
        r = _deflate(ctx, CONTENTS["random"](n), mb, 192)
        print("random:", n, "members of", mb, "->", _body_size(r))
        assert _body_size(r) <= 1.01 * n + 64 * len(r)        # needs the stored-block fallback


@functools.lru_cache(maxsize=None)
def _phantom(name, shape=(192, 160, 128)):
    from boa_hip import synthetic
    vol = getattr(synthetic, f"label_phantom_{name}")(shape)
    vol.setflags(write=False)
    return vol


@pytest.mark.parametrize("name", ["total", "regions", "parts"])
def test_size_label_phantoms_against_zlib_level_1(ctx, name):
    """<= 1.25 x zlib level 1 (what the CPU path writes); a greedy parse with full 258-byte matches reaches 0.92 - 1.11 on a CPU
    model, matches cut at 128 or 256 byte pieces give 1.14 - 1.63."""
    payload = np.asfortranarray(_phantom(name)).reshape(-1, order="F")
    members = _deflate(ctx, payload, 4 << 20, 192)
    _check(members, payload, 4 << 20)
    ours, ref = _body_size(members), len(zlib.compress(payload.tobytes(), 1))
    print(f"{name}: device {ours} B, zlib level 1 {ref} B, ratio {ours / ref:.3f}")
    assert ours <= 1.25 * ref


def test_capacity_is_checked_before_anything_is_written(ctx):
    from boa_hip import _lib
    n, mb, guard = 100_000, 40_000, 4096
    payload = CONTENTS["random"](n)
    bound = int(ctx.lib.boa_deflate_bound(n, mb))
    assert bound == n + 5 * (3 + 3 + 2)                         # 8 blocks, every one stored
    assert int(ctx.lib.boa_deflate_bound(0, mb)) == 5 and int(ctx.lib.boa_deflate_bound(n, 0)) == 0
    src = ctx.from_numpy(payload)
    out = ctx.from_numpy(np.full(bound + guard, 0xA5, np.uint8))
    offs, crcs = (C.c_size_t * 4)(), (C.c_uint32 * 3)()
    try:
        rc = ctx.lib.boa_deflate_members(ctx.h, src.vp, n, mb, 0, out.vp, bound - 1, offs, crcs)
        assert rc == _lib.BOA_EINVAL
        msg = ctx.lib.boa_last_error().decode()
        assert "out_capacity" in msg and str(bound) in msg
        assert (out.download((bound + guard,), np.uint8) == 0xA5).all()
        # exactly the bound: random data fills it to the last byte and leaves the guard alone
        _lib.check(ctx.lib.boa_deflate_members(ctx.h, src.vp, n, mb, 0, out.vp, bound, offs, crcs), "boa_deflate_members")
        got = out.download((bound + guard,), np.uint8)
        assert list(offs) == [0, 40_000 + 15, 80_000 + 30, bound]
        assert (got[bound:] == 0xA5).all()
        for m in range(3):
            piece = payload[m * mb:(m + 1) * mb].tobytes()
            assert zlib.decompress(got[offs[m]:offs[m + 1]].tobytes(), -15) == piece and crcs[m] == zlib.crc32(piece)
        for bad in (dict(mb=0), dict(mb=(1 << 30) + 1)):
            assert ctx.lib.boa_deflate_members(ctx.h, src.vp, n, bad["mb"], 0, out.vp, bound, offs, crcs) == _lib.BOA_EINVAL
    finally:
        src.free()
        out.free()


@pytest.mark.parametrize("source", ["devarray_file_order", "devarray_other_order", "numpy"])
def test_nifti_save_with_ctx(ctx, tmp_path, source):
    """The device-written file against the CPU-written one: same decompressed bytes; `nifti.load` (the parallel "BO" path: the header
    member, then two data members) gives the same array, affine and extension."""
    from boa_hip import nifti
    from boa_hip.devarray import DevArray
    vol = _phantom("regions", (200, 168, 130))                  # 4.37 MB: a full member and a ragged one
    aff = np.diag([-1.5, -1.5, 5.0, 1.0])
    aff[:3, 3] = [10.0, -20.0, 30.0]
    ext = [(0, nifti.label_xml({1: "subcutaneous", 255: "ignore"}))]
    cpu, dev = tmp_path / "cpu.nii.gz", tmp_path / "dev.nii.gz"
    nifti.save(cpu, vol, aff, extensions=ext)
    if source == "numpy":
        nifti.save(dev, vol, aff, extensions=ext, ctx=ctx)
    else:
        if source == "devarray_file_order":
            d = DevArray.from_numpy(ctx, np.ascontiguousarray(vol.transpose(2, 1, 0))).transpose((2, 1, 0))   # x fastest: file order
            assert d.strides == (1, 200, 200 * 168)
        else:
            d = DevArray.from_numpy(ctx, vol)
        assert d.shape == vol.shape
        nifti.save(dev, d, aff, extensions=ext, ctx=ctx)
        np.testing.assert_array_equal(d.download(), vol)          # the source is left as it was
        d.free()
    raw = dev.read_bytes()
    assert gzip.decompress(raw) == gzip.decompress(cpu.read_bytes())
    tab = nifti._member_table(raw)
    assert tab is not None and [t[2] for t in tab][1:] == [4 << 20, vol.size - (4 << 20)]
    got, gaff, hdr = nifti.load(dev, threads=4)
    want, waff, whdr = nifti.load(cpu)
    np.testing.assert_array_equal(got, vol)
    assert got.dtype == np.uint8 and np.array_equal(gaff, waff) and hdr.extensions == whdr.extensions and hdr.raw == whdr.raw
    assert nifti.parse_label_xml(hdr.extensions[0][1]) == {1: "subcutaneous", 255: "ignore"}


def _write_models(root, sp_zyx_total, sp_zyx_bca):
    """The synthetic model folders of the drop-in test: five `total` part models and the two BCA networks."""
    from boa_hip import label_maps, model_store, plans
    for tid, nc in zip(label_maps.PART_TASK_IDS, (25, 27, 19, 24, 27)):
        pj, dj = plans.synthetic_plans(patch=(32, 32, 32), features=(32, 64), num_classes=nc, spacing=sp_zyx_total)
        geom = plans.model_config_from_plans(pj, dj).geometry
        model_store.write_model_folder(root, tid, f"TotalSegmentator_part{tid - 290}", "nnUNetTrainerNoMirroring", pj, dj,
                                       [plans.synthetic_state_dict(geom, seed=tid)])
    for tid, nc, name, trainer in ((543, 7, "BCA_body_parts", "nnUNetTrainer_1500epochs_NoMirroring"),
                                   (542, 12, "BCA_inference", "nnUNetTrainerNoMirroring")):
        pj, dj = plans.synthetic_plans(patch=(32, 32, 32), features=(32, 64), num_classes=nc, spacing=sp_zyx_bca)
        geom = plans.model_config_from_plans(pj, dj).geometry
        model_store.write_model_folder(root, tid, name, trainer, pj, dj,
                                       [plans.synthetic_state_dict(geom, seed=tid + f) for f in range(5)])


def test_drop_in_outputs_do_not_depend_on_the_switch(tmp_path, monkeypatch):
    """compute_all_models(["total", "bca"]) with and without BOA_SAVE_DEVICE=1: every .nii.gz decompresses to the same bytes, the
    JSON files are equal, and the five uint8 label volumes (not the int16 CT) took the device encoder exactly when asked to."""
    from boa_hip import nifti
    from boa_hip.compute.inference import compute_all_models
    from boa_hip.synthetic import ct_phantom
    root = tmp_path / "results"
    _write_models(str(root), (1.5, 1.5, 1.5), (5.0, 1.5, 1.5))
    monkeypatch.setenv("nnUNet_results", str(root))
    ct = ct_phantom((48, 40, 56), seed=5)
    aff = np.diag([-1.5, -1.5, 1.5, 1.0])
    aff[:3, 3] = [30.0, 40.0, -100.0]
    ct_path = tmp_path / "ct.nii.gz"
    nifti.save(ct_path, ct, aff)
    params = {"preview": False, "fast": False, "ml": True, "nr_thr_resamp": 1, "nr_thr_saving": 1, "quiet": True,
              "verbose": False, "device": "gpu", "license_number": None}
    bca_params = {"median_filtering": False, "examined_body_region": None, "save_pdf": False, "theme": "light"}
    calls = []
    real = nifti.device_deflate
    monkeypatch.setattr(nifti, "device_deflate", lambda *a, **k: (calls.append(a[2]), real(*a, **k))[1])
    counts = {}
    for switch in ("off", "on"):
        if switch == "on":
            monkeypatch.setenv("BOA_SAVE_DEVICE", "1")
        else:
            monkeypatch.delenv("BOA_SAVE_DEVICE", raising=False)
        del calls[:]
        compute_all_models(ct_path, tmp_path / switch, ["total", "bca"], params, fast_bca=True, bca_params=bca_params)
        counts[switch] = list(calls)
    assert counts["off"] == [] and counts["on"] == [48 * 40 * 56] * 5
    names = sorted(p.name for p in (tmp_path / "off").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "on").iterdir())
    assert {"total.nii.gz", "ct_pfav.nii.gz", "body_parts.nii.gz", "body_regions.nii.gz", "tissues.nii.gz",
            "total-measurements.json", "bca-measurements.json"} <= set(names)
    for name in names:
        a, b = (tmp_path / "off" / name).read_bytes(), (tmp_path / "on" / name).read_bytes()
        if name.endswith(".nii.gz"):
            assert gzip.decompress(a) == gzip.decompress(b), name
            assert nifti._member_table(b) is not None, name
        elif name.endswith(".json"):
            assert json.loads(a) == json.loads(b), name
