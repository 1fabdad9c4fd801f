"""The dynamic-Huffman mode of the device deflate encoder (`boa_deflate_members2`, BOA_DEFLATE_DYNAMIC) against zlib's inflate, the
bit-level reader and the CPU restatement of tests/deflate_model.py: every member inflates alone, the tokens are the model's greedy
parse, the codes cost exactly what an optimal code costs, the block form is the smallest of the three, and the layers above
(`nifti.save(dynamic=True)`, BOA_SAVE_DEVICE=2) write files that decompress to the bytes of the CPU path."""
import ctypes as C
import functools
import gzip
import zlib

import numpy as np
import pytest

import deflate_model as dm

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 3, 257, 258, 259, 16383, 16384, 16385)
ROWS = (0, 7, 192, 32768, 32769)
NEARS = (1, 2, 16)


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.compute.inference import get_context
    return get_context("gpu")


def _deflate(ctx, payload, member_bytes, row_bytes, near=1, dynamic=True, shift=0):
    """[(body, crc32, size)] per member through the Python binding; `shift`: bytes of padding in front (an unaligned source)."""
    from boa_hip import nifti
    payload = np.frombuffer(bytes(payload), np.uint8) if not isinstance(payload, np.ndarray) else payload.view(np.uint8).reshape(-1)
    buf = ctx.from_numpy(np.concatenate([np.zeros(shift, np.uint8), payload, np.zeros(1, np.uint8)]))
    try:
        return nifti.device_deflate(ctx, buf.ptr + shift, len(payload), row_bytes, member_bytes, near_bytes=near, dynamic=dynamic)
    finally:
        buf.free()


def _check(members, payload, member_bytes):
    from boa_hip import nifti
    raw = bytes(payload)
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


def _size(members):
    return sum(len(b) for b, _, _ in members)


def _blocks(members):
    """The blocks of every member, without the empty stored block that must follow each coded block that is not the last."""
    out = []
    for body, _, _ in members:
        blocks = iter(dm.parse_blocks(bytes(body)))
        for b in blocks:
            out.append(b)
            if b["type"] != 0 and not b["final"]:
                sync = next(blocks)
                assert sync["type"] == 0 and not sync["data"] and not sync["final"], "no byte alignment after a coded block"
    return out


def _f_order(vol):
    return np.asfortranarray(vol).reshape(-1, order="F").view(np.uint8)


@functools.lru_cache(maxsize=None)
def _phantom(name, shape):
    from boa_hip import synthetic
    vol = synthetic.ct_phantom(shape, seed=5) if name == "ct" else getattr(synthetic, f"label_phantom_{name}")(shape)
    vol.setflags(write=False)
    return vol


# ---------------------------------------------------------------------------------------------------------------- round trips
@pytest.mark.parametrize("content", sorted(dm.CONTENTS))
def test_round_trip_single_member(ctx, content):
    for n in SIZES:
        payload = dm.CONTENTS[content](n)
        for near in NEARS:
            for row in ROWS:
                _check(_deflate(ctx, payload, 4 << 20, row, near), payload.tobytes(), 4 << 20)


@pytest.mark.parametrize("content", sorted(dm.CONTENTS))
def test_round_trip_ragged_members(ctx, content):
    """member_bytes = 40 000, n = 3 x 40 000 + 1: members of two full blocks and a ragged one, and a member of one byte; an odd member
    size; a source that is not 16-byte aligned."""
    n = 3 * 40_000 + 1
    payload = dm.CONTENTS[content](n)
    for near in NEARS:
        for row in ROWS:
            _check(_deflate(ctx, payload, 40_000, row, near), payload.tobytes(), 40_000)
        _check(_deflate(ctx, payload, 40_001, 192, near), payload.tobytes(), 40_001)
        _check(_deflate(ctx, payload, 40_000, 7, near, shift=3), payload.tobytes(), 40_000)


def test_bad_arguments_are_refused_before_any_launch(ctx):
    from boa_hip import _lib
    n, mb, guard = 50_000, 40_000, 4096
    bound = int(ctx.lib.boa_deflate_bound(n, mb))
    src = ctx.from_numpy(dm.CONTENTS["regions_like"](n))
    out = ctx.from_numpy(np.full(bound + guard, 0xA5, np.uint8))
    offs, crcs = (C.c_size_t * 3)(), (C.c_uint32 * 2)()
    try:
        for near, flags, word in ((0, 1, "near_bytes"), (17, 1, "near_bytes"), (-1, 0, "near_bytes"), (2, 0, "near_bytes"), (1, 2, "flags"), (1, 3, "flags"), (2, -1, "flags")):
            assert ctx.lib.boa_deflate_members2(ctx.h, src.vp, n, mb, 192, near, flags, out.vp, bound, offs, crcs) == _lib.BOA_EINVAL
            assert word in ctx.lib.boa_last_error().decode()
        assert ctx.lib.boa_deflate_members2(ctx.h, src.vp, n, mb, 192, 2, 1, out.vp, bound - 1, offs, crcs) == _lib.BOA_EINVAL
        assert (out.download((bound + guard,), np.uint8) == 0xA5).all()
    finally:
        src.free()
        out.free()


# ---------------------------------------------------------------------------------------------------------------- the codes
def _distance_cost(d):
    used = [f for f in d if f]
    return (0, 0) if not used else dm.huffman_cost_and_depth(d)


def _check_dynamic_block(b, where):
    """One dynamic block against its own tokens.  -> the depth of the unlimited Huffman trees of its two alphabets."""
    ll, d, extra = dm.histograms(b["tokens"])
    assert max(b["ll_lens"]) <= 15 and max(b["d_lens"]) <= 15 and max(b["cl_lens"]) <= 7, where
    assert len(b["ll_lens"]) == b["hlit"] and len(b["d_lens"]) == b["hdist"]
    ll_lens = b["ll_lens"] + [0] * (286 - b["hlit"])
    d_lens = b["d_lens"] + [0] * (30 - b["hdist"])
    assert all(bool(f) == bool(ln) for f, ln in zip(ll, ll_lens)) and all(bool(f) == bool(ln) for f, ln in zip(d, d_lens)), where
    assert dm.kraft(ll_lens) == 1 << 15, where
    assert b["payload_bits"] == sum(f * ln for f, ln in zip(ll, ll_lens)) + sum(f * ln for f, ln in zip(d, d_lens)) + extra
    # trimmed to the last used symbol, and no more header bits than the rule costs for these lengths
    hlit, hdist, hclen, _, _, bits = dm.header_plan(ll_lens, d_lens)
    assert (b["hlit"], b["hdist"], b["hclen"]) == (hlit, hdist, hclen), where
    assert b["header_bits"] <= bits, (where, b["header_bits"], bits)
    # the smallest of the three forms, and strictly so
    final = b["final"]
    mine = dm.form_bytes(b["header_bits"] + b["payload_bits"], final)
    assert mine < dm.form_bytes(dm.fixed_bits(b["tokens"]), final) and mine < 5 + len(b["data"]), where
    (ll_cost, ll_depth), (d_cost, d_depth) = dm.huffman_cost_and_depth(ll), _distance_cost(d)
    return ll_cost + d_cost + extra, max(ll_depth, d_depth)


CODE_CASES = {"total": ("total", (96, 80, 64), 96, 1), "regions": ("regions", (96, 80, 64), 96, 1), "parts": ("parts", (96, 80, 64), 96, 1),
              "ct_int16": ("ct", (64, 64, 24), 128, 2)}


@pytest.mark.parametrize("case", sorted(CODE_CASES))
def test_codes_are_exact(ctx, case):
    """Every block of the device stream against the model: the same form, the same tokens; a dynamic block's payload costs what an
    optimal prefix code costs for its own histograms (the cost of an optimal code is unique: an equality), as long as a Huffman tree
    of these histograms fits into 15 bits -- which holds for every block of these inputs."""
    name, shape, row, near = CODE_CASES[case]
    payload = _f_order(_phantom(name, shape))
    members = _deflate(ctx, payload, 4 << 20, row, near)
    _check(members, payload.tobytes(), 4 << 20)
    blocks = _blocks(members)
    streams, records = dm.encode_model(payload.tobytes(), 4 << 20, row, near)
    assert [b["type"] for b in blocks] == [r["type"] for r in records]
    n_dyn = 0
    for k, (b, r) in enumerate(zip(blocks, records)):
        if b["type"] == 0:
            continue
        assert b["tokens"] == r["tokens"], f"block {k}: not the greedy parse"
        if b["type"] == 2:
            optimum, depth = _check_dynamic_block(b, f"{case} block {k}")
            assert depth <= 15, f"block {k}: this input was chosen to stay inside the length limit"
            assert b["payload_bits"] == optimum == r["payload_bits"], f"block {k}"
            n_dyn += 1
    assert n_dyn >= len(blocks) // 2
    print(f"{case}: {len(blocks)} blocks, {n_dyn} dynamic; device {_size(members)} B, model {sum(map(len, streams))} B")
    assert _size(members) <= sum(map(len, streams))


def test_forced_length_limit(ctx):
    """A block whose histogram (with the end-of-block symbol) is the first 18 Fibonacci numbers: its Huffman tree is 17 deep.  The
    encoder builds the optimal 15-bit code (package-merge), so the repair may cost nothing: the payload equals the model's
    length-limited optimum."""
    payload = dm.fibonacci_block()
    members = _deflate(ctx, payload, 4 << 20, 0, 1)
    _check(members, payload.tobytes(), 4 << 20)
    (b,) = _blocks(members)
    assert b["type"] == 2 and b["tokens"] == list(payload.tobytes())
    ll, d, extra = dm.histograms(b["tokens"])
    unlimited, depth = dm.huffman_cost_and_depth(ll)
    assert depth >= 16 and not any(d) and extra == 0
    _check_dynamic_block(b, "fibonacci")
    assert max(b["ll_lens"]) == 15 and dm.kraft(b["ll_lens"]) == 1 << 15
    best = sum(f * ln for f, ln in zip(ll, dm.limited_lengths(ll, 15)))
    print(f"fibonacci block: device payload {b['payload_bits']} bits, length-limited optimum {best}, unlimited Huffman {unlimited}")
    assert unlimited < b["payload_bits"] == best


# ---------------------------------------------------------------------------------------------------------------- alphabet edges
def _walk(n, seed, k=4):
    """n bytes of k values, no two neighbours equal: nothing matches at distance 1."""
    steps = np.random.default_rng(seed).integers(1, k, n)
    return (np.cumsum(steps) % k).astype(np.uint8)


def test_block_without_a_match(ctx):
    payload = _walk(16384, 1)
    members = _deflate(ctx, payload, 4 << 20, 0, 1)
    _check(members, payload.tobytes(), 4 << 20)
    (b,) = _blocks(members)
    assert b["type"] == 2 and all(isinstance(t, int) for t in b["tokens"])
    assert b["hdist"] == 1 and b["d_lens"] == [0]
    _check_dynamic_block(b, "no match")


def test_single_distance_code(ctx):
    """Only near matches (no row candidate), and only row matches (a row without equal neighbours, repeated): one 1-bit code."""
    payload = dm.CONTENTS["regions_like"](3 * 16384)
    for near in (1, 2):
        data = np.repeat(payload, near)[:3 * 16384]
        members = _deflate(ctx, data, 4 << 20, 0, near)
        _check(members, data.tobytes(), 4 << 20)
        for b in _blocks(members):
            assert b["type"] == 2 and {t[1] for t in b["tokens"] if isinstance(t, tuple)} == {near}
            assert b["hdist"] == near and b["d_lens"] == [0] * (near - 1) + [1]
            _check_dynamic_block(b, "near only")
    tiled = np.tile(_walk(64, 2), 3 * 256)
    members = _deflate(ctx, tiled, 4 << 20, 64, 1)
    _check(members, tiled.tobytes(), 4 << 20)
    for b in _blocks(members):
        assert b["type"] == 2 and {t[1] for t in b["tokens"] if isinstance(t, tuple)} == {64}
        assert b["hdist"] == 12 and b["d_lens"] == [0] * 11 + [1]          # distances 49 .. 64 are symbol 11
        _check_dynamic_block(b, "row only")


def test_both_distances_one_repeated_byte_and_the_last_symbols(ctx):
    payload = _f_order(_phantom("regions", (96, 80, 64)))
    blocks = _blocks(_deflate(ctx, payload, 4 << 20, 96, 1))
    both = [b for b in blocks if b["type"] == 2 and {t[1] for t in b["tokens"] if isinstance(t, tuple)} == {1, 96}]
    assert both and all(b["d_lens"][0] == 1 and b["d_lens"][12] == 1 and sum(b["d_lens"]) == 2 for b in both)      # 96: symbol 12
    for byte in (0, 7, 255):
        # one literal, 63 full 258-byte matches (symbol 285: HLIT = 286) and a shorter one per block; 255 is the last literal
        payload = np.full(2 * 16384, byte, np.uint8)
        members = _deflate(ctx, payload, 4 << 20, 192, 1)
        _check(members, payload.tobytes(), 4 << 20)
        blocks = _blocks(members)
        assert blocks[0]["tokens"][0] == byte and blocks[0]["ll_lens"][byte]                 # (the only literal of the member)
        for b in blocks:
            assert b["type"] == 2 and b["hlit"] == 286 and b["ll_lens"][285]
            assert sum(1 for t in b["tokens"] if t == (258, 1)) == 63
            _check_dynamic_block(b, f"byte {byte}")


def test_every_length_code(ctx):
    """The prefix image of tests/test_gpu_deflate.py at its row distance: all 29 length symbols, in the forms the model chooses."""
    img = dm.prefix_image()
    members = _deflate(ctx, img, 4 << 20, dm.IMG_W, 1)
    _check(members, img.tobytes(), 4 << 20)
    blocks = _blocks(members)
    _, records = dm.encode_model(img.tobytes(), 4 << 20, dm.IMG_W, 1)
    assert [b["type"] for b in blocks] == [r["type"] for r in records] and 2 in {b["type"] for b in blocks}
    seen = set()
    for b, r in zip(blocks, records):
        if b["type"]:
            assert b["tokens"] == r["tokens"]
            seen |= {dm.len_symbol(t[0])[0] for t in b["tokens"] if isinstance(t, tuple) and b["type"] == 2}
        if b["type"] == 2:
            _check_dynamic_block(b, "prefix image")
    assert seen == set(range(257, 286))


def test_small_blocks_fall_back_to_fixed(ctx):
    """1 .. 64 distinct, scattered byte values: the header of a dynamic block (17 bits, the code-length code, a length per used
    symbol and the zero runs between them) outweighs what its codes save, so the block is fixed -- as the model says.  Where few
    symbols repeat (4 values) a dynamic block can win even here; the form is the model's in every case."""
    perm = np.random.default_rng(6).permutation(144).astype(np.uint8)
    for n in range(1, 65):
        for payload, want in ((perm[:n], 1), (dm.CONTENTS["random0to3"](n), None)):
            members = _deflate(ctx, payload, 4 << 20, 0, 1)
            _check(members, payload.tobytes(), 4 << 20)
            (b,) = _blocks(members)
            _, (r,) = dm.encode_model(payload.tobytes(), 4 << 20, 0, 1)
            assert b["type"] == r["type"] and (want is None or b["type"] == want), n
            if b["type"] == 1:
                assert bytes(members[0][0]) == bytes(_deflate(ctx, payload, 4 << 20, 0, 1, dynamic=False)[0][0])


def test_random_bytes_are_stored_within_the_bound(ctx):
    from boa_hip import _lib
    n, mb, guard = 100_000, 40_000, 4096
    payload = dm.CONTENTS["random"](n)
    bound = int(ctx.lib.boa_deflate_bound(n, mb))
    src = ctx.from_numpy(payload)
    out = ctx.from_numpy(np.full(bound + guard, 0xA5, np.uint8))
    offs, crcs = (C.c_size_t * 4)(), (C.c_uint32 * 3)()
    try:
        _lib.check(ctx.lib.boa_deflate_members2(ctx.h, src.vp, n, mb, 192, 1, 1, out.vp, bound, offs, crcs), "boa_deflate_members2")
        got = out.download((bound + guard,), np.uint8)
        assert list(offs) == [0, 40_000 + 15, 80_000 + 30, bound] and (got[bound:] == 0xA5).all()
        for m in range(3):
            body = got[offs[m]:offs[m + 1]].tobytes()
            assert zlib.decompress(body, -15) == payload[m * mb:(m + 1) * mb].tobytes()
            assert {b["type"] for b in dm.parse_blocks(body)} == {0}
    finally:
        src.free()
        out.free()


# ---------------------------------------------------------------------------------------------------------------- sizes
SIZE_CASES = {"total": ("total", (192, 160, 128), 192, 1), "regions": ("regions", (192, 160, 128), 192, 1),
              "parts": ("parts", (192, 160, 128), 192, 1), "ct_int16": ("ct", (64, 64, 24), 128, 2)}


@pytest.mark.parametrize("case", sorted(SIZE_CASES))
def test_size_against_the_model(ctx, case):
    """At most the model's size x 1.01 (the header's freedom between trees of equal cost); printed with the ratio to zlib level 1."""
    name, shape, row, near = SIZE_CASES[case]
    payload = _f_order(_phantom(name, shape))
    members = _deflate(ctx, payload, 4 << 20, row, near)
    _check(members, payload.tobytes(), 4 << 20)
    fixed = _size(_deflate(ctx, payload, 4 << 20, row, 1, dynamic=False))
    streams, _ = dm.encode_model(payload.tobytes(), 4 << 20, row, near)
    ours, model, ref = _size(members), sum(map(len, streams)), len(zlib.compress(payload.tobytes(), 1))
    print(f"{case}: device dynamic {ours} B, model {model} B, device fixed {fixed} B, zlib level 1 {ref} B, dynamic / zlib-1 {ours / ref:.3f}")
    assert ours <= 1.01 * model and ours < fixed


# ---------------------------------------------------------------------------------------------------------------- fixed mode
def test_fixed_mode_is_untouched_and_both_modes_are_deterministic(ctx):
    payload = _f_order(_phantom("regions", (96, 80, 64)))
    n, mb = len(payload), 100_000
    fixed = _deflate(ctx, payload, mb, 96, dynamic=False)
    n_mem = -(-n // mb)
    bound = int(ctx.lib.boa_deflate_bound(n, mb))
    src, out = ctx.from_numpy(payload), ctx.alloc(bound)
    offs, crcs = (C.c_size_t * (n_mem + 1))(), (C.c_uint32 * n_mem)()
    try:
        assert ctx.lib.boa_deflate_members(ctx.h, src.vp, n, mb, 96, out.vp, bound, offs, crcs) == 0
        got = out.download((int(offs[n_mem]),), np.uint8).tobytes()
    finally:
        src.free()
        out.free()
    assert [bytes(b) for b, _, _ in fixed] == [got[offs[m]:offs[m + 1]] for m in range(n_mem)]
    assert [c for _, c, _ in fixed] == list(crcs)
    assert {b["type"] for b in _blocks(fixed)} <= {0, 1}
    for dynamic in (False, True):
        a = _deflate(ctx, payload, mb, 96, dynamic=dynamic)
        b = _deflate(ctx, payload, mb, 96, dynamic=dynamic)
        assert [(bytes(x), c, s) for x, c, s in a] == [(bytes(x), c, s) for x, c, s in b]
    _check(a, payload.tobytes(), mb)


# ---------------------------------------------------------------------------------------------------------------- upper layers
@pytest.mark.parametrize("dtype", ["uint8", "int16"])
@pytest.mark.parametrize("source", ["devarray_file_order", "devarray_other_order", "numpy"])
def test_nifti_save_dynamic(ctx, tmp_path, source, dtype):
    from boa_hip import nifti
    from boa_hip.devarray import DevArray
    vol = _phantom("regions", (200, 168, 130)) if dtype == "uint8" else _phantom("ct", (160, 128, 110))      # 4.4 MB: two members
    aff = np.diag([-1.5, -1.5, 5.0, 1.0])
    aff[:3, 3] = [10.0, -20.0, 30.0]
    ext = [(0, nifti.label_xml({1: "subcutaneous", 255: "ignore"}))]
    cpu, dev = tmp_path / "cpu.nii.gz", tmp_path / "dev.nii.gz"
    nifti.save(cpu, vol, aff, extensions=ext)
    calls = []
    real = nifti.device_deflate
    nifti.device_deflate = lambda *a, **k: (calls.append(k), real(*a, **k))[1]
    try:
        if source == "numpy":
            nifti.save(dev, vol, aff, extensions=ext, ctx=ctx, dynamic=True)
        else:
            if source == "devarray_file_order":
                d = DevArray.from_numpy(ctx, np.ascontiguousarray(vol.transpose(2, 1, 0))).transpose((2, 1, 0))
                assert d.strides == (1, vol.shape[0], vol.shape[0] * vol.shape[1])
            else:
                d = DevArray.from_numpy(ctx, vol)
            nifti.save(dev, d, aff, extensions=ext, ctx=ctx, dynamic=True)
            np.testing.assert_array_equal(d.download(), vol)
            d.free()
    finally:
        nifti.device_deflate = real
    assert calls == [dict(near_bytes=vol.dtype.itemsize, dynamic=True)]
    raw = dev.read_bytes()
    assert gzip.decompress(raw) == gzip.decompress(cpu.read_bytes())
    tab = nifti._member_table(raw)
    assert tab is not None and [t[2] for t in tab][1:] == [4 << 20, vol.nbytes - (4 << 20)]
    assert 2 in {b["type"] for b in dm.parse_blocks(raw[tab[2][0]:tab[2][1]])}
    got, gaff, hdr = nifti.load(dev, threads=4)
    want, waff, whdr = nifti.load(cpu)
    np.testing.assert_array_equal(got, vol)
    assert got.dtype == vol.dtype and np.array_equal(gaff, waff) and hdr.extensions == whdr.extensions and hdr.raw == whdr.raw
    print(f"{dtype} {source}: device file {len(raw)} B, CPU file {len(cpu.read_bytes())} B")


def test_get_image_info_switch(tmp_path, monkeypatch):
    """image.nii.gz of a 12 x 40 x 48 series: BOA_SAVE_DEVICE=2 sends it through the device encoder once, with near 2 and dynamic
    codes; without the switch and with BOA_SAVE_DEVICE=1 the encoder is not called; the files decompress to the same bytes."""
    from boa_hip import nifti, synthetic
    from boa_hip.compute.io import get_image_info
    from dicom_writer import write_series
    vol = (synthetic.ct_phantom((48, 40, 12), seed=3).astype(np.int32) + 1024).astype(np.uint16).transpose(2, 1, 0)
    write_series(tmp_path / "in", np.ascontiguousarray(vol), bits_stored=12)
    calls = []
    real = nifti.device_deflate
    monkeypatch.setattr(nifti, "device_deflate", lambda *a, **k: (calls.append((a[2], a[3], k)), real(*a, **k))[1])
    raw = {}
    for switch in (None, "1", "2"):
        if switch is None:
            monkeypatch.delenv("BOA_SAVE_DEVICE", raising=False)
        else:
            monkeypatch.setenv("BOA_SAVE_DEVICE", switch)
        del calls[:]
        path, _ = get_image_info(tmp_path / "in", tmp_path / f"out{switch}")
        raw[switch] = path.read_bytes()
        assert calls == ([(48 * 40 * 12 * 2, 48 * 2, dict(near_bytes=2, dynamic=True))] if switch == "2" else []), switch
    assert raw[None] == raw["1"]
    assert gzip.decompress(raw["2"]) == gzip.decompress(raw[None]) and nifti._member_table(raw["2"]) is not None
    data, _, _ = nifti.load(tmp_path / "out2" / "image.nii.gz")
    np.testing.assert_array_equal(data, vol.transpose(2, 1, 0).astype(np.int32) - 1024)
    assert data.dtype == np.int16
