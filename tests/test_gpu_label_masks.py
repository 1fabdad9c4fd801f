"""Per-structure mask files from a label volume on the device: the presence pass (`boa_label_member_presence`) against numpy, the fused
mask encode (`boa_deflate_label_pairs`) byte for byte against `boa_deflate_members2` on the uploaded (labels == k) mask and against
zlib's inflate and CRC-32, and `nifti.save_label_masks` / `task.write_structure_masks` against `nifti.save` of every mask.  The cases
come from tests/label_mask_cases.py (pinned by tests/test_label_mask_cases_cpu.py)."""
import ctypes as C
import functools
import gzip
import os
import zlib

import numpy as np
import pytest

import label_mask_cases as lm

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in lm.cases()}
ROWS = (0, 37, 40000)             # no row candidate, the volume's x-row, beyond the encoder's 32 768 (= none)
GUARD = 4096


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.compute.inference import get_context
    return get_context("gpu")


class _Source:
    """`payload` on the device, `shift` bytes off the (256-byte aligned) start of its buffer, one byte of padding behind it."""

    def __init__(self, ctx, payload, shift=0):
        payload = np.asarray(payload, np.uint8).reshape(-1)
        self.buf = ctx.from_numpy(np.concatenate([np.full(shift, 0xEE, np.uint8), payload, np.full(1, 0xEE, np.uint8)]))
        self.ptr, self.n = self.buf.ptr + shift, payload.size

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.buf.free()


def _presence_words(ctx, ptr, n, member_bytes):
    from boa_hip import _lib
    bits = np.full((lm.n_members(n, member_bytes), 8), 0xDEADBEEF, dtype="<u4")
    _lib.check(ctx.lib.boa_label_member_presence(ctx.h, C.c_void_p(ptr), n, member_bytes, bits.ctypes.data_as(C.POINTER(C.c_uint32))),
               "boa_label_member_presence")
    return bits


@functools.lru_cache(maxsize=None)
def _mask_members(ctx, key, label, member_bytes, row, dynamic):
    """The reference: `boa_deflate_members2` (near 1) on the uploaded mask of `label` -> ((body bytes, crc32, size), ..) per member."""
    from boa_hip import nifti
    payload = lm.volume() if key == "volume" else CASES[key]["payload"]
    mask = (payload == label).astype(np.uint8)
    with _Source(ctx, mask) as s:
        return tuple((bytes(b), c, z) for b, c, z in nifti.device_deflate(ctx, s.ptr, s.n, row, member_bytes, dynamic=dynamic))


def _check_pairs(ctx, key, payload, got, pairs, member_bytes, row, dynamic):
    assert len(got) == len(pairs)
    for (k, m), (body, crc, size) in zip(pairs, got):
        want = lm.pair_payload(payload, member_bytes, k, m)
        where = f"{key}: label {k} member {m} row {row} dynamic {dynamic}"
        assert size == len(want), where
        d = zlib.decompressobj(-15)
        assert d.decompress(bytes(body)) + d.flush() == want and d.eof and d.unused_data == b"", where
        assert crc == zlib.crc32(want), where
        ref = _mask_members(ctx, key, k, member_bytes, row, dynamic)[m]
        assert (bytes(body), crc, size) == ref, where


# ---------------------------------------------------------------------------------------------------------------- presence
@pytest.mark.parametrize("shift", [0, 1])
def test_presence_equals_numpy(ctx, shift):
    v = lm.volume()
    with _Source(ctx, v, shift) as s:
        for mb in lm.PRESENCE_MEMBER_BYTES:
            want = lm.presence_words(lm.presence_table(v, mb))
            got = _presence_words(ctx, s.ptr, s.n, mb)
            np.testing.assert_array_equal(got, want, err_msg=f"member_bytes {mb}")
            np.testing.assert_array_equal(_presence_words(ctx, s.ptr, s.n, mb), got)      # deterministic


@pytest.mark.parametrize("name", sorted(CASES))
def test_presence_of_the_cases(ctx, name):
    from boa_hip import nifti
    c = CASES[name]
    with _Source(ctx, c["payload"], c["shift"]) as s:
        for mb in sorted({c["member_bytes"], 17, 4096} | ({1} if len(c["payload"]) <= 20_000 else set())):
            want = lm.presence_table(c["payload"], mb)
            np.testing.assert_array_equal(_presence_words(ctx, s.ptr, s.n, mb), lm.presence_words(want), err_msg=f"member_bytes {mb}")
        np.testing.assert_array_equal(nifti.label_member_presence(ctx, s.ptr, s.n, c["member_bytes"]), lm.presence_table(c["payload"], c["member_bytes"]))


def test_presence_of_a_volume_that_spans_many_workgroups(ctx):
    """1 MiB + 5 bytes (33 workgroups of 32 KiB), members that straddle workgroups and vectors (65 537) and members of one vector"""
    rng = np.random.default_rng(11)
    p = np.repeat(rng.integers(0, 256, 1 + (1 << 20) // 512).astype(np.uint8), 512)[:(1 << 20) + 5]
    p[rng.integers(0, p.size, 64)] = rng.integers(0, 256, 64).astype(np.uint8)          # single voxels
    with _Source(ctx, p, 3) as s:
        for mb in (16, 65537, 1 << 20, 1 << 30):
            np.testing.assert_array_equal(_presence_words(ctx, s.ptr, s.n, mb), lm.presence_words(lm.presence_table(p, mb)), err_msg=f"member_bytes {mb}")


def test_presence_refuses_bad_sizes(ctx):
    from boa_hip import _lib
    bits = (C.c_uint32 * 8)()
    with _Source(ctx, np.zeros(16, np.uint8)) as s:
        for mb in (0, (1 << 30) + 1):
            assert ctx.lib.boa_label_member_presence(ctx.h, C.c_void_p(s.ptr), 16, mb, bits) == _lib.BOA_EINVAL
            assert "member_bytes" in ctx.lib.boa_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- pairs
@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("dynamic", [False, True])
def test_pairs_of_the_volume_equal_the_mask_encoder(ctx, dynamic, row):
    """every (label, member) pair of the volume's ids and of an id it does not hold, present or not, at members of 4096 bytes"""
    from boa_hip import nifti
    v, mb = lm.volume(), 4096
    ids = sorted(set(v.tolist())) + [100]
    pairs = [(k, m) for k in ids for m in range(lm.n_members(v.size, mb))]
    table = lm.presence_table(v, mb)
    assert any(table[m, k] for k, m in pairs) and any(not table[m, k] for k, m in pairs)
    with _Source(ctx, v) as s:
        got = nifti.device_deflate_label_pairs(ctx, s.ptr, s.n, pairs, row, mb, dynamic=dynamic)
        _check_pairs(ctx, "volume", v, got, pairs, mb, row, dynamic)
        again = nifti.device_deflate_label_pairs(ctx, s.ptr, s.n, pairs, row, mb, dynamic=dynamic)
        assert [(bytes(b), c, z) for b, c, z in got] == [(bytes(b), c, z) for b, c, z in again]      # deterministic
        # any order, with repeats: a pair's body does not depend on its neighbours in the list
        mixed = pairs[::-3] + pairs[:5] + pairs[:5]
        _check_pairs(ctx, "volume", v, nifti.device_deflate_label_pairs(ctx, s.ptr, s.n, mixed, row, mb, dynamic=dynamic), mixed, mb, row, dynamic)


@pytest.mark.parametrize("name", sorted(CASES))
def test_pairs_of_the_cases_equal_the_mask_encoder(ctx, name):
    from boa_hip import nifti
    c = CASES[name]
    payload, mb = c["payload"], c["member_bytes"]
    nm = lm.n_members(len(payload), mb)
    pairs = list(c["present"]) + list(c["absent"]) + [(k, m) for k, _, _, _ in c["boundary"] for m in range(nm)]
    with _Source(ctx, payload, c["shift"]) as s:
        for dynamic in (False, True):
            for row in ROWS:
                got = nifti.device_deflate_label_pairs(ctx, s.ptr, s.n, pairs, row, mb, dynamic=dynamic)
                _check_pairs(ctx, name, payload, got, pairs, mb, row, dynamic)


def test_absent_pairs_are_the_canned_zero_member(ctx):
    from boa_hip import nifti
    v, mb = lm.volume(), 4096
    nm = lm.n_members(v.size, mb)
    table = lm.presence_table(v, mb)
    absent = [(k, m) for k in (1, 5, 12, 100, 254, 255) for m in range(nm) if not table[m, k]]
    assert {m for _, m in absent} == set(range(nm))
    for dynamic in (False, True):
        zero = {}
        for size in (mb, v.size - (nm - 1) * mb):
            z = ctx.zeros(size)
            (body, crc, got_size), = nifti.device_deflate(ctx, z.ptr, size, 37, size, dynamic=dynamic)
            z.free()
            zero[size] = (bytes(body), crc, got_size)
            assert zlib.decompress(bytes(body), -15) == bytes(size) and crc == zlib.crc32(bytes(size))
        with _Source(ctx, v) as s:
            got = nifti.device_deflate_label_pairs(ctx, s.ptr, s.n, absent, 37, mb, dynamic=dynamic)
        for (k, m), (body, crc, size) in zip(absent, got):
            assert (bytes(body), crc, size) == zero[size], (k, m, dynamic)


def test_bad_arguments_are_refused_before_any_launch(ctx):
    from boa_hip import _lib, nifti
    v, mb = lm.volume(), 4096
    nm = lm.n_members(v.size, mb)
    pairs = [(1, 0), (2, 3), (255, nm - 1)]
    cap = nifti.pair_capacity(ctx, v.size, mb, [m for _, m in pairs])
    assert cap == 2 * (4096 + 5) + (v.size - (nm - 1) * mb + 5)
    offs, crcs = (C.c_size_t * 4)(*[7] * 4), (C.c_uint32 * 3)()
    out = ctx.from_numpy(np.full(cap + GUARD, 0xA5, np.uint8))

    def call(members, n_pairs, capacity, flags=0):
        lab = (C.c_uint8 * 3)(*[k for k, _ in pairs])
        mem = (C.c_uint32 * 3)(*members)
        return ctx.lib.boa_deflate_label_pairs(ctx.h, C.c_void_p(s.ptr), s.n, mb, 37, flags, lab, mem, n_pairs, out.vp, capacity, offs, crcs)

    with _Source(ctx, v) as s:
        try:
            good = [m for _, m in pairs]
            for args, word in (((good, 3, cap - 1), "out_capacity"), (([0, 3, nm], 3, cap), "member"), (([0, 3, 0xFFFFFFFF], 3, cap), "member"),
                               ((good, 3, cap, 2), "flags"), ((good, 3, cap, 3), "flags"), ((good, 3, cap, -1), "flags"),
                               ((good, -1, cap), "n_pairs")):
                assert call(*args) == _lib.BOA_EINVAL, args
                assert word in ctx.lib.boa_last_error().decode(), args
            assert ctx.lib.boa_deflate_label_pairs(ctx.h, C.c_void_p(s.ptr), s.n, 0, 37, 0, None, None, 0, out.vp, 0, offs, crcs) == _lib.BOA_EINVAL
            # no pairs: nothing to do, nothing touched
            assert call(good, 0, 0) == _lib.BOA_OK and offs[0] == 0
            assert ctx.lib.boa_deflate_label_pairs(ctx.h, C.c_void_p(s.ptr), s.n, mb, 37, 0, None, None, 0, None, 0, offs, None) == _lib.BOA_OK
            assert (out.download((cap + GUARD,), np.uint8) == 0xA5).all()
            # the smallest capacity that is accepted is enough, and nothing is written behind the bodies
            assert call(good, 3, cap) == _lib.BOA_OK
            got = out.download((cap + GUARD,), np.uint8)
            assert 0 < offs[3] <= cap and (got[offs[3]:] == 0xA5).all()
        finally:
            out.free()


def test_random_bits_stay_within_the_bound(ctx):
    """the mask of a random 0 / 1 volume, every form the encoder has tried on it; the body fits the capacity the call asks for"""
    from boa_hip import nifti
    c = CASES["random_bits"]
    with _Source(ctx, c["payload"]) as s:
        for dynamic in (False, True):
            (body, crc, size), = nifti.device_deflate_label_pairs(ctx, s.ptr, s.n, [(1, 0)], 0, c["member_bytes"], dynamic=dynamic)
            assert len(body) <= nifti.pair_capacity(ctx, s.n, c["member_bytes"], [0]) and size == s.n
            print(f"random bits, dynamic {dynamic}: {s.n} B -> {len(body)} B")


# ---------------------------------------------------------------------------------------------------------------- files
NAMES = {1: "box_a", 5: "box_e", 12: "box_l", 13: "first_voxel", 254: "x_row", 255: "last_voxel", 100: "absent", 0: "background"}


@pytest.fixture(scope="module")
def like(tmp_path_factory):
    """the header of a CT file as the pipeline has it (int16, its own pixdim units and descrip)"""
    from boa_hip import nifti
    p = tmp_path_factory.mktemp("like") / "ct.nii.gz"
    nifti.save(p, np.zeros(lm.VOLUME_SHAPE, np.int16), _affine(), form_codes=(1, 1))
    return nifti.load(p)[2]


def _affine():
    aff = np.diag([-1.5, -1.5, 3.0, 1.0])
    aff[:3, 3] = [10.0, -20.0, 30.0]
    return aff


def _volume3d():
    return lm.volume().reshape(lm.VOLUME_SHAPE, order="F")


def _read_all(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


@pytest.mark.parametrize("dynamic", [False, True])
def test_files_equal_nifti_save_of_every_mask(ctx, tmp_path, monkeypatch, like, dynamic):
    """members of 4096 bytes (the module's member size, set for this test) so that the small volume has seven of them"""
    from boa_hip import nifti
    monkeypatch.setattr(nifti, "_GZ_BLOCK", 4096)
    seg, aff = _volume3d(), _affine()
    out = tmp_path / "masks"
    out.mkdir()
    info = {}
    nifti.save_label_masks(out, seg, aff, NAMES, ctx, like=like, dynamic=dynamic, info=info)
    files = _read_all(out)
    assert sorted(files) == sorted(f"{v}.nii.gz" for v in NAMES.values())
    table = lm.presence_table(lm.volume(), 4096)
    assert info["pairs"] == len(NAMES) * 7 and info["present"] == int(sum(table[:, k].sum() for k in NAMES)) < info["pairs"]
    assert info["compressed_bytes"] == sum(map(len, files.values()))
    for k, name in NAMES.items():
        mask = (seg == k).astype(np.uint8)
        dev, cpu = tmp_path / "dev.nii.gz", tmp_path / "cpu.nii.gz"
        nifti.save(dev, mask, aff, like=like, ctx=ctx, dynamic=dynamic)
        nifti.save(cpu, mask, aff, like=like)
        raw = files[f"{name}.nii.gz"]
        assert raw == dev.read_bytes(), name
        assert gzip.decompress(raw) == gzip.decompress(cpu.read_bytes()), name
        assert len(nifti._member_table(raw)) == 1 + 7
        got, gaff, hdr = nifti.load(out / f"{name}.nii.gz", threads=4)
        np.testing.assert_array_equal(got, mask)
        assert got.dtype == np.uint8 and np.array_equal(gaff, aff) and hdr.get_data_dtype() == np.uint8
    assert not nifti.load(out / "absent.nii.gz")[0].any()


def test_grouping_determinism_and_device_arrays(ctx, tmp_path, monkeypatch, like):
    from boa_hip import nifti
    from boa_hip.devarray import DevArray
    monkeypatch.setattr(nifti, "_GZ_BLOCK", 4096)
    seg, aff = _volume3d(), _affine()
    calls = []
    real = nifti.device_deflate_label_pairs
    monkeypatch.setattr(nifti, "device_deflate_label_pairs", lambda *a, **k: (calls.append(len(a[3])), real(*a, **k))[1])

    def run(tag, data=seg, **kw):
        d = tmp_path / tag
        d.mkdir()
        del calls[:]
        nifti.save_label_masks(d, data, aff, NAMES, ctx, like=like, **kw)
        return _read_all(d), list(calls)

    want, n_default = run("default")
    present = sum(n_default)
    assert len(n_default) == 1 and present > 6
    again, _ = run("again")
    assert again == want                                             # two runs are byte-identical
    one, n_one = run("one", group_bytes=4096)
    assert one == want and n_one == [1] * present
    three, n_three = run("three", group_bytes=3 * 4096)
    assert three == want and sum(n_three) == present and max(n_three) == 3 and len(n_three) > 2
    # a DevArray in file order is read in place, any other one is reordered on the device
    d_file = DevArray.from_numpy(ctx, np.ascontiguousarray(seg.transpose(2, 1, 0))).transpose((2, 1, 0))
    assert d_file.strides == (1, seg.shape[0], seg.shape[0] * seg.shape[1])
    d_other = DevArray.from_numpy(ctx, np.ascontiguousarray(seg))
    assert run("dev_file", d_file)[0] == want and run("dev_other", d_other)[0] == want
    np.testing.assert_array_equal(d_file.download(), seg)
    d_file.free()
    d_other.free()
    with pytest.raises(TypeError, match="uint8"):
        nifti.save_label_masks(tmp_path, seg.astype(np.int16), aff, NAMES, ctx)
    with pytest.raises(ValueError, match="0 .. 255"):
        nifti.save_label_masks(tmp_path, seg, aff, {256: "x"}, ctx)


def test_write_structure_masks_selects_as_the_reference(ctx, tmp_path, like):
    """the module's own member size (one member here); `roi_subset` writes only the named files, into a folder it creates"""
    from boa_hip import nifti
    from boa_hip.task import write_structure_masks
    seg, aff = _volume3d(), _affine()
    names = {k: v for k, v in NAMES.items() if k}
    assert write_structure_masks(ctx, seg, aff, names, tmp_path / "all" / "total", like=like) == list(names.values())
    assert sorted(os.listdir(tmp_path / "all" / "total")) == sorted(f"{v}.nii.gz" for v in names.values())
    subset = ["x_row", "absent", "not_a_class"]
    assert write_structure_masks(ctx, seg, aff, names, tmp_path / "sub", like=like, roi_subset=subset) == ["x_row", "absent"]
    assert sorted(os.listdir(tmp_path / "sub")) == ["absent.nii.gz", "x_row.nii.gz"]
    for k, name in names.items():
        ref = tmp_path / "ref.nii.gz"
        nifti.save(ref, (seg == k).astype(np.uint8), aff, like=like, ctx=ctx)
        assert (tmp_path / "all" / "total" / f"{name}.nii.gz").read_bytes() == ref.read_bytes(), name
    assert (tmp_path / "sub" / "x_row.nii.gz").read_bytes() == (tmp_path / "all" / "total" / "x_row.nii.gz").read_bytes()
    got, gaff, _ = nifti.load(tmp_path / "sub" / "absent.nii.gz")
    assert got.shape == seg.shape and not got.any() and np.array_equal(gaff, aff)
