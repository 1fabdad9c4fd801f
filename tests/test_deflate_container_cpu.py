"""CPU: the gzip member container that `nifti.save` shares between its zlib path and the device encoder (csrc/deflate.hip), pinned
with bodies made by zlib, and the guarantee that nothing changes for callers that do not ask for the device path."""
import gzip
import struct
import zlib

import numpy as np
import pytest

from boa_hip import nifti


def _raw_deflate(piece: bytes) -> bytes:
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    return c.compress(piece) + c.flush()


def _payload(n, seed=3):
    rng = np.random.default_rng(seed)
    runs = np.repeat(rng.integers(0, 120, n // 40 + 1, dtype=np.uint8), rng.integers(1, 80, n // 40 + 1))[:n]
    return np.concatenate([runs, rng.integers(0, 256, n - len(runs), dtype=np.uint8)]).tobytes()


@pytest.mark.parametrize("cuts", [(0, 70_000), (0, 1, 2, 40_000, 40_001, 90_000), (0, 0, 5000)])
def test_wrapped_members_inflate_with_gzip_and_read_bytes(tmp_path, cuts):
    """(body, crc, length) triples -> file: gzip reads it as one stream and verifies every CRC-32 and ISIZE; read_bytes finds the
    "BO" index in every member and inflates them in parallel.  Ragged members and an empty one included."""
    payload = _payload(cuts[-1])
    pieces = [payload[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    path = tmp_path / "x.bin.gz"
    with open(path, "wb") as f:
        nifti.write_wrapped_members(f, [(_raw_deflate(p), zlib.crc32(p), len(p)) for p in pieces])
    raw = path.read_bytes()
    assert gzip.decompress(raw) == payload
    tab = nifti._member_table(raw)
    assert tab is not None and [t[2] for t in tab] == [len(p) for p in pieces]
    assert bytes(nifti.read_bytes(path, threads=4)) == payload
    assert bytes(nifti.read_bytes(path, threads=1)) == payload
    # the container itself: magic, deflate, FEXTRA with the "BO" subfield holding the member's total length
    first = nifti.gzip_member(_raw_deflate(pieces[0]), zlib.crc32(pieces[0]), len(pieces[0]))
    assert raw.startswith(first) and first[:4] == b"\x1f\x8b\x08\x04" and first[10:16] == b"\x08\x00BO\x04\x00"
    assert struct.unpack("<I", first[16:20])[0] == len(first)
    assert struct.unpack("<II", first[-8:]) == (zlib.crc32(pieces[0]), len(pieces[0]))


def test_a_wrong_crc_is_caught_by_both_readers(tmp_path):
    payload = _payload(30_000)
    path = tmp_path / "bad.bin.gz"
    with open(path, "wb") as f:
        nifti.write_wrapped_members(f, [(_raw_deflate(payload[:10_000]), zlib.crc32(payload[:10_000]), 10_000),
                                        (_raw_deflate(payload[10_000:]), zlib.crc32(payload[10_000:]) ^ 1, 20_000)])
    with pytest.raises(Exception):
        gzip.decompress(path.read_bytes())
    with pytest.raises(ValueError):
        nifti.read_bytes(path, threads=4)


@pytest.mark.parametrize("dtype,shape,threads", [(np.uint8, (37, 29, 11), 1), (np.uint8, (130, 128, 300), 4), (np.int16, (64, 40, 9), 2)])
def test_save_without_ctx_writes_what_write_gzip_members_writes(tmp_path, dtype, shape, threads):
    """`nifti.save(path, data, affine)` = header + extensions as one run of members, then the F-ordered data as another, both straight
    from write_gzip_members (zlib level 1, 4 MiB members): the path every caller had before the `ctx` keyword existed."""
    rng = np.random.default_rng(1)
    data = (rng.integers(0, 5, shape) * 40).astype(dtype)
    aff = np.diag([-1.5, -1.5, 3.0, 1.0])
    ext = [(0, nifti.label_xml({1: "a", 2: "b"}))]
    p = tmp_path / "a.nii.gz"
    nifti.save(p, data, aff, extensions=ext, threads=threads)
    blob = bytes(nifti.read_bytes(p))
    vox = int(struct.unpack("<f", blob[108:112])[0])
    assert blob[vox:] == np.asfortranarray(data).reshape(-1, order="F").tobytes()
    q = tmp_path / "b.nii.gz"
    with open(q, "wb") as f:
        nifti.write_gzip_members(f, blob[:vox], 1, 1)
        nifti.write_gzip_members(f, blob[vox:], 1, threads)
    assert p.read_bytes() == q.read_bytes()
    # and explicitly ctx=None is that same path
    r = tmp_path / "c.nii.gz"
    nifti.save(r, data, aff, extensions=ext, threads=threads, ctx=None)
    assert r.read_bytes() == p.read_bytes()
    got, gaff, hdr = nifti.load(p)
    np.testing.assert_array_equal(got, data)
    assert np.allclose(gaff, aff) and hdr.extensions == [(0, ext[0][1] + b"\0" * ((-8 - len(ext[0][1])) % 16))]


@pytest.mark.parametrize("env", [None, "0", ""])
def test_file_level_callers_stay_off_the_device_without_the_switch(tmp_path, monkeypatch, env):
    """compute_all_models and the ct_pfav writer save through `nifti.save_volume` with their context; unless BOA_SAVE_DEVICE is 1
    that must never reach the device encoder."""
    import inspect

    from boa_hip.compute import inference, measurements

    def boom(*a, **k):
        raise AssertionError("device encoder called without BOA_SAVE_DEVICE=1")

    monkeypatch.setattr(nifti, "device_deflate", boom)
    monkeypatch.setattr(nifti, "_device_body", boom)
    if env is None:
        monkeypatch.delenv("BOA_SAVE_DEVICE", raising=False)
    else:
        monkeypatch.setenv("BOA_SAVE_DEVICE", env)
    data = (np.arange(20 * 12 * 7) % 3).astype(np.uint8).reshape(20, 12, 7)
    aff = np.eye(4)
    nifti.save_volume(tmp_path / "v.nii.gz", data, aff, ctx=object())
    nifti.save(tmp_path / "w.nii.gz", data, aff)
    assert (tmp_path / "v.nii.gz").read_bytes() == (tmp_path / "w.nii.gz").read_bytes()
    # with the switch on, a uint8 volume does go there (and only a uint8 .gz one)
    monkeypatch.setenv("BOA_SAVE_DEVICE", "1")
    with pytest.raises(AssertionError, match="device encoder"):
        nifti.save_volume(tmp_path / "x.nii.gz", data, aff, ctx=object())
    nifti.save_volume(tmp_path / "y.nii.gz", data.astype(np.int16), aff, ctx=object())
    nifti.save_volume(tmp_path / "z.nii", data, aff, ctx=object())
    nifti.save_volume(tmp_path / "n.nii.gz", data, aff, ctx=None)
    # the label-volume writers of the file-level interface all go through save_volume; image.nii.gz (int16 CT) does not
    src = inspect.getsource(inference)
    assert src.count("nifti.save_volume(") == 3 and "nifti.save(" not in src
    assert 'nifti.save_volume(segmentation_folder / "ct_pfav.nii.gz"' in inspect.getsource(measurements)
