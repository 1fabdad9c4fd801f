"""tests/inflate_model.py against zlib, and the gzip header parser of boa_hip/nifti.py: what the device inflate and its tests rest on."""
import gzip
import itertools
import os
import zlib

import numpy as np
import pytest

import inflate_model as im
from conftest import GOLDEN


@pytest.fixture(scope="module")
def streams():
    """{(payload name, encoder name): (raw deflate body, payload)} of the GPU tests' list."""
    return {(pn, en): (enc(p), p) for pn, p in im.payloads().items() for en, enc in im.ENCODERS.items()}


def test_model_inflate_equals_zlib(streams):
    for key, (body, payload) in streams.items():
        out, bounds = im.inflate(body)
        assert out == payload == zlib.decompress(body, -15), key
        assert bounds[0][0] == 0 and bounds[-1][2] == 1, key
    # the list reaches every block type, and empty stored blocks in the flushed streams
    body, _ = streams["ct_phantom", "sync_flush"]
    assert {b[1] for b in im.inflate(body)[1]} >= {0, 2}
    assert {b[1] for b in im.inflate(streams["ct_phantom", "fixed"][0])[1]} == {1}


def test_block_start_accepts_every_true_dynamic_boundary(streams):
    """The block-start test is true at every true dynamic non-final boundary, and false at the stored, fixed and final ones.  For
    information: over 1 MiB of random bytes (default_rng(1), all 8 388 608 bit offsets) it accepted 0 offsets when this test was
    written; the test scans 64 KiB of it and only asserts that a random hit is rare."""
    seen = 0
    for key, (body, _) in streams.items():
        for bit, btype, final in im.inflate(body)[1]:
            if btype == 2 and not final:
                assert im.block_start(body, bit), (key, bit)
                seen += 1
            else:
                assert not im.block_start(body, bit), (key, bit)       # stored, fixed and final blocks are no candidates
    assert seen > 100
    noise = np.random.default_rng(1).integers(0, 256, 65536, dtype=np.uint8).tobytes()
    hits = sum(1 for bit in im._header_bits(noise, 0, 8 * len(noise) - 64) if im.block_start(noise, int(bit)))
    assert hits <= 2


@pytest.mark.parametrize("key", [("ct_phantom", "full_flush"), ("ct_phantom", "level1"), ("label_phantom", "level6"),
                                 ("one_byte", "level6"), ("empty", "level6")])
def test_model_chunked_inflate(streams, key):
    body, payload = streams[key]
    out, info = im.chunked_inflate(body, 512)
    assert out == payload
    assert info["rejected"] == 0 or info["candidates"] > 0


def test_model_markers_cross_chunks():
    """Distance 16384 everywhere: split at the true block boundaries, every chunk's symbols are markers into its predecessor."""
    block = np.random.default_rng(17).integers(0, 256, 16384, dtype=np.uint8).tobytes()
    payload = block * 8
    body = im.ENCODERS["sync_flush"](payload)
    starts = [b[0] for b in im.inflate(body)[1] if b[1] != 0 and not b[2]]      # (the model's chain takes any true boundary)
    assert len(starts) > 3
    syms, _, _ = im.decode(body, starts[-1], im.NO_STOP, markers=True)
    assert any(s & 0x8000 for s in syms)
    out, info = im.chunked_inflate(body, 4096, starts=[0] + starts[1:])
    assert out == payload and info["live"] == len(starts) and info["rejected"] == 0


def test_model_rejects_the_planted_decoy():
    body, payload, bit = im.planted_decoy()
    assert im.block_start(body, bit)
    assert not any(b[0] == bit for b in im.inflate(body)[1])
    out, info = im.chunked_inflate(body, 4096)
    assert out == payload and info["rejected"] >= 1


# ---- the gzip header parser ----
def test_gzip_header_every_flag_combination():
    from boa_hip import nifti
    payload = b"header test " * 20
    body = zlib.compress(payload, 6)[2:-4]
    for text, hcrc, extra, name, comment in itertools.product((0, 1), repeat=5):
        flags = text | hcrc << 1 | extra << 2 | name << 3 | comment << 4
        raw = im.gzip_wrap(body, payload, flags, extra=b"AB\x03\x00xyz", name=b"ct.nii", comment=b"a comment")
        assert gzip.decompress(raw) == payload, flags                      # the writer of this test is right
        at = nifti.gzip_header_end(raw)
        assert at is not None and raw[at:len(raw) - 8] == body, flags
        assert nifti._gzip_streams(raw) == [(at, len(raw) - 8, len(payload), zlib.crc32(payload))]
        for cut in range(at):                                              # truncated inside the header
            assert nifti.gzip_header_end(raw[:cut]) is None, (flags, cut)
        if hcrc:
            bad = bytearray(raw)
            bad[at - 1] ^= 1
            assert nifti.gzip_header_end(bytes(bad)) is None
    assert nifti.gzip_header_end(b"\x1f\x8b\x07" + bytes(20)) is None       # method
    assert nifti.gzip_header_end(b"\x1f\x8b\x08\x20" + bytes(20)) is None   # reserved flag
    assert nifti.gzip_header_end(b"\x1f\x8c\x08\x00" + bytes(20)) is None   # magic
    assert nifti._gzip_streams(b"") is None


def test_gzip_header_of_the_reference_file_and_of_own_files(tmp_path):
    from boa_hip import nifti
    with open(os.path.join(GOLDEN, "ref_example_ct_sm.nii.gz"), "rb") as f:
        raw = f.read()
    (lo, hi, size, crc), = nifti._gzip_streams(raw)
    payload = gzip.decompress(raw)
    assert zlib.decompress(raw[lo:hi], -15) == payload and size == len(payload) and crc == zlib.crc32(payload)
    vol = (np.arange(40 * 30 * 20) % 7).astype(np.uint8).reshape(40, 30, 20)
    nifti.save(tmp_path / "own.nii.gz", vol, np.eye(4))
    own = (tmp_path / "own.nii.gz").read_bytes()
    streams = nifti._gzip_streams(own)
    assert len(streams) == 2                                               # header member, data member
    assert b"".join(zlib.decompress(own[a:b], -15) for a, b, _, _ in streams) == gzip.decompress(own)
    assert all(zlib.crc32(zlib.decompress(own[a:b], -15)) == c and n == len(zlib.decompress(own[a:b], -15)) for a, b, n, c in streams)


def test_load_without_a_context_and_the_switch(tmp_path, monkeypatch):
    """ctx=None changes nothing, and the file-level callers pass their context only under BOA_LOAD_DEVICE=1."""
    from boa_hip import nifti
    monkeypatch.setattr(nifti, "device_inflate", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device path without a context")))
    vol = (np.arange(24 * 20 * 16) % 5).astype(np.int16).reshape(24, 20, 16)
    nifti.save(tmp_path / "v.nii.gz", vol, np.eye(4))
    assert (nifti.load(tmp_path / "v.nii.gz")[0] == vol).all() and (nifti.load(tmp_path / "v.nii.gz", ctx=None)[0] == vol).all()
    token = object()
    monkeypatch.delenv("BOA_LOAD_DEVICE", raising=False)
    assert nifti.load_context(token) is None
    monkeypatch.setenv("BOA_LOAD_DEVICE", "0")
    assert nifti.load_context(token) is None
    monkeypatch.setenv("BOA_LOAD_DEVICE", "1")
    assert nifti.load_context(token) is token
