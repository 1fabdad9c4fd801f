"""The device inflate (csrc/inflate.hip, `boa_inflate_streams`, `nifti.device_inflate`) against zlib: every stream of
tests/inflate_model.py at three chunk sizes must come back byte-identical through the device path, a planted false block start must
be rejected by the chain check, files of other writers and of this project must load to the same arrays with and without a
context, and damaged files must report a status and raise what the host path raises."""
import gzip
import json
import os
import zlib

import numpy as np
import pytest

import inflate_model as im
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CHUNKS = (512, 4096, None)         # None = the default of boa_inflate_default_chunk()
PAYLOADS = ("ct_phantom", "label_phantom", "empty", "one_byte", "random300k", "zeros1m", "repeat32k", "repeat16k")


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.compute.inference import get_context
    return get_context("gpu")


@pytest.fixture(scope="module")
def payloads():
    return im.payloads()


def _inflate(ctx, raw, chunk):
    from boa_hip import nifti
    return nifti.device_inflate(ctx, raw, chunk_bytes=chunk)


@pytest.mark.parametrize("name", PAYLOADS)
def test_every_encoder_and_chunk_size(ctx, payloads, name):
    payload = payloads[name]
    assert len(payload) <= 1 << 20
    for enc_name, enc in im.ENCODERS.items():
        body = enc(payload)
        assert zlib.decompress(body, -15) == payload
        raw = im.gzip_wrap(body, payload)
        for chunk in CHUNKS:
            out, info = _inflate(ctx, raw, chunk)
            assert info["host"] is False and info["status"] == ["ok"], (name, enc_name, chunk, info)
            assert out.dtype == np.uint8 and out.tobytes() == payload, (name, enc_name, chunk, info)
            assert info["chunks"] == max(1, -(-len(body) // (chunk or 65536))) and 1 <= info["live"] <= info["chunks"]
            assert info["rejected"] <= info["candidates"] < info["chunks"]
            if enc_name in ("fixed", "level0"):        # no dynamic block: a candidate, if any, is false, and chunk 0's decode goes on
                assert info["candidates"] == info["rejected"], (name, enc_name, chunk, info)


def test_the_chunks_do_decode_in_parallel(ctx, payloads):
    """A flushed stream has a dynamic block start every 3 000 payload bytes: at 512 and 4096 bytes per chunk most chunks find one
    and stay in the chain, and every match of the repeated block reaches into an earlier chunk."""
    for name in ("ct_phantom", "repeat16k"):
        body = im.ENCODERS["sync_flush"](payloads[name])
        raw = im.gzip_wrap(body, payloads[name])
        for chunk in (512, 4096):
            out, info = _inflate(ctx, raw, chunk)
            assert out.tobytes() == payloads[name] and not info["host"]
            assert info["live"] >= 4 and info["live"] >= info["candidates"] - info["rejected"], (name, chunk, info)


def test_planted_false_block_start(ctx):
    body, payload, bit = im.planted_decoy()
    assert im.block_start(body, bit)                                       # not vacuous: the find pass's test accepts the decoy
    assert all(b[0] != bit for b in im.inflate(body)[1])                   # and it is no block boundary
    raw = im.gzip_wrap(body, payload)
    for chunk in CHUNKS:
        out, info = _inflate(ctx, raw, chunk)
        assert not info["host"] and out.tobytes() == payload == zlib.decompress(body, -15), (chunk, info)
        if chunk is not None and bit >= 8 * chunk:                         # (inside chunk 0 nobody looks for a start)
            assert info["rejected"] >= 1 and info["rounds"] >= 1, (chunk, info)
    assert bit >= 8 * 4096


def test_optional_header_fields(ctx, payloads):
    body = im.ENCODERS["level6"](payloads["label_phantom"])
    raw = im.gzip_wrap(body, payloads["label_phantom"], flags=1 | 2 | 4 | 8 | 16, extra=b"AB\x02\x00xy", name=b"v.nii", comment=b"c")
    assert gzip.decompress(raw) == payloads["label_phantom"]
    out, info = _inflate(ctx, raw, 4096)
    assert not info["host"] and out.tobytes() == payloads["label_phantom"]


def _same(a, b):
    assert a[0].dtype == b[0].dtype and a[0].shape == b[0].shape and (a[0] == b[0]).all()
    assert (a[1] == b[1]).all() and a[2].raw == b[2].raw and a[2].extensions == b[2].extensions


def test_foreign_and_own_files(ctx, tmp_path, monkeypatch):
    from boa_hip import nifti
    from boa_hip.synthetic import ct_phantom
    calls = []
    real = nifti.device_inflate
    monkeypatch.setattr(nifti, "device_inflate", lambda *a, **k: (lambda r: (calls.append(r[1]), r)[1])(real(*a, **k)))
    ref = os.path.join(GOLDEN, "ref_example_ct_sm.nii.gz")
    _same(nifti.load(ref, ctx=ctx), nifti.load(ref))
    assert len(calls) == 1 and not calls[0]["host"] and calls[0]["streams"] == 1
    ct = ct_phantom((48, 40, 56), seed=5)
    lab = (np.arange(ct.size).reshape(ct.shape) // 97 % 11).astype(np.uint8)
    aff = np.diag([-1.5, -1.5, 1.5, 1.0])
    for k, (vol, kw) in enumerate([(ct, {}), (lab, {}), (lab, {"ctx": ctx}), (lab, {"ctx": ctx, "dynamic": True}),
                                   (ct, {"ctx": ctx, "dynamic": True})]):
        path = tmp_path / f"v{k}.nii.gz"
        nifti.save(path, vol, aff, extensions=[(0, nifti.label_xml({1: "a"}))], **kw)
        del calls[:]
        got = nifti.load(path, ctx=ctx)
        _same(got, nifti.load(path))
        assert (got[0] == vol).all() and len(calls) == 1 and not calls[0]["host"] and calls[0]["streams"] >= 2, (k, calls)
    # a .nii file and a multi-member file without the index go to the host code
    nifti.save(tmp_path / "plain.nii", lab, aff)
    del calls[:]
    _same(nifti.load(tmp_path / "plain.nii", ctx=ctx), nifti.load(tmp_path / "plain.nii"))
    assert calls == []
    blob = nifti.read_bytes(tmp_path / "v1.nii.gz")
    (tmp_path / "two.nii.gz").write_bytes(gzip.compress(bytes(blob[:1000])) + gzip.compress(bytes(blob[1000:])))
    _same(nifti.load(tmp_path / "two.nii.gz", ctx=ctx), nifti.load(tmp_path / "v1.nii.gz"))
    assert len(calls) == 1 and calls[0]["host"] and calls[0]["status"] == ["trailing"]


@pytest.mark.parametrize("damage", ["flipped_byte", "cut_tail", "wrong_crc"])
def test_damaged_input(ctx, tmp_path, damage):
    """Error paths of a bounded decoder: a status per stream, and the loader raises what the host path raises."""
    from boa_hip import nifti
    from boa_hip.synthetic import ct_phantom
    blob = bytearray(352) + ct_phantom((32, 32, 16), seed=2).tobytes(order="F")
    raw = bytearray(gzip.compress(bytes(blob), 6))
    if damage == "flipped_byte":
        raw[len(raw) // 2] ^= 0x40
    elif damage == "cut_tail":
        del raw[len(raw) - 300:]
    else:
        raw[-8] ^= 1
    for chunk in CHUNKS:
        out, info = _inflate(ctx, bytes(raw), chunk)
        assert out is None and info["host"] and info["status"] != ["ok"] and len(info["status"]) == 1, (chunk, info)
    if damage == "wrong_crc":
        assert _inflate(ctx, bytes(raw), None)[1]["status"] == ["crc"]
    path = tmp_path / "bad.nii.gz"
    path.write_bytes(bytes(raw))
    with pytest.raises(Exception) as host:
        nifti.load(path)
    with pytest.raises(type(host.value)) as dev:
        nifti.load(path, ctx=ctx)
    assert str(dev.value) == str(host.value)


def test_drop_in_outputs_do_not_depend_on_the_load_switch(tmp_path, monkeypatch):
    """compute_all_models(["total"]) on a small phantom with and without BOA_LOAD_DEVICE=1: the same label volume and the same
    total-measurements.json, and the CT went through the device inflate exactly when asked to."""
    from boa_hip import label_maps, model_store, nifti, plans
    from boa_hip.compute.inference import compute_all_models
    from boa_hip.synthetic import ct_phantom
    root = tmp_path / "results"
    for tid, nc in zip(label_maps.PART_TASK_IDS, (25, 27, 19, 24, 27)):
        pj, dj = plans.synthetic_plans(patch=(32, 32, 32), features=(32, 64), num_classes=nc, spacing=(1.5, 1.5, 1.5))
        geom = plans.model_config_from_plans(pj, dj).geometry
        model_store.write_model_folder(str(root), tid, f"TotalSegmentator_part{tid - 290}", "nnUNetTrainerNoMirroring", pj, dj,
                                       [plans.synthetic_state_dict(geom, seed=tid)])
    monkeypatch.setenv("nnUNet_results", str(root))
    monkeypatch.delenv("BOA_SAVE_DEVICE", raising=False)
    ct = ct_phantom((48, 40, 56), seed=5)
    aff = np.diag([-1.5, -1.5, 1.5, 1.0])
    aff[:3, 3] = [30.0, 40.0, -100.0]
    ct_path = tmp_path / "ct.nii.gz"
    ct_path.write_bytes(gzip.compress(_nii_bytes(tmp_path, ct, aff), 6))       # a foreign, single-member file
    params = {"preview": False, "fast": False, "ml": True, "nr_thr_resamp": 1, "nr_thr_saving": 1, "quiet": True,
              "verbose": False, "device": "gpu", "license_number": None}
    calls = []
    real = nifti.device_inflate
    monkeypatch.setattr(nifti, "device_inflate", lambda *a, **k: (lambda r: (calls.append(r[1]["host"]), r)[1])(real(*a, **k)))
    counts = {}
    for switch in ("off", "on"):
        if switch == "on":
            monkeypatch.setenv("BOA_LOAD_DEVICE", "1")
        else:
            monkeypatch.delenv("BOA_LOAD_DEVICE", raising=False)
        del calls[:]
        compute_all_models(ct_path, tmp_path / switch, ["total"], params)
        counts[switch] = list(calls)
    assert counts["off"] == [] and len(counts["on"]) >= 2 and not any(counts["on"])      # compute_all_models and compute_measurements
    names = sorted(p.name for p in (tmp_path / "off").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "on").iterdir()) and {"total.nii.gz", "total-measurements.json"} <= set(names)
    for name in names:
        a, b = (tmp_path / "off" / name).read_bytes(), (tmp_path / "on" / name).read_bytes()
        if name.endswith(".nii.gz"):
            assert gzip.decompress(a) == gzip.decompress(b), name
        elif name.endswith(".json"):
            assert json.loads(a) == json.loads(b), name


def _nii_bytes(tmp_path, vol, aff):
    from boa_hip import nifti
    nifti.save(tmp_path / "plain_ct.nii", vol, aff)
    return (tmp_path / "plain_ct.nii").read_bytes()
