"""Irreversible (9/7) JPEG 2000 DICOM series decoded on the device (csrc/j2k.hip): the committed OpenJPEG fixtures of
tests/golden/j2k97 decoded to OpenJPEG's very pixels, alone and in one batch mixed with reversible frames, blocks cut at every
pass count against the numpy model, the clamp at both range ends, corrupted block data and invalid pass counts, get_image_info
on .91 series against the uncompressed series of OpenJPEG's pixels, a series mixing reversible and irreversible slices, and a
512 x 512 x 600 series (two chunks).  No Pillow here: only the committed fixtures are read."""
import dataclasses

import numpy as np
import pytest

import j2k97_fixtures as FX
import j2k97_reference as M
import j2k_writer as JW
from dicom_writer import write_series

pytestmark = pytest.mark.gpu
REVERSIBLE = ("129x97_u16_rpcl_precincts", "129x97_u8_7res", "40x33_u16_trunc_rpcl_cb4x4_3layers")
J_INVALID = 1                                     # include/boa_hip.h: BOA_J2K_INVALID


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.compute.inference import get_context
    return get_context("gpu")


@pytest.fixture(scope="module")
def fixtures():
    return FX.load_fixtures()


@pytest.fixture(scope="module")
def reversible():
    fx = {f["name"]: f for f in JW.load_fixtures()}
    return [fx[n] for n in REVERSIBLE]


def _by_name(fixtures, name):
    return next(f for f in fixtures if f["name"] == name)


def test_every_fixture_alone(ctx, fixtures):
    from boa_hip import jpeg2000 as J
    assert len(fixtures) == 10
    for fx in fixtures:
        fr = FX.parse(fx)
        assert fr.transform == 0
        px, st = J.decode_frames(ctx, [fr])
        assert st[0] == 0, fx["name"]
        np.testing.assert_array_equal(px[0], FX.expected(fx), err_msg=fx["name"])


def test_lossy_and_reversible_frames_in_one_call(ctx, fixtures, reversible):
    """Every 9/7 fixture and three 5/3 ones (7 resolutions; truncated by its layers) in one call, twice over in a shuffled order:
    both transforms, 0 .. 6 levels and sizes 2 x 2 .. 512 x 512 in one chunk."""
    from boa_hip import jpeg2000 as J
    every = [(f, FX.expected(f)) for f in fixtures] + [(f, JW.expected(f)) for f in reversible]
    order = np.random.default_rng(0).permutation(2 * len(every)) % len(every)
    frames = [J.parse_frame(every[i][0]["stream"], rows=every[i][0]["rows"], cols=every[i][0]["cols"],
                            name=f"{every[i][0]['name']}#{k}") for k, i in enumerate(order)]
    assert {f.transform for f in frames} == {0, 1} and {f.levels for f in frames} >= {0, 1, 2, 5, 6}
    px, st = J.decode_frames(ctx, frames)
    assert (st == 0).all(), st
    for i, got in zip(order, px):
        np.testing.assert_array_equal(got, every[i][1], err_msg=every[i][0]["name"])


@pytest.mark.parametrize("name", ["40x33_u8_lrcp_2layers", "40x33_s8_random"])
def test_every_pass_count_equals_the_model(ctx, fixtures, name):
    """One frame per P = 0 .. the most passes of a block, every block cut to its first min(P, own) passes, all in one call:
    the b_last rule under dequantisation, for every kind of last pass at every plane."""
    from boa_hip import jpeg2000 as J
    fr = FX.parse(_by_name(fixtures, name))
    own = fr.blocks[:, 6]
    frames = []
    for P in range(int(own.max()) + 1):
        b = fr.blocks.copy()
        b[:, 6] = np.minimum(P, own)
        frames.append(dataclasses.replace(fr, blocks=b, name=f"{name}#P{P}"))
    px, st = J.decode_frames(ctx, frames)
    assert (st == 0).all(), st
    want = [M.decode_frame(f) for f in frames]
    assert all(ok for _, ok in want)
    for P, (got, (w, _)) in enumerate(zip(px, want)):
        np.testing.assert_array_equal(got, w, err_msg=f"{name}: {P} passes")
    np.testing.assert_array_equal(px[-1], FX.expected(_by_name(fixtures, name)))
    assert len({w.tobytes() for w, _ in want}) > len(want) // 2         # (the cut frames really differ from one another)


def test_checkerboard_clamps_at_both_ends(ctx, fixtures):
    from boa_hip import jpeg2000 as J
    fx = _by_name(fixtures, "40x33_u16_checkerboard_rate20")
    fr = FX.parse(fx)
    plane, ok = M.reconstruct(fr)
    v = np.rint(plane) + 32768
    assert ok and v.min() < 0 and v.max() > 65535                       # the transform's output leaves the range at both ends
    px, st = J.decode_frames(ctx, [fr])
    assert st[0] == 0 and px[0].min() == 0 and px[0].max() == 65535
    np.testing.assert_array_equal(px[0], FX.expected(fx))


def test_corrupted_blocks_decode_without_a_fault_and_invalid_pass_counts_report(ctx, fixtures):
    from boa_hip import jpeg2000 as J
    from boa_hip.dicom import DicomError
    fx = _by_name(fixtures, "129x97_u16_ct_rate10_3res_cb16")
    good = FX.parse(fx, "good.dcm")
    noise = np.random.default_rng(1).integers(0, 256, len(good.data), dtype=np.uint8)
    garbage = dataclasses.replace(good, data=noise.tobytes(), name="garbage.dcm")
    b = good.blocks.copy()
    k = int(np.argmax(b[:, 6]))
    b[k, 6] = 3 * b[k, 5] - 1                                           # one pass beyond 3 x planes - 2
    over = dataclasses.replace(good, blocks=b, name="over.dcm")
    px, st = J.decode_frames(ctx, [good, garbage, over, good])
    assert list(st) == [0, 0, J_INVALID, 0], st
    np.testing.assert_array_equal(px[0], FX.expected(fx))
    np.testing.assert_array_equal(px[3], FX.expected(fx))
    np.testing.assert_array_equal(px[1], M.decode_frame(garbage)[0])    # garbage in, the model's garbage out
    with pytest.raises(DicomError, match="over.dcm"):
        J.decode(ctx, [good, over])
    px = J.decode(ctx, [good] * 3)                                      # the next batch decodes exactly
    np.testing.assert_array_equal(px, np.stack([FX.expected(fx)] * 3))


def test_host_entry_validates_transform_and_step(ctx, fixtures):
    from boa_hip import jpeg2000 as J
    fr = FX.parse(_by_name(fixtures, "40x33_u16_1res"))
    for steps in (np.array([np.nan], dtype=np.float32), np.array([0.0], dtype=np.float32), np.array([-1.0], dtype=np.float32),
                  np.array([np.inf], dtype=np.float32)):
        with pytest.raises(ValueError, match="boa_j2k_decode"):
            J.decode_frames(ctx, [dataclasses.replace(fr, steps=steps)])
    with pytest.raises(ValueError, match="boa_j2k_decode"):
        J.decode_frames(ctx, [dataclasses.replace(fr, transform=2)])
    px, st = J.decode_frames(ctx, [fr])
    assert st[0] == 0


@pytest.mark.parametrize("signed_pr", [False, True])
def test_get_image_info_lossy_series_equals_openjpeg_pixels(ctx, fixtures, tmp_path, signed_pr):
    """A .91 series of 9/7 streams reads as the uncompressed series that holds OpenJPEG's decoded pixels: the image and its HU,
    with unsigned and with signed PixelRepresentation (the same 16-bit patterns)."""
    from boa_hip import nifti
    from boa_hip.compute.io import get_image_info
    fxs = [_by_name(fixtures, n) for n in ("129x97_u16_ct_rate10_rpcl_precincts_cb32", "129x97_u16_ct_rate10_3res_cb16")]
    n = 12
    pats = [FX.expected(f) for f in fxs]
    stored = np.stack([(pats[z % 2].view(np.int16) if signed_pr else pats[z % 2]).astype(np.int64) for z in range(n)])
    kw = dict(signed=signed_pr, intercept=0 if signed_pr else -1024)
    write_series(tmp_path / "raw", stored, **kw)
    JW.write_series(tmp_path / "j2k", stored, [fxs[z % 2]["stream"] for z in range(n)], transfer_syntax=JW.J2K, **kw)
    p_raw, info_raw = get_image_info(tmp_path / "raw", tmp_path / "o_raw")
    p_j2k, info_j2k = get_image_info(tmp_path / "j2k", tmp_path / "o_j2k")
    d_raw, a_raw, _ = nifti.load(p_raw)
    d_j2k, a_j2k, _ = nifti.load(p_j2k)
    assert d_raw.dtype == d_j2k.dtype
    np.testing.assert_array_equal(d_j2k, d_raw)
    np.testing.assert_array_equal(a_j2k, a_raw)
    np.testing.assert_array_equal(d_raw.transpose(2, 1, 0), stored + (0 if signed_pr else -1024))
    assert info_raw == info_j2k


def test_series_mixing_reversible_and_irreversible_slices(ctx, fixtures, reversible, tmp_path):
    from boa_hip import dicom
    lossy = _by_name(fixtures, "129x97_u16_ct_rate10_3res_cb16")
    lossless = reversible[0]
    assert (lossless["rows"], lossless["cols"]) == (129, 97)
    pix = [lossy["decoded"], lossless["source"]]
    stored = np.stack([pix[z % 2] for z in range(10)])
    JW.write_series(tmp_path / "mix", stored, [(lossy, lossless)[z % 2]["stream"] for z in range(10)],
                    transfer_syntax=JW.J2K)
    data, geom, files = dicom.load_series(tmp_path / "mix", ctx=ctx)
    np.testing.assert_array_equal(data.transpose(2, 1, 0), stored - 1024)


def test_600_slice_series_in_two_chunks(ctx, fixtures):
    from boa_hip import jpeg2000 as J
    ph = [f for f in fixtures if f["name"].startswith("512x512_ct_phantom")]
    assert len(ph) == 2
    base = [FX.parse(f) for f in ph]
    frames = [base[z % 2] for z in range(600)]
    # the workspace of a chunk is capped at 1 GiB, 8 bytes per sample and the flag words: 600 frames do not fit one chunk
    assert 600 * 512 * 512 * 8 > 1 << 30
    px = J.decode(ctx, frames)
    assert px.shape == (600, 512, 512)
    for k in range(2):
        np.testing.assert_array_equal(px[k::2], np.broadcast_to(FX.expected(ph[k]), (300, 512, 512)))
