"""RLE Lossless (PS3.5 Annex G) DICOM series decoded on the device (csrc/rle.hip): libtiff's PackBits strips (tests/golden/rle),
every encoder style of tests/rle_writer.py at sizes around the chunk size, controls placed against chunk boundaries on purpose,
the parallel decoder at three chunk sizes against the serial one and the Python model, bit for bit; per-frame errors; and
get_image_info on RLE series against the uncompressed series of the same volume."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from dicom_writer import write_slice as write_native_slice
import rle_writer as R

pytestmark = pytest.mark.gpu
CHUNKS = (256, 1024, 4096)


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.compute.inference import get_context
    return get_context("gpu")


def _frame(data, shape, bits=16, name="frame"):
    from boa_hip import rle_lossless as RL
    return RL.parse_frame(data, rows=shape[0], cols=shape[1], bits_allocated=bits, name=name)


def _decode_all(ctx, frames, want_px, want_status):
    """The serial decoder and the parallel one at every chunk size: the expected status, and for the frames that decode the
    expected samples (the samples of a failed frame are unspecified)."""
    from boa_hip import rle_lossless as RL
    ok = np.asarray(want_status) == 0
    for kw in [dict(serial=True)] + [dict(chunk_bytes=cb) for cb in CHUNKS]:
        px, st = RL.decode_frames(ctx, frames, **kw)
        assert px.dtype == np.uint16 and px.shape == (len(frames), frames[0].rows, frames[0].cols)
        np.testing.assert_array_equal(st, want_status, err_msg=str(kw))
        for i in np.flatnonzero(ok):
            np.testing.assert_array_equal(px[i], want_px[i], err_msg=f"{kw} frame {i} ({frames[i].name})")


def _ct_like(shape, seed):
    rng = np.random.default_rng(seed)
    rows, cols = shape
    yy, xx = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    body = ((yy - rows / 2) ** 2 / max(rows * 0.4, 1) ** 2 + (xx - cols / 2) ** 2 / max(cols * 0.4, 1) ** 2) < 1
    return (np.where(body, 1064 + rng.integers(-200, 201, shape), 24)).astype(np.int64)


def test_golden_libtiff_strips(ctx):
    g = np.load(os.path.join(GOLDEN, "rle", "packbits_libtiff.npz"))
    for i in range(2):
        src = g[f"source_{i}"]
        strips = [g[f"strip_{i}_{k}"].tobytes() for k in range(2)]
        _decode_all(ctx, [_frame(R.frame_of(strips), src.shape, name=f"golden{i}")], [src], [0])
        # each plane alone, as an 8-bit frame
        for k in range(2):
            _decode_all(ctx, [_frame(R.frame_of(strips[k:k + 1]), src.shape, 8, name=f"golden{i}_{k}")],
                        [(src >> (8 - 8 * k)) & 0xFF], [0])


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (97, 129), (64, 200), (512, 512)])
def test_sizes_every_encoder_style(ctx, shape):
    """16-bit noise on a CT-like base and its low byte as an 8-bit image, every encoder style: parallel == serial == model."""
    x16 = _ct_like(shape, shape[0] * 7 + shape[1])
    for bits, x in ((16, x16), (8, x16 & 0xFF)):
        data = [R.encode_frame(x, bits, mode, k=700) for mode in R.MODES]
        if shape == (64, 200) and bits == 16:
            lit = R.segments_of(data[R.MODES.index("literal")])
            assert all(R.n_chunks(s, 1024) >= 12 and R.n_chunks(s, 256) >= 50 for s in lit)
        model = [R.decode_frame(d, *shape) for d in data]
        assert all(st == 0 and (px == x).all() for px, st in model)
        _decode_all(ctx, [_frame(d, shape, bits, name=m) for d, m in zip(data, R.MODES)], [px for px, _ in model], [0] * len(data))


@pytest.mark.parametrize("cb", [256, 1024])
def test_controls_against_chunk_boundaries(ctx, cb):
    """Streams built for chunks of `cb` bytes (rle_writer.boundary_cases), each an 8-bit frame of 1 x wanted samples, decoded
    at every chunk size; the properties the cases are named for are checked on the model first."""
    cases = R.boundary_cases(cb)
    tables = {n: [R.chunk_map(s, cb, k) for k in range(R.n_chunks(s, cb))] for n, (s, _) in cases.items()}
    chains = {n: R.chain(tables[n], cases[n][1]) for n in cases}
    assert cases["c127_on_last_byte"][0][cb - 1] == 127 and chains["c127_on_last_byte"][1][1] == 128
    assert cases["repeat_on_last_byte"][0][cb - 1] > 128 and chains["repeat_on_last_byte"][1][1] == 1
    assert len(cases["ends_on_boundary"][0]) == 2 * cb and len(tables["ends_on_boundary"]) == 2
    assert b"\x80" * 600 in cases["noop_flood"][0] and any(t[0] & R.T_COUNT_MASK == 0 for t in tables["noop_flood"])
    assert set(cases["dense"][0][0::2]) == {0, 255}
    seg, wanted = cases["last_run_clipped"]
    assert seg[-2] == 129 and len(R.decode_segment(seg[:-2], wanted)[0]) == wanted - 5
    for name, (seg, wanted) in cases.items():
        out, st = R.decode_segment(seg, wanted)
        assert st == int(name in ("cut_short", "operand_overrun", "repeat_without_operand", "empty_after_header")), name
        want = np.frombuffer(out + bytes(wanted - len(out)), dtype=np.uint8).reshape(1, wanted)
        _decode_all(ctx, [_frame(R.frame_of([seg]), (1, wanted), 8, name=name)], [want], [st])


def test_one_batch_of_unlike_frames_keeps_order(ctx):
    """Constant, CT-like and noise frames, 16-bit frames and frames of one plane in one batch (also decoded in groups of frames
    under a small workspace cap); a table that points outside the data is refused before anything is launched."""
    from boa_hip import rle_lossless as RL
    shape = (64, 80)
    rng = np.random.default_rng(4)
    imgs = [np.full(shape, 1024), _ct_like(shape, 1), rng.integers(0, 1 << 16, shape), _ct_like(shape, 2) & 0xFF,
            np.zeros(shape, dtype=np.int64), rng.integers(0, 256, shape), _ct_like(shape, 3)]
    bits = [16, 16, 16, 8, 16, 8, 16]
    modes = ["rows", "crossing", "literal", "rows", "dense", "noops", "rows"]
    frames = [_frame(R.encode_frame(x, b, m, k=300), shape, b, name=f"f{i}") for i, (x, b, m) in enumerate(zip(imgs, bits, modes))]
    sizes = [len(f.data) for f in frames]
    assert max(sizes) > 8 * min(sizes)
    _decode_all(ctx, frames, imgs, [0] * len(frames))
    os.environ["BOA_RLE_WS_MB"] = "1"                   # 7 frames of 2 x 5 KiB planes and their tables: several groups of frames
    try:
        many = frames * 40
        _decode_all(ctx, many, imgs * 40, [0] * len(many))
    finally:
        del os.environ["BOA_RLE_WS_MB"]
    data, ftab = RL.build_batch(frames)
    for f, word, value in ((2, 2, len(data)), (0, 0, len(data) - 10), (3, 5, sizes[3] + 1), (1, 4, -1), (1, 6, ftab[1, 7] + 1),
                           (4, 3, 3), (4, 3, 0)):
        bad = ftab.copy()
        bad[f, word] = value
        for serial in (False, True):
            with pytest.raises(ValueError, match="boa_rle_decode: frame"):
                RL._decode_tables(ctx, data, bad, *shape, serial=serial)
    with pytest.raises(ValueError, match="chunk_bytes"):
        RL.decode_frames(ctx, frames, chunk_bytes=128)
    with pytest.raises(ValueError, match="chunk_bytes"):
        RL.decode_frames(ctx, frames, chunk_bytes=768)
    _decode_all(ctx, frames, imgs, [0] * len(frames))


def test_malformed_frames_report_and_next_batch_decodes(ctx):
    from boa_hip import rle_lossless as RL
    from boa_hip.dicom import DicomError
    shape = (48, 50)
    x = _ct_like(shape, 8)
    hi, lo = [R.encode_segment(p, "rows") for p in R.planes_of(x, 16)]
    lit = R.encode_segment(R.planes_of(x, 16)[1], "literal")
    overrun = lit[:129 * 9] + bytes([100]) + lit[129 * 9 + 1:129 * 9 + 30]         # a literal control whose operands pass the end
    data = [("good.dcm", R.frame_of([hi, lo])), ("cut_low.dcm", R.frame_of([hi, lo[:len(lo) // 2]])),
            ("good2.dcm", R.frame_of([hi, lit])), ("overrun.dcm", R.frame_of([hi, overrun])),
            ("cut_high.dcm", R.frame_of([hi[:len(hi) // 3], lo]))]
    frames = [_frame(d, shape, name=n) for n, d in data]
    model = [R.decode_frame(d, *shape) for _, d in data]
    assert [st for _, st in model] == [0, 1, 0, 1, 1]
    _decode_all(ctx, frames, [x] * 5, [0, 1, 0, 1, 1])
    for kw in (dict(serial=True), dict(), dict(chunk_bytes=256)):
        for bad in (frames[1], frames[3], frames[4]):
            with pytest.raises(DicomError, match=f"{bad.name}: RLE Lossless decode failed: segment truncated"):
                RL.decode(ctx, [frames[0], bad, frames[2]], **kw)
        np.testing.assert_array_equal(RL.decode(ctx, [frames[0], frames[2], frames[0]], **kw), np.stack([x] * 3).astype(np.uint16))


def _ct_volume(n=12, rows=40, cols=48, seed=0):
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(np.arange(n), np.arange(rows), np.arange(cols), indexing="ij")
    body = ((yy - rows / 2) ** 2 / (rows * 0.4) ** 2 + (xx - cols / 2) ** 2 / (cols * 0.4) ** 2) < 1
    hu = np.where(body, 40 + 10 * np.sin(zz / 3.0), -1000) + rng.normal(0, 15, body.shape)
    return np.clip(np.round(hu), -1024, 3071).astype(np.int64)


@pytest.mark.parametrize("signed,alloc,stored", [(False, 16, 16), (True, 16, 12), (False, 8, 8)])
def test_get_image_info_rle_equals_uncompressed(ctx, tmp_path, signed, alloc, stored):
    from boa_hip import nifti
    from boa_hip.compute.io import get_image_info
    hu = _ct_volume(seed=alloc + stored)
    if alloc == 8:
        values = (hu + 1024) >> 4                   # 0 .. 255, slope 1 intercept 0
        kw = dict(signed=False, intercept=0, bits_stored=8)
    else:
        values = np.clip(hu, -1024, 2047) if signed else hu + 1024
        kw = dict(signed=signed, intercept=0 if signed else -1024, bits_stored=stored)
    R.write_series(tmp_path / "raw", values, compressed=False, bits_allocated=alloc, **kw)
    R.write_series(tmp_path / "rle", values, bits_allocated=alloc, **kw)
    p_raw, info_raw = get_image_info(tmp_path / "raw", tmp_path / "o_raw")
    p_rle, info_rle = get_image_info(tmp_path / "rle", tmp_path / "o_rle")
    d_raw, a_raw, _ = nifti.load(p_raw)
    d_rle, a_rle, _ = nifti.load(p_rle)
    assert d_raw.dtype == d_rle.dtype
    np.testing.assert_array_equal(d_rle, d_raw)
    np.testing.assert_array_equal(a_rle, a_raw)
    np.testing.assert_array_equal(d_raw.transpose(2, 1, 0), values + kw["intercept"])
    assert info_raw == info_rle


def test_load_series_mixed_rle_and_native(ctx, tmp_path):
    """RLE slices in one to three fragments, with and without an offset table, in every encoder style, beside native slices."""
    from boa_hip import dicom
    hu = _ct_volume(n=10, seed=9) + 1024
    os.makedirs(tmp_path / "mix")
    for z in range(10):
        p = str(tmp_path / "mix" / f"IM{z:04d}.dcm")
        ipp = (-100.0, -120.0, 50.0 + 1.5 * z)
        if z % 4 == 3:
            write_native_slice(p, hu[z], ipp=ipp, instance=z + 1)
        else:
            R.write_slice(p, hu[z], mode=R.MODES[z % len(R.MODES)], ipp=ipp, instance=z + 1, fragments=1 + z % 3, bot=bool(z % 2))
    data, geom, files = dicom.load_series(tmp_path / "mix", ctx=ctx)
    np.testing.assert_array_equal(data.transpose(2, 1, 0), hu - 1024)
