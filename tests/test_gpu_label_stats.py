"""boa_label_basic_stats / boa_label_apply_lut (csrc/label_stats.hip) and boa_hip/statistics.py against the numpy restatement of
tests/basic_statistics_reference.py (pinned to the reference's own get_basic_statistics by tests/test_basic_statistics_reference_cpu.py).
Integer work: table and dict are compared bit for bit; only the normalised mean, a float sum in the reference, has a tolerance (rtol
1e-12 on the unrounded value, one unit of the fifth decimal on the rounded one).

Launch geometry the shapes are chosen for (csrc/label_stats.hip): a lane reads 16 voxels, a workgroup of 256 lanes 4 096 per iteration,
the last n % 16 voxels are read one by one, up to 8 workgroups per CU: above 8 * CUs * 4 096 voxels (8.4 M on 256 CUs) a workgroup makes
more than one iteration; a wave hands at most 4 distinct labels per step to its leaders, the other lanes add their own runs."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import basic_statistics_cases as cases
import basic_statistics_reference as R

pytestmark = pytest.mark.gpu

WORDS = 770


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


def _table(ctx, seg, ct, border=3):
    """the raw words of boa_label_basic_stats through the C ABI"""
    from boa_hip._lib import check, int3
    seg = np.ascontiguousarray(seg, dtype=np.uint8)
    ct = np.ascontiguousarray(ct)
    code = {np.dtype(np.int16): 1, np.dtype(np.int32): 2}[ct.dtype]
    d_seg, d_ct, d_out = ctx.from_numpy(seg), ctx.from_numpy(ct), ctx.alloc(WORDS * 8)
    try:
        d_out.upload(np.full(WORDS, 0xA5A5A5A5A5A5A5A5, np.uint64))          # (the call overwrites the table)
        check(ctx.lib.boa_label_basic_stats(ctx.h, d_ct.vp, code, d_seg.vp, int3(seg.shape), border, d_out.vp), "boa_label_basic_stats")
        return d_out.download((WORDS,), np.uint64)
    finally:
        for b in (d_seg, d_ct, d_out):
            b.free()


def _assert_table(got, seg, ct, border=3):
    want = R.stats_table(seg, ct, border)
    for name, a, b in (("count", 0, 256), ("sum", 256, 512), ("touches", 512, 768), ("min/max", 768, 770)):
        g, w = got[a:b], want[a:b]
        if name == "touches":
            g = (g != 0).astype(np.uint64)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (name, bad[:8], g[bad[:8]].view(np.int64), w[bad[:8]].view(np.int64))


def _random_case(shape, seed, dtype=np.int16):
    rng = np.random.default_rng(seed)
    seg = rng.integers(0, 256, size=shape).astype(np.uint8)
    ct = rng.integers(-32768, 32768, size=shape).astype(dtype)
    if ct.size >= 8:
        ct.flat[1], ct.flat[ct.size // 2], ct.flat[-1], ct.flat[-2] = -32768, 32767, 32767, -32768
    return seg, ct


def _structured(shape, seed):
    """boxes of labels in a background of 0 (long runs per lane), HU noise"""
    rng = np.random.default_rng(seed)
    seg = np.zeros(shape, np.uint8)
    for v in range(1, 40):
        lo = [int(rng.integers(0, s - 2)) for s in shape]
        hi = [int(min(s, l + rng.integers(2, max(3, s // 3)))) for s, l in zip(shape, lo)]
        seg[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = v if v < 39 else 255
    return seg, rng.integers(-1024, 3072, size=shape).astype(np.int16)


@pytest.mark.parametrize("shape", [(5, 4, 5), (2, 9, 70), (37, 29, 67), (1, 1, 1), (1, 3, 15), (3, 3, 16), (16, 16, 16)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["i16", "i32"])
def test_random_labels_table(ctx, shape, dtype):
    """per-voxel uniform labels 0..255 (64 distinct labels in a wave) over the whole int16 range: (5, 4, 5) every axis shorter than 6 --
    everything touches; (2, 9, 70) an axis shorter than the border; (37, 29, 67) odd sizes, 18 workgroups, a tail of 5 voxels; volumes
    below 16 voxels are tail only"""
    seg, ct = _random_case(shape, 7, dtype)
    got = _table(ctx, seg, ct)
    _assert_table(got, seg, ct)
    if shape in ((5, 4, 5), (2, 9, 70)):
        assert ((got[512:768] != 0) == (got[:256] != 0)).all()           # every present label touches
    if shape == (37, 29, 67):
        assert got[0] > 0 and got[255] > 0 and (got[:256] > 0).all()      # labels 0 and 255 are rows of the table like any other
        assert got[768:].view(np.int64).tolist() == [-32768, 32767]


def test_int32_values_beyond_int16(ctx):
    seg, _ = _random_case((21, 17, 45), 3)
    ct = np.random.default_rng(4).integers(-2 ** 31, 2 ** 31, size=seg.shape).astype(np.int32)
    ct.flat[5], ct.flat[-7] = -2 ** 31, 2 ** 31 - 1
    _assert_table(_table(ctx, seg, ct), seg, ct)


@pytest.mark.parametrize("border", [0, 1, 3, 4])
def test_border_off_by_one(ctx, border):
    """twelve single-voxel labels at index 2 and at index 3 from each of the six faces: with border 3 exactly the six at index 2 touch"""
    shape = (11, 12, 19)
    seg = np.zeros(shape, np.uint8)
    v = 1
    expect = {}
    for ax in range(3):
        for depth in (2, 3):
            for pos in (depth, shape[ax] - 1 - depth):
                idx = [5, 6, 9]
                idx[ax] = pos
                seg[tuple(idx)] = v
                expect[v] = depth < border
                v += 1
    assert v == 13
    ct = np.random.default_rng(1).integers(-500, 500, size=shape).astype(np.int16)
    got = _table(ctx, seg, ct, border)
    _assert_table(got, seg, ct, border)
    assert {k: bool(got[512 + k]) for k in expect} == expect
    assert bool(got[512]) == (border > 0)


def test_sums_beyond_32_bits(ctx):
    """192^3: one label whose halves are 32767 and -32768, a second one at 32767 only: the sums pass 2^32 (2.1 M x 32 767 = 7e10 for the
    second; the first cancels to a small total through partial sums of 1e11) -- an int32 or a float32 accumulator gives neither"""
    shape = (192, 192, 192)
    seg = np.zeros(shape, np.uint8)
    ct = np.zeros(shape, np.int16)
    seg[:, :, :] = 9
    ct[:96], ct[96:] = 32767, -32768
    seg[40:150, 30:160, 20:170] = 200
    ct[40:150, 30:160, 20:170] = 32767
    got = _table(ctx, seg, ct)
    _assert_table(got, seg, ct)
    n200 = 110 * 130 * 150
    assert int(got[256 + 200].view(np.int64)) == n200 * 32767 > 2 ** 32 and int(got[200]) == n200
    assert not got[512 + 200] and got[512 + 9]


def test_structured_labels_several_iterations_per_workgroup(ctx):
    """9.06 M voxels with odd sizes: more than 8 workgroups per CU of 4 096 voxels, so a workgroup makes two iterations and a lane's
    open run carries from one into the next; boxes in a background of zeros"""
    shape = (131, 257, 269)
    seg, ct = _structured(shape, 11)
    got = _table(ctx, seg, ct)
    _assert_table(got, seg, ct)
    assert got[255] > 0 and got[0] > got[1:256].max()


def test_two_runs_give_identical_bytes(ctx):
    seg, ct = _random_case((37, 29, 67), 21)
    assert _table(ctx, seg, ct).tobytes() == _table(ctx, seg, ct).tobytes()
    seg, ct = _structured((60, 70, 83), 5)
    a = _table(ctx, seg, ct)
    assert a.tobytes() == _table(ctx, seg, ct).tobytes()
    _assert_table(a, seg, ct)


def test_argument_checks(ctx):
    from boa_hip._lib import BOA_EINVAL, int3
    d = ctx.alloc(4096)
    out = ctx.alloc(WORDS * 8)
    err = lambda: ctx.lib.boa_last_error().decode()
    try:
        assert ctx.lib.boa_label_basic_stats(ctx.h, d.vp, 0, d.vp, int3((4, 4, 4)), 3, out.vp) == BOA_EINVAL and "dtype" in err()
        assert ctx.lib.boa_label_basic_stats(ctx.h, d.vp, 1, d.vp, int3((4, -4, 4)), 3, out.vp) == BOA_EINVAL
        assert ctx.lib.boa_label_basic_stats(ctx.h, C.c_void_p(d.ptr + 2), 1, d.vp, int3((4, 4, 4)), 3, out.vp) == BOA_EINVAL and "aligned" in err()
        assert ctx.lib.boa_label_basic_stats(None, d.vp, 1, d.vp, int3((4, 4, 4)), 3, out.vp) == BOA_EINVAL
        # an empty volume: the table is still written
        assert ctx.lib.boa_label_basic_stats(ctx.h, d.vp, 1, d.vp, int3((0, 4, 4)), 3, out.vp) == 0
        t = out.download((WORDS,), np.uint64)
        assert not t[:768].any() and t[768:].view(np.int64).tolist() == [2 ** 63 - 1, -2 ** 63]
    finally:
        d.free()
        out.free()


# ---- boa_hip.statistics.basic_statistics ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "g17_basic_statistics.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("k", range(len(cases.CALLS)), ids=[cases.call_key(k) for k in range(len(cases.CALLS))])
def test_basic_statistics_dict(ctx, golden, k, tmp_path):
    """the dict and the json file of the calls of tests/basic_statistics_cases.py: the restatement and the reference's own output (G17)"""
    from boa_hip import label_maps, statistics as S
    name, kw = cases.CALLS[k]
    seg, ct, zooms = cases.volume(name)
    path = tmp_path / "statistics.json"
    got, raw = S.basic_statistics(ctx, seg, ct, zooms, task=cases.TASK, file_out=path, return_unrounded=True, **kw)
    cm = dict(sorted(label_maps.class_map(cases.TASK).items()))
    want = R.basic_statistics(seg, ct, zooms, cm, **kw)
    ref = golden["calls"][cases.call_key(k)]["stats"]
    assert list(got) == list(want) == [r[0] for r in ref]
    norm_mean = kw.get("normalized_intensities") and kw["metric"] == "mean"
    for (nme, vol, inten) in ref:
        g, w = got[nme], want[nme]
        assert float(w["volume"]) == vol and float(w["intensity"]) == inten
        assert isinstance(g["volume"], float) and float(g["volume"]) == vol, (nme, g, vol)
        if norm_mean:
            assert abs(float(g["intensity"]) - inten) <= 1.0000001e-5, (nme, g, inten)
        else:
            assert float(g["intensity"]) == inten, (nme, g, inten)
    if norm_mean:
        hu = np.asarray(ct).astype(np.int16)
        f = (hu - hu.min()) / (hu.max() - hu.min())
        inv = {n: i for i, n in cm.items()}
        assert raw
        for nme, v in raw.items():
            np.testing.assert_allclose(v, np.average(f, weights=(seg == inv[nme]).astype(np.uint8)), rtol=1e-12, atol=0)
    with open(path) as fh:
        text = fh.read()
    assert text == json.dumps(got, indent=4) and list(json.loads(text)) == list(got)


def test_basic_statistics_on_resident_int32_ct(ctx):
    """DevArrays in, the CT as the int32 model-grid image: no conversion copy for the mean, the same dict as from host arrays"""
    from boa_hip import statistics as S
    from boa_hip.devarray import DevArray
    seg, ct, zooms = cases.volume("blocks")
    d_seg, d_ct = DevArray.from_numpy(ctx, seg), DevArray.from_numpy(ctx, ct.astype(np.int32))
    try:
        for metric in ("mean", "median"):
            a = S.basic_statistics(ctx, d_seg, d_ct, zooms, metric=metric)
            b = S.basic_statistics(ctx, seg, ct, zooms, metric=metric)
            assert list(a) == list(b) and all(a[n] == b[n] for n in a)
    finally:
        d_seg.free()
        d_ct.free()


def test_basic_statistics_refuses_what_the_reference_cannot_cast(ctx):
    from boa_hip import statistics as S
    seg, ct, zooms = cases.volume("blocks")
    big = ct.astype(np.int32)
    big[0, 0, 0] = 40000
    with pytest.raises(ValueError, match="int16"):
        S.basic_statistics(ctx, seg, big, zooms)
    with pytest.raises(ValueError, match="int16"):
        S.basic_statistics(ctx, seg, big.astype(np.float64), zooms)
    s2, c2, z2 = cases.volume("extremes")
    with pytest.raises(ValueError, match="wraps"):
        S.basic_statistics(ctx, s2, c2, z2, normalized_intensities=True)
    with pytest.raises(ValueError, match="metric"):
        S.basic_statistics(ctx, seg, ct, zooms, metric="max")


# ---- boa_label_apply_lut -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,off_in,off_out", [(1, 0, 0), (15, 0, 0), (4099, 0, 0), (70001, 3, 3), (70001, 5, 6), (33, 15, 15), (20, 9, 9)])
def test_apply_lut(ctx, n, off_in, off_out):
    """`img *= isin(img, subset)` as a table: whole vectors, heads and tails, views that share or do not share their 16-byte alignment,
    and in place"""
    from boa_hip._lib import check
    rng = np.random.default_rng(n + off_in)
    a = rng.integers(0, 256, size=n + 32).astype(np.uint8)
    keep = rng.choice(np.arange(1, 256), size=9, replace=False)
    lut = np.zeros(256, np.uint8)
    lut[keep] = keep
    d_in, d_out = ctx.from_numpy(a), ctx.from_numpy(np.full(n + 48, 0xEE, np.uint8))
    try:
        check(ctx.lib.boa_label_apply_lut(ctx.h, C.c_void_p(d_in.ptr + off_in), n, lut.ctypes.data_as(C.c_void_p), C.c_void_p(d_out.ptr + off_out)))
        got = d_out.download((n + 48,), np.uint8)
        want = a[off_in:off_in + n] * np.isin(a[off_in:off_in + n], keep)
        np.testing.assert_array_equal(got[off_out:off_out + n], want)
        assert (got[:off_out] == 0xEE).all() and (got[off_out + n:] == 0xEE).all()          # nothing written outside
        check(ctx.lib.boa_label_apply_lut(ctx.h, C.c_void_p(d_in.ptr + off_in), n, lut.ctypes.data_as(C.c_void_p), C.c_void_p(d_in.ptr + off_in)))
        got = d_in.download((n + 32,), np.uint8)
        np.testing.assert_array_equal(got[off_in:off_in + n], want)
        np.testing.assert_array_equal(got[:off_in], a[:off_in])
        np.testing.assert_array_equal(got[off_in + n:], a[off_in + n:])
    finally:
        d_in.free()
        d_out.free()
