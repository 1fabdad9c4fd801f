"""Bin-exact stress tests of the integer voxel statistics kernels through the C ABI: boa_label_hu_histogram (every bin of the
[256, nbins] table in every case), boa_tissue_aggregate (every int16 HU x every region byte), boa_tissue_projections,
boa_median3_inplane (0-1 principle), boa_slice_label_presence, boa_label_hu_mask, boa_label_select -- each against the plain
numpy statement of the operation in tests/voxel_stats_reference.py (itself pinned by test_voxel_stats_reference_cpu.py).
All comparisons are exact integer equality; no case is sampled.

What the cases are for, checked once with deliberately wrong (in-bounds) kernels on an MI355X -- each turned these tests red:
  the global fallback after 16 probes dropping its count  -> table_exactly_full (1 368 bins short by 1), around_the_flush_threshold,
                                                             many_flushes, views_at_every_voxel_offset, clamps_and_key_extremes
  bin_of clamping the top to nbins - 2                    -> clamps_and_key_extremes, sizes, views_at_every_voxel_offset, two_calls
  `r < 255` -> `r <= 255` in the projections              -> every test_tissue_projections case and the LDS-bound case (silhouettes)
  one exchange of the median network removed              -> median3_zero_one_principle (31 of the 512 windows), short_axes_and_full_range
  `hu[j]` -> `hr[j]` in the tissue sums                   -> tissue_rules_from_a_second_volume, tissue_sums_at_the_int16_extremes
The flush race fixed alongside (a wave flushing alone) is a timing window: the unfixed kernel passes all of this file too; the tests
pin the table logic around the threshold, the barrier in k_label_hist closes the window."""
import ctypes as C

import numpy as np
import pytest

import voxel_stats_reference as R

pytestmark = pytest.mark.gpu

# ---- launch geometry of k_label_hist: csrc/agg.hip, `constexpr int LOG2 = 14, HT = 1024` in boa_label_hu_histogram and
# HIST_FLUSH / the 16-probe limit in k_label_hist.  A retune of the table is a one-line change here. ----------------------
HIST_LOG2 = 14                      # 2^LOG2 {key, count} slots in LDS
HIST_THREADS = 1024                 # HT: threads per workgroup
LANE_VOX = 16                       # voxels a thread takes per iteration
WAVE = 64
HIST_SLOTS = 1 << HIST_LOG2
ITER_VOX = HIST_THREADS * LANE_VOX  # voxels one workgroup counts between two flush decisions
WAVE_VOX = WAVE * LANE_VOX


def flush_threshold(log2):
    """a workgroup flushes its table after an iteration that leaves more than this many distinct keys in it"""
    return (1 << log2) * 2 // 3


HIST_FLUSH = flush_threshold(HIST_LOG2)


def iters_per_workgroup(n, cu_count):
    """groups_per_block of boa_label_hu_histogram for an aligned volume of n voxels"""
    iters = (n // LANE_VOX + HIST_THREADS - 1) // HIST_THREADS
    return max(1, (iters + cu_count - 1) // cu_count)


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cu_count(ctx):
    return int(ctx.info()["cu_count"])


def _view(ctx, arr, offset, pad_value, pad=48):
    """`arr` on the device as a BufferView that starts `offset` elements into an allocation filled with `pad_value` around it"""
    from boa_hip.device import BufferView
    arr = np.ascontiguousarray(arr).ravel()
    host = np.full(arr.size + pad, pad_value, dtype=arr.dtype)
    host[offset:offset + arr.size] = arr
    buf = ctx.from_numpy(host)
    assert buf.ptr % 16 == 0, "allocations are expected to be 16-byte aligned (the offsets below are relative to that)"
    return BufferView(buf, offset * arr.itemsize, arr.size * arr.itemsize), buf


def _run_hist(ctx, d_ct, d_lab, d_mask, n, hu_min, nbins, d_hist=None):
    from boa_hip._lib import check
    own = d_hist is None
    if own:
        d_hist = ctx.alloc(256 * nbins * 4)
    check(ctx.lib.boa_memset(ctx.h, d_hist.vp, 0xA5, 256 * nbins * 4))      # the call itself must clear the table
    check(ctx.lib.boa_label_hu_histogram(ctx.h, d_ct.vp, d_lab.vp, d_mask.vp if d_mask is not None else None, n, hu_min, nbins,
                                         d_hist.vp), "boa_label_hu_histogram")
    h = d_hist.download((256, nbins), np.uint32)
    if own:
        d_hist.free()
    return h


def _check_hist(ctx, ct, lab, mask, hu_min, nbins, offsets=(0, 0, 0), what=""):
    """one call on views at the given element offsets (labels, ct, mask) of their allocations; every bin compared"""
    ct = np.ascontiguousarray(ct, dtype=np.int16).ravel()
    lab = np.ascontiguousarray(lab, dtype=np.uint8).ravel()
    n = ct.size
    assert lab.size == n and (mask is None or mask.size == n)
    # (the padding around the views carries measurable voxels: reading outside [0, n) changes the table)
    v_lab, b_lab = _view(ctx, lab, offsets[0], 9)
    v_ct, b_ct = _view(ctx, ct, offsets[1], 77)
    v_m, b_m = _view(ctx, np.ascontiguousarray(mask, dtype=np.uint8), offsets[2], 1) if mask is not None else (None, None)
    got = _run_hist(ctx, v_ct, v_lab, v_m, n, hu_min, nbins)
    for b in (b_lab, b_ct, b_m):
        if b is not None:
            b.free()
    want = R.label_hu_histogram(ct, lab, mask, hu_min, nbins)
    np.testing.assert_array_equal(got, want, err_msg=f"{what} n={n} hu_min={hu_min} nbins={nbins} offsets={offsets}")
    return got


FULL = (-32768, 65536)      # hu_min, nbins: the key is (label, HU) itself, no clamp


# ---- the LDS table -----------------------------------------------------------------------------------------------------
def test_hist_table_exactly_full_past_the_probe_limit(ctx):
    """One workgroup, one iteration, as many distinct keys as the table has slots: probe chains grow past the 16-probe limit and
    the global fallback carries real counts (at load factor 1 the expected probe length of linear probing is unbounded).  Then
    every key 2..5 times at scattered positions (several workgroups, each with a table near full, the same keys meeting in the
    global table)."""
    assert ITER_VOX >= HIST_SLOTS
    rng = np.random.default_rng(100)
    ids = R.distinct_ids(rng, ITER_VOX, FULL[1])
    ct, lab = R.keys_to_voxels(ids, *FULL)
    assert lab.min() >= 1 and ct.min() < -30000 and ct.max() > 30000 and len(set(lab)) == 255
    h = _check_hist(ctx, ct, lab, None, *FULL, what="full table")
    assert int(h.sum()) == ITER_VOX and int(h.max()) == 1
    vol, reps = R.repeated_keys_volume(rng, ids, 2, 5)
    ct, lab = R.keys_to_voxels(vol, *FULL)
    h = _check_hist(ctx, ct, lab, None, *FULL, what="full table, repeated keys")
    assert int(h.max()) == 5 and int((h > 0).sum()) == ITER_VOX


@pytest.mark.parametrize("delta", [-1, 0, 1, 2])
@pytest.mark.parametrize("log2", [12, 13, 14])
def test_hist_around_the_flush_threshold(ctx, cu_count, log2, delta):
    """Every workgroup's range holds exactly flush_threshold(log2) + delta distinct keys after its first iteration and 4 000 new
    keys in each of the two following ones: at the threshold of the table in use the first flush happens (delta > 0) or not,
    the table is refilled, flushed by the second iteration, and the final flush carries the remainder.  The thresholds of the
    smaller tables are pinned too in case the default moves."""
    k_first, k_next, gpb = flush_threshold(log2) + delta, 4000, 3
    assert k_first <= ITER_VOX
    rng = np.random.default_rng(200 + 10 * log2 + delta)
    nbins, hu_min = 2048, -1024
    ids = R.threshold_volume(rng, cu_count, gpb, ITER_VOX, k_first, k_next, nbins)
    assert iters_per_workgroup(ids.size, cu_count) == gpb
    for w in (0, cu_count - 1):                                             # the stated property, on the first and last range
        a = w * gpb * ITER_VOX
        assert np.unique(ids[a:a + ITER_VOX]).size == k_first
        assert np.unique(ids[a:a + 2 * ITER_VOX]).size == k_first + k_next
    ct, lab = R.keys_to_voxels(ids, hu_min, nbins)
    _check_hist(ctx, ct, lab, None, hu_min, nbins, what=f"threshold 2^{log2} {delta:+d}")


def test_hist_many_flushes_per_workgroup(ctx, cu_count):
    """labels uniform in 0..255, HU uniform over all of int16: ~16 000 distinct keys per iteration, every iteration of every
    workgroup overflows the threshold; three iterations per workgroup and a 5-voxel tail"""
    n = cu_count * ITER_VOX * 3 + 5
    assert iters_per_workgroup(n, cu_count) >= 3
    rng = np.random.default_rng(300)
    ct = rng.integers(-32768, 32768, size=n).astype(np.int16)
    lab = rng.integers(0, 256, size=n).astype(np.uint8)
    assert np.unique(R.keys_of(ct[:ITER_VOX], lab[:ITER_VOX], *FULL)).size > HIST_FLUSH
    _check_hist(ctx, ct, lab, None, *FULL, what="many flushes")


# ---- the wave-uniform shortcut -----------------------------------------------------------------------------------------
SMALL = (-256, 512)


def test_hist_uniform_waves(ctx):
    n = 2 * ITER_VOX + 3 * WAVE_VOX
    ct = np.full(n, 100, np.int16)
    lab = np.full(n, 3, np.uint8)
    h = _check_hist(ctx, ct, lab, None, *SMALL, what="one key")
    assert h[3, 100 - SMALL[0]] == n
    _check_hist(ctx, ct, np.zeros(n, np.uint8), None, *SMALL, what="all label 0")
    _check_hist(ctx, ct, lab, np.zeros(n, np.uint8), *SMALL, what="all masked out")
    _check_hist(ctx, ct, lab, np.full(n, 255, np.uint8), *SMALL, what="all masked in")
    # the last wave lies partly beyond n / 16: 10 live lanes (uniform count = 16 x 10), then a 7-voxel tail
    m = 3 * WAVE_VOX + 10 * LANE_VOX + 7
    _check_hist(ctx, ct[:m], lab[:m], None, *SMALL, what="partial last wave")
    _check_hist(ctx, ct[:m], lab[:m], np.ones(m, np.uint8), *SMALL, what="partial last wave, mask")


@pytest.mark.parametrize("kind", ["hu", "label", "label0", "masked"])
@pytest.mark.parametrize("pos", [0, LANE_VOX - 1, (WAVE - 1) * LANE_VOX, WAVE_VOX - 1], ids=["lane0_first", "lane0_last", "lane63_first", "lane63_last"])
def test_hist_one_odd_voxel_in_a_uniform_wave(ctx, pos, kind):
    """the odd voxel differs in HU, in label, is background, or is masked out; it sits in wave 1 of 4, and once more in the last
    wave"""
    n = 4 * WAVE_VOX
    for wave in (1, 3):
        ct = np.full(n, -7, np.int16)
        lab = np.full(n, 200, np.uint8)
        mask = np.full(n, 1, np.uint8) if kind == "masked" else None
        i = wave * WAVE_VOX + pos
        if kind == "hu":
            ct[i] = -8
        elif kind == "label":
            lab[i] = 201
        elif kind == "label0":
            lab[i] = 0
        else:
            mask[i] = 0
        _check_hist(ctx, ct, lab, mask, *SMALL, what=f"odd voxel {kind} at {i}")


def test_hist_alternating_uniform_and_mixed_waves(ctx):
    rng = np.random.default_rng(400)
    n = 2 * ITER_VOX
    ct = rng.integers(-300, 300, size=n).astype(np.int16)                  # (clamps at both ends of SMALL)
    lab = rng.integers(0, 4, size=n).astype(np.uint8)
    for w in range(0, n // WAVE_VOX, 2):
        ct[w * WAVE_VOX:(w + 1) * WAVE_VOX] = 5 + w
        lab[w * WAVE_VOX:(w + 1) * WAVE_VOX] = (w // 2) % 3                # (every third uniform wave is background)
    _check_hist(ctx, ct, lab, None, *SMALL, what="alternating waves")


# ---- run folding -------------------------------------------------------------------------------------------------------
def test_hist_run_folding(ctx):
    """Runs of equal keys inside a lane's 16 voxels, every length at every offset, between distinct keys, between background
    voxels and between both; runs that straddle two lanes (they must NOT be merged across the lane: each lane folds its own
    part)."""
    nbins, hu_min = 512, -256
    run = 5 * nbins + 300                                                   # label 6, bin 300
    others = [1 * nbins + 10, 2 * nbins + 20, 3 * nbins + 30]
    parts = [R.run_lanes(run, others), R.run_lanes(run, [-1]), R.run_lanes(run, [-1, -1, others[0], -1])]
    assert all(p.shape == (136, LANE_VOX) for p in parts)
    straddle = []
    for s in range(1, LANE_VOX):
        for L in range(2, 2 * LANE_VOX + 1):
            row = np.array([others[j % 3] for j in range(3 * LANE_VOX)], np.int64)
            row[LANE_VOX - s:LANE_VOX - s + L] = run
            straddle.append(row)
    ids = np.concatenate([p.ravel() for p in parts] + straddle)
    assert ids.size % LANE_VOX == 0
    ct, lab = R.keys_to_voxels(ids, hu_min, nbins)
    _check_hist(ctx, ct, lab, None, hu_min, nbins, what="runs")
    _check_hist(ctx, ct, lab, (np.arange(ids.size) % 5 != 0).astype(np.uint8) * 3, hu_min, nbins, what="runs cut by the mask")


# ---- sizes, alignment --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, ITER_VOX - 1, ITER_VOX, ITER_VOX + 1])
def test_hist_sizes(ctx, n):
    rng = np.random.default_rng(500 + n)
    ct = rng.integers(-32768, 32768, size=n).astype(np.int16)
    lab = rng.integers(0, 256, size=n).astype(np.uint8)
    mask = rng.integers(0, 2, size=n).astype(np.uint8)
    _check_hist(ctx, ct, lab, None, -1024, 2048, what="size")
    _check_hist(ctx, ct, lab, mask, -1024, 2048, what="size, mask")


@pytest.mark.parametrize("off", range(16))
def test_hist_views_at_every_voxel_offset(ctx, off):
    """Views that start `off` voxels into their allocations.  The same offset for all three arrays (and ct 8 voxels = 16 bytes
    further) can be aligned together: vector kernel with head = (16 - off) % 16 voxels one by one.  Differing offsets: the scalar
    kernel.  n leaves a non-empty head (off != 0) and a 9-voxel tail."""
    rng = np.random.default_rng(600 + off)
    head = (16 - off) % 16
    n = head + ITER_VOX + 7 * LANE_VOX + 9
    ct = rng.integers(-1200, 1200, size=n).astype(np.int16)
    lab = rng.integers(0, 256, size=n).astype(np.uint8)
    mask = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=n)
    for m in (None, mask):
        _check_hist(ctx, ct, lab, m, -1024, 2048, offsets=(off, off, off), what="aligned together")
        _check_hist(ctx, ct, lab, m, -1024, 2048, offsets=(off, off + 8, off), what="aligned together, ct 16 bytes on")
        _check_hist(ctx, ct, lab, m, -1024, 2048, offsets=(off, off + 1, off), what="ct apart")
        _check_hist(ctx, ct, lab, m, -1024, 2048, offsets=(off, (off + 13) % 16, (off + 3) % 16), what="all apart")
    _check_hist(ctx, ct, lab, mask, -1024, 2048, offsets=(off, off, (off + 5) % 16), what="mask apart")
    # fewer voxels than the head
    for k in (1, max(1, head - 1), head + 1):
        _check_hist(ctx, ct[:k], lab[:k], mask[:k], -1024, 2048, offsets=(off, off, off), what="shorter than the head")


# ---- clamps, key extremes, masks ---------------------------------------------------------------------------------------
def test_hist_clamps_and_key_extremes(ctx):
    rng = np.random.default_rng(700)
    n = 3 * ITER_VOX + 11
    ct = rng.integers(-32768, 32768, size=n).astype(np.int16)
    ct[::7] = rng.integers(-152, 152, size=ct[::7].size)                     # (and plenty of voxels around both edges)
    lab = rng.integers(0, 256, size=n).astype(np.uint8)
    h = _check_hist(ctx, ct, lab, None, -150, 300, what="clamps")
    assert h[:, 0].sum() > n // 3 and h[:, 299].sum() > n // 3                # below -> bin 0, above -> bin 299
    h = _check_hist(ctx, ct, lab, None, 0, 1, what="nbins = 1")
    np.testing.assert_array_equal(h[:, 0], np.concatenate([[0], np.bincount(lab, minlength=256)[1:]]))
    for hu_min in (-32768, 32767, 40000, -40000):
        _check_hist(ctx, ct[:ITER_VOX + 5], lab[:ITER_VOX + 5], None, hu_min, 2, what="nbins = 2")
    # the ends of the key space: (label 1, HU -32768) = key 0x00010000, (label 255, HU 32767) = key 0x00FFFFFF next to the
    # table's empty marker; between random voxels, in uniform waves, and alone
    ct[5], lab[5] = -32768, 1
    ct[6], lab[6] = 32767, 255
    ct[ITER_VOX + 100:ITER_VOX + 200], lab[ITER_VOX + 100:ITER_VOX + 200] = 32767, 255
    ct[2 * WAVE_VOX:3 * WAVE_VOX], lab[2 * WAVE_VOX:3 * WAVE_VOX] = 32767, 255
    ct[4 * WAVE_VOX:5 * WAVE_VOX], lab[4 * WAVE_VOX:5 * WAVE_VOX] = -32768, 255
    h = _check_hist(ctx, ct, lab, None, *FULL, what="key extremes")
    assert h[255, 65535] >= WAVE_VOX + 101 and h[1, 0] >= 1 and h[255, 0] >= WAVE_VOX
    h = _check_hist(ctx, np.array([32767, -32768], np.int16), np.array([255, 255], np.uint8), None, *FULL, what="two voxels")
    assert h[255, 65535] == 1 and h[255, 0] == 1 and h.sum() == 2


def test_hist_count_above_2_to_16_in_one_bin(ctx):
    """one key 70 000 times among random voxels (mixed waves: LDS adds and flushes) and 5 x 16 384 times in uniform waves"""
    rng = np.random.default_rng(800)
    n = 12 * ITER_VOX
    ct = rng.integers(-1000, 1000, size=n).astype(np.int16)
    lab = rng.integers(0, 256, size=n).astype(np.uint8)
    at = rng.choice(7 * ITER_VOX, size=70000, replace=False)
    ct[at], lab[at] = 321, 42
    ct[7 * ITER_VOX:], lab[7 * ITER_VOX:] = 321, 42
    h = _check_hist(ctx, ct, lab, None, -1024, 2048, what="large count")
    assert h[42, 321 + 1024] >= 70000 + 5 * ITER_VOX > 1 << 16


def test_hist_mask_bytes_and_mask_as_labels(ctx):
    rng = np.random.default_rng(900)
    n = 2 * ITER_VOX + 37
    ct = rng.integers(-500, 500, size=n).astype(np.int16)
    lab = rng.integers(0, 256, size=n).astype(np.uint8)
    mask = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=n)
    h = _check_hist(ctx, ct, lab, mask, -1024, 2048, what="mask bytes")
    assert int(h.sum()) == int(((mask != 0) & (lab != 0)).sum())
    m01 = (rng.random(n) < 0.6).astype(np.uint8)                             # _masked_stats: the 0 / 1 mask IS the label volume
    h = _check_hist(ctx, ct, m01, None, *FULL, what="mask as labels")
    assert int(h[1].sum()) == int(m01.sum()) and int(h.sum()) == int(m01.sum())


def test_hist_two_calls_into_the_same_table(ctx):
    rng = np.random.default_rng(1000)
    n = 3 * ITER_VOX + 1
    ct = rng.integers(-32768, 32768, size=n).astype(np.int16)
    lab = rng.integers(0, 256, size=n).astype(np.uint8)
    d_ct, d_lab = ctx.from_numpy(ct), ctx.from_numpy(lab)
    d_hist = ctx.alloc(256 * 2048 * 4)
    a = _run_hist(ctx, d_ct, d_lab, None, n, -1024, 2048, d_hist).copy()
    from boa_hip._lib import check
    check(ctx.lib.boa_label_hu_histogram(ctx.h, d_ct.vp, d_lab.vp, None, n, -1024, 2048, d_hist.vp))   # (no clearing in between)
    b = d_hist.download((256, 2048), np.uint32)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, R.label_hu_histogram(ct, lab, None, -1024, 2048))
    check(ctx.lib.boa_label_hu_histogram(ctx.h, d_ct.vp, d_lab.vp, None, 0, -1024, 2048, d_hist.vp))   # n = 0 still clears
    assert int(d_hist.download((256, 2048), np.uint32).sum()) == 0
    for x in (d_ct, d_lab, d_hist):
        x.free()


# ---- boa_tissue_aggregate ----------------------------------------------------------------------------------------------
def _run_aggregate(ctx, v_ct, v_rules, v_reg, v_parts, v_tis, Z, Y, X):
    from boa_hip._lib import check
    cnt, sums = ctx.alloc(Z * 16 * 4), ctx.alloc(Z * 16 * 8)
    check(ctx.lib.boa_memset(ctx.h, cnt.vp, 0x5A, Z * 16 * 4))
    check(ctx.lib.boa_memset(ctx.h, sums.vp, 0x5A, Z * 16 * 8))
    check(ctx.lib.boa_tissue_aggregate(ctx.h, v_ct.vp, v_rules.vp if v_rules is not None else None, v_reg.vp,
                                       v_parts.vp if v_parts is not None else None, v_tis.vp if v_tis is not None else None,
                                       Z, Y, X, cnt.vp, sums.vp), "boa_tissue_aggregate")
    c, s = cnt.download((Z, 2, 8), np.uint32), sums.download((Z, 2, 8), np.int64)
    cnt.free()
    sums.free()
    return c, s


def _check_aggregate(ctx, ct, rules, regions, parts, Y, X, offsets=(0, 0, 0, 0, 0), want_tissues=True, max_z=65535, what=""):
    """The flat voxel sequences cut into (Z, Y, X) volumes (wrapped round at the end so that no voxel is left out; several calls
    where Z would exceed the grid's 65 535 slices), read through views at the given element offsets (ct, ct_rules, regions,
    parts, tissues) of their allocations.  Tissue map, counts and sums of every call equal the reference."""
    from boa_hip.device import BufferView
    n, sv = ct.size, Y * X
    z_all = -(-n // sv)
    total = z_all * sv

    def wrap(a):
        return None if a is None else np.ascontiguousarray(np.resize(a.ravel(), total))

    ct, rules, regions, parts = wrap(ct), wrap(rules), wrap(regions), wrap(parts)
    v_ct, b_ct = _view(ctx, ct, offsets[0], 31000)
    v_ru, b_ru = _view(ctx, rules, offsets[1], 0) if rules is not None else (None, None)
    v_rg, b_rg = _view(ctx, regions, offsets[2], 5)
    v_pt, b_pt = _view(ctx, parts, offsets[3], 1) if parts is not None else (None, None)
    v_ts, b_ts = _view(ctx, np.full(total, 0xEE, np.uint8), offsets[4], 0xEE) if want_tissues else (None, None)

    def sub(v, itemsize, a, b):
        return None if v is None else BufferView(v._keep, v.ptr - v._keep.ptr + a * itemsize, (b - a) * itemsize)

    for z0 in range(0, z_all, max_z):
        z1 = min(z0 + max_z, z_all)
        a, b, Z = z0 * sv, z1 * sv, z1 - z0
        c, s = _run_aggregate(ctx, sub(v_ct, 2, a, b), sub(v_ru, 2, a, b), sub(v_rg, 1, a, b), sub(v_pt, 1, a, b), sub(v_ts, 1, a, b), Z, Y, X)
        shp = (Z, Y, X)
        t_ref, c_ref, s_ref = R.tissue_aggregate(ct[a:b].reshape(shp), None if rules is None else rules[a:b].reshape(shp),
                                                 regions[a:b].reshape(shp), None if parts is None else parts[a:b].reshape(shp))
        msg = f"{what} Y={Y} X={X} slices {z0}..{z1} offsets={offsets}"
        np.testing.assert_array_equal(c.astype(np.int64), c_ref, err_msg=msg)
        np.testing.assert_array_equal(s, s_ref, err_msg=msg)
        if want_tissues:
            np.testing.assert_array_equal(sub(v_ts, 1, a, b).download(shp, np.uint8), t_ref, err_msg=msg)
    if want_tissues:      # nothing written outside the view
        whole = b_ts.download((total + 48,), np.uint8)
        assert (whole[:offsets[4]] == 0xEE).all() and (whole[offsets[4] + total:] == 0xEE).all()
    for x in (b_ct, b_ru, b_rg, b_pt, b_ts):
        if x is not None:
            x.free()


@pytest.fixture(scope="module")
def truth():
    ct, regions = R.tissue_truth_table()
    rng = np.random.default_rng(1100)
    parts = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=ct.size)
    return ct.ravel(), regions.ravel(), parts


def test_tissue_truth_table_vector_path(ctx, truth):
    """every int16 HU x every region byte 0..255 as 256 slices of 256 x 256 (slice z = region z): 16-byte loads"""
    ct, regions, parts = truth
    _check_aggregate(ctx, ct, None, regions, parts, 256, 256, what="vector")
    _check_aggregate(ctx, ct, None, regions, None, 256, 256, what="vector, no parts")
    _check_aggregate(ctx, ct, None, regions, parts, 256, 256, want_tissues=False, what="vector, tissues_out = NULL")


def test_tissue_truth_table_scalar_path_same_slice_size(ctx, truth):
    """the same data and slice size through views that cannot be read with vector loads: each array in turn, then all"""
    ct, regions, parts = truth
    for offsets in ((1, 0, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 3, 0), (0, 0, 0, 0, 5), (1, 0, 3, 5, 7), (8, 0, 8, 8, 8)):
        _check_aggregate(ctx, ct, None, regions, parts, 256, 256, offsets=offsets, what="views")


def test_tissue_truth_table_ragged_and_small_slices(ctx, truth):
    ct, regions, parts = truth
    _check_aggregate(ctx, ct, None, regions, parts, 251, 261, what="ragged")            # odd slice size
    _check_aggregate(ctx, ct, None, regions, parts, 15, 13, what="slice < 256 voxels")
    _check_aggregate(ctx, ct, None, regions, parts, 1, 7, what="slice < 8 voxels")
    _check_aggregate(ctx, ct, None, regions, parts, 2, 4, what="slice = 8 voxels")      # one vector per slice


def test_tissue_rules_from_a_second_volume(ctx, truth):
    """ct_rules = the truth table, ct = a permuted copy: tissues from ct_rules, sums from ct; with the torso row; also with
    ct_rules alone in a view at an odd voxel offset next to an aligned ct (the wrapper must not take the 16-byte-load path on
    ct_rules' account), and with tissues_out = NULL"""
    rules, regions, parts = truth
    rng = np.random.default_rng(1200)
    ct = rng.permutation(rules)
    _check_aggregate(ctx, ct, rules, regions, parts, 256, 256, what="ct_rules")
    _check_aggregate(ctx, ct, rules, regions, parts, 256, 256, offsets=(0, 1, 0, 0, 0), what="ct_rules at an odd voxel")
    _check_aggregate(ctx, ct, rules, regions, parts, 256, 256, offsets=(0, 8, 0, 0, 0), what="ct_rules 16 bytes on")
    _check_aggregate(ctx, ct, rules, regions, parts, 256, 256, want_tissues=False, what="ct_rules, tissues_out = NULL")
    _check_aggregate(ctx, ct, rules, regions, parts, 37, 29, what="ct_rules, ragged")


def test_tissue_sums_at_the_int16_extremes(ctx, truth):
    """ct_rules runs through the truth table (so the bone / muscle / adipose windows are hit) while ct sits at -32 768 / 32 767,
    mostly negative in the slices of regions 1, 5, 9 and mostly positive in those of 2, 3, 7: the negative sums travel through
    unsigned 64-bit atomics.  Then whole slices of bone at one extreme: sums of -2^31 and 2^31 - 65 536, outside int32."""
    rules, regions, parts = truth
    rng = np.random.default_rng(1300)
    n = rules.size
    share = np.full(256, 0.5)
    share[[1, 5, 9]], share[[2, 3, 7]] = 0.97, 0.03
    ct = np.where(rng.random(n) < np.repeat(share, n // 256), -32768, 32767).astype(np.int16)
    _check_aggregate(ctx, ct, rules, regions, parts, 256, 256, what="extremes")
    _check_aggregate(ctx, ct, rules, regions, parts, 256, 256, offsets=(1, 1, 1, 1, 1), what="extremes, scalar")
    s = R.tissue_aggregate(ct.reshape(256, 256, 256), rules.reshape(256, 256, 256), regions.reshape(256, 256, 256), None)[2]
    assert s.min() < -(1 << 26) and s.max() > (1 << 22)                       # (the case is what it says)
    Z = 6
    ct = np.repeat(np.array([-32768, 32767, -32768, -32768, 32767, 32767], np.int16), 65536)
    bone, zeros = np.full(Z * 65536, 5, np.uint8), np.zeros(Z * 65536, np.int16)
    for offsets in ((0, 0, 0, 0, 0), (3, 5, 1, 1, 1)):
        _check_aggregate(ctx, ct, zeros, bone, np.ones(Z * 65536, np.uint8), 256, 256, offsets=offsets, what="whole slices of bone")
    s = R.tissue_aggregate(ct.reshape(Z, 256, 256), zeros.reshape(Z, 256, 256), bone.reshape(Z, 256, 256), None)[2]
    assert s[0, 0, 2] == -(1 << 31) and s[1, 0, 2] == (1 << 31) - 65536


# ---- boa_tissue_projections --------------------------------------------------------------------------------------------
def _run_projections(ctx, tissues, regions, vals):
    from boa_hip._lib import check
    Z, Y, X = tissues.shape
    T = len(vals)
    v = np.ascontiguousarray(vals, dtype=np.uint8)
    d_t, d_r = ctx.from_numpy(tissues), ctx.from_numpy(regions)
    d_c, d_s, d_mc, d_ms = ctx.alloc(T * Z * X * 4), ctx.alloc(T * Z * Y * 4), ctx.alloc(Z * X), ctx.alloc(Z * Y)
    try:
        for b, nb in ((d_c, T * Z * X * 4), (d_s, T * Z * Y * 4), (d_mc, Z * X), (d_ms, Z * Y)):
            check(ctx.lib.boa_memset(ctx.h, b.vp, 0x77, nb))
        check(ctx.lib.boa_tissue_projections(ctx.h, d_t.vp, d_r.vp, Z, Y, X, v.ctypes.data_as(C.c_void_p), T, d_c.vp, d_s.vp, d_mc.vp,
                                             d_ms.vp), "boa_tissue_projections")
        return (d_c.download((T, Z, X), np.uint32), d_s.download((T, Z, Y), np.uint32), d_mc.download((Z, X), np.uint8),
                d_ms.download((Z, Y), np.uint8))
    finally:
        for b in (d_t, d_r, d_c, d_s, d_mc, d_ms):
            b.free()


@pytest.mark.parametrize("T", [1, 7, 16])
@pytest.mark.parametrize("YX", [(1, 1), (5, 63), (37, 64), (3, 257), (9, 300), (40, 513), (512, 512)])
def test_tissue_projections(ctx, YX, T):
    """X below one wave, exactly one wave, one column pass (X <= 256), several with a padded last pass; tissue values that are not
    in the value list; rows and columns of region 0 / 255 (255 is not body)"""
    Y, X = YX
    Z = 3
    rng = np.random.default_rng(1400 + 7 * X + Y + T)
    vals = [int(v) for v in rng.permutation(np.arange(1, 20))[:T]]
    tissues = rng.integers(0, 24, size=(Z, Y, X), dtype=np.uint8)
    tissues[0, :, X // 2] = vals[0]
    tissues[1, Y // 2, :] = vals[-1]
    assert set(np.unique(tissues)) - set(vals) or Y * X == 1
    regions = rng.choice(np.array([0, 0, 0, 1, 11, 254, 255, 255], np.uint8), size=(Z, Y, X))
    regions[0, Y // 2, :] = 0
    regions[0, :, X // 3] = 255
    regions[1, :, X // 2] = 0
    regions[1, Y // 3, :] = 255
    regions[2] = rng.choice(np.array([0, 255], np.uint8), size=(Y, X))        # no body at all in this slice
    regions[2, Y - 1, X - 1] = 254 if T == 7 else 255                         # ... or a single body voxel in the last lane
    cor, sag, mc, ms = _run_projections(ctx, tissues, regions, vals)
    w_cor, w_sag, w_mc, w_ms = R.tissue_projections(tissues, regions, vals)
    np.testing.assert_array_equal(cor.astype(np.int64), w_cor)
    np.testing.assert_array_equal(sag.astype(np.int64), w_sag)
    np.testing.assert_array_equal(mc, w_mc.astype(np.uint8))
    np.testing.assert_array_equal(ms, w_ms.astype(np.uint8))
    assert not w_mc[0, X // 3] and not w_ms[0, Y // 2] and w_mc[2].any() == (T == 7)


def test_tissue_projections_lds_bound(ctx):
    """(T (X + Y) + X + Y) * 4 bytes of LDS: the largest slice that fits runs and is right; one column more is refused with
    BOA_EINVAL before anything is launched"""
    T, Y = 16, 1
    x_max = 160 * 1024 // 4 // (T + 1) - Y
    rng = np.random.default_rng(1500)
    vals = list(range(1, T + 1))
    tissues = rng.integers(0, 18, size=(2, Y, x_max), dtype=np.uint8)
    regions = rng.choice(np.array([0, 3, 255], np.uint8), size=(2, Y, x_max))
    cor, sag, mc, ms = _run_projections(ctx, tissues, regions, vals)
    w = R.tissue_projections(tissues, regions, vals)
    np.testing.assert_array_equal(cor.astype(np.int64), w[0])
    np.testing.assert_array_equal(sag.astype(np.int64), w[1])
    np.testing.assert_array_equal(mc, w[2].astype(np.uint8))
    np.testing.assert_array_equal(ms, w[3].astype(np.uint8))
    big = np.zeros((1, Y, x_max + 1), np.uint8)
    with pytest.raises(ValueError, match=r"needs \d+ bytes of LDS"):
        _run_projections(ctx, big, big, vals)
    with pytest.raises(ValueError, match=r"tissue values"):
        _run_projections(ctx, big[:, :, :8], big[:, :, :8], list(range(17)))


# ---- boa_median3_inplane -----------------------------------------------------------------------------------------------
def _run_median(ctx, vol, flat_axis):
    from boa_hip import bca
    d = ctx.from_numpy(vol)
    o = bca.median_filter_inplane(ctx, d, vol.shape, flat_axis)
    out = o.download(vol.shape, np.int16)
    d.free()
    o.free()
    return out


@pytest.mark.parametrize("flat_axis", [0, 1, 2])
@pytest.mark.parametrize("lo_hi", [(-32768, 32767), (0, 1), (32767, -32768)], ids=["extremes", "zero_one", "swapped"])
def test_median3_zero_one_principle(ctx, flat_axis, lo_hi):
    """All 512 binary 3x3 neighbourhoods, each the complete window of its own centre.  A comparator network that selects the
    median of every 0-1 input selects it for every input (0-1 principle; the exchanges only compare and swap)."""
    vol, (c0, c1), want = R.binary_neighbourhoods(lo_hi[0], lo_hi[1], flat_axis)
    got = _run_median(ctx, vol, flat_axis)
    g = np.moveaxis(got, flat_axis, 0)
    np.testing.assert_array_equal(g[0, c0, c1], want)
    np.testing.assert_array_equal(g[1, c0, c1], want)
    np.testing.assert_array_equal(got, R.median3_inplane(vol, flat_axis))     # (and the borders between / around the cells)


@pytest.mark.parametrize("flat_axis", [0, 1, 2])
def test_median3_short_axes_and_full_range(ctx, flat_axis):
    """in-plane axes of length 1 and 2: every sample is a border sample (mode="reflect" repeats the edge); random full-range int16"""
    rng = np.random.default_rng(1600 + flat_axis)
    for l0, l1 in ((1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (7, 1), (2, 9), (9, 2), (3, 3), (19, 23)):
        shape = [l0, l1]
        shape.insert(flat_axis, 5)
        vol = rng.integers(-32768, 32768, size=shape).astype(np.int16)
        np.testing.assert_array_equal(_run_median(ctx, vol, flat_axis), R.median3_inplane(vol, flat_axis), err_msg=str(shape))
        vol = rng.choice(np.array([-32768, -1, 0, 1, 32767], np.int16), size=shape)    # ties
        np.testing.assert_array_equal(_run_median(ctx, vol, flat_axis), R.median3_inplane(vol, flat_axis), err_msg=str(shape))


# ---- boa_slice_label_presence / boa_label_hu_mask / boa_label_select ----------------------------------------------------
@pytest.mark.parametrize("YX", [(1, 1), (1, 255), (1, 256), (1, 257), (2049, 33)])
def test_slice_label_presence(ctx, YX):
    """all 256 labels; slices of one voxel, around one workgroup's 256 threads, and of several workgroups; a label present only in
    the last voxel of its slice"""
    from boa_hip import bca
    Y, X = YX
    rng = np.random.default_rng(1700 + X)
    Z = 260
    lab = np.empty((Z, Y, X), np.uint8)
    for z in range(Z):
        some = rng.permutation(256)[:1 + z % 9].astype(np.uint8)            # a few labels per slice ...
        lab[z] = some[rng.integers(0, some.size, size=(Y, X))]
    lab[:256, 0, 0] = np.arange(256)                                         # ... every label in some slice ...
    last = (np.arange(Z) * 7 + 3) % 256
    for z in range(Z):
        if Y * X > 1:
            lab[z][lab[z] == last[z]] = (last[z] + 1) % 256
            lab[z, Y - 1, X - 1] = last[z]                                   # ... and one only in the slice's last voxel
    d = ctx.from_numpy(lab)
    got = bca.slice_label_presence(ctx, d, lab.shape)
    d.free()
    want = R.slice_label_presence(lab)
    np.testing.assert_array_equal(got, want)
    assert want.any(axis=0).all()
    if Y * X > 1:
        assert all(want[z, last[z]] and (lab[z].ravel()[:-1] != last[z]).all() for z in range(Z))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_label_hu_mask(ctx, cu_count, mode):
    """HU at lo - 1, lo, hi, hi + 1 and the int16 extremes x all 256 labels over full 256-entry look-up tables (non-zero = in);
    more voxels than one grid pass covers"""
    from boa_hip._lib import check
    rng = np.random.default_rng(1800 + mode)
    n = cu_count * 32 * 256 * 2 + 13
    for lo, hi in ((-190, -30), (-32768, 32767), (-32767, 32766), (5, 5), (6, 5)):
        edge = np.array([lo - 1, lo, hi, hi + 1, -32768, 32767, 0]).clip(-32768, 32767).astype(np.int16)
        ct = edge[rng.integers(0, edge.size, size=n)]
        lab = rng.integers(0, 256, size=n).astype(np.uint8)
        ct[:256 * edge.size] = np.repeat(edge, 256)                          # every (edge HU, label) pair
        lab[:256 * edge.size] = np.tile(np.arange(256, dtype=np.uint8), edge.size)
        lut = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), size=256)
        d_ct, d_lab, d_out = ctx.from_numpy(ct), ctx.from_numpy(lab), ctx.alloc(n + 16)
        check(ctx.lib.boa_memset(ctx.h, d_out.vp, 0x33, n + 16))
        check(ctx.lib.boa_label_hu_mask(ctx.h, d_ct.vp, d_lab.vp, lut.ctypes.data_as(C.c_void_p), mode, lo, hi, n, d_out.vp), "boa_label_hu_mask")
        got = d_out.download((n + 16,), np.uint8)
        np.testing.assert_array_equal(got[:n], R.label_hu_mask(ct, lab, lut, mode, lo, hi), err_msg=f"window {lo}..{hi}")
        assert (got[n:] == 0x33).all()
        for b in (d_ct, d_lab, d_out):
            b.free()


def test_label_select(ctx, cu_count):
    from boa_hip._lib import check
    rng = np.random.default_rng(1900)
    n = cu_count * 32 * 256 + 257
    lab = rng.integers(0, 256, size=n).astype(np.uint8)
    lab[:256] = np.arange(256)
    d_lab, d_out = ctx.from_numpy(lab), ctx.alloc(n + 16)
    for mode, vals in ((0, (0, 9, 9)), (0, (7, 0, 0)), (0, (255, 0, 0)), (1, (0, 0, 0)), (1, None), (2, (3, 255, 0)), (2, (9, 9, 9)),
                       (2, (1, 2, 254))):
        check(ctx.lib.boa_memset(ctx.h, d_out.vp, 0x33, n + 16))
        v = (C.c_int * 3)(*vals) if vals is not None else None
        check(ctx.lib.boa_label_select(ctx.h, d_lab.vp, n, mode, v, d_out.vp), "boa_label_select")
        got = d_out.download((n + 16,), np.uint8)
        np.testing.assert_array_equal(got[:n], R.label_select(lab, mode, vals or (0, 0, 0)), err_msg=f"mode {mode} {vals}")
        assert (got[n:] == 0x33).all()
    d_lab.free()
    d_out.free()
