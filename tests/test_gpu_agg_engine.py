"""The sharded connected-component engine on the device, in ONE process: agg_shard.HipAggEngine under the in-process communicator of
tests/agg_shard_cases.py over every (mask, cut plan) pair that tests/test_agg_shard_cases_cpu.py runs with the numpy engine -- slabs
of one plane, of no plane, without foreground, cuts on and next to a CCL tile boundary, components that exist only through an
interface.  filter_largest_sharded and remove_small_sharded must equal the whole-volume references (scipy / flood fill) AND the
single-GPU filters (boa_ccl26 + boa_ccl_filter_largest / boa_ccl_remove_small); the four-filter region chain must equal
_postprocess_region_segmentation_device_bytes; HipAggEngine.boundary_and_components must return what NumpyAggEngine returns; the three
C entry points behind the engine (boa_ccl_list_components, boa_scatter_u32, boa_ccl_fill_unmarked) are called directly between guard
regions; and the two halo claims of the sharded measurements (erosion on slab + ERODE_REACH planes, histograms over owned views) are
checked for every cut plan.  Integers only: every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import agg_shard_cases as AC
import morph_cases as MC
from test_gpu_bits_morph import ctx  # noqa: F401  (the module-scoped device context fixture)

pytestmark = pytest.mark.gpu

MARK = 0xFFFFFFFF
GUARD = 256                      # bytes before and after every device array a kernel under test writes or reads
FILL = 0xA5


def _check(rc, what=""):
    from boa_hip._lib import check
    check(rc, what)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class _Dev:
    """a host array on the device between two guard regions; read() returns the body and asserts that the guards are untouched"""

    def __init__(self, ctx, arr):
        from boa_hip.device import BufferView
        self.host = np.ascontiguousarray(arr)
        self.nb = self.host.nbytes
        raw = np.full(self.nb + 2 * GUARD, FILL, np.uint8)
        raw[GUARD:GUARD + self.nb] = self.host.reshape(-1).view(np.uint8)
        self.buf = ctx.from_numpy(raw)
        self.body = BufferView(self.buf, GUARD, self.nb)

    @property
    def vp(self):
        return self.body.vp

    def view(self, byte_offset, nbytes):
        from boa_hip.device import BufferView
        assert 0 <= byte_offset and byte_offset + nbytes <= self.nb
        return BufferView(self.buf, GUARD + byte_offset, nbytes)

    def read(self):
        raw = self.buf.download((self.nb + 2 * GUARD,), np.uint8)
        assert (raw[:GUARD] == FILL).all() and (raw[GUARD + self.nb:] == FILL).all(), "guard region written"
        return raw[GUARD:GUARD + self.nb].view(self.host.dtype).reshape(self.host.shape).copy()

    def free(self):
        self.buf.free()


class _Slabs:
    """the engines (one per slab shape) and the slab views of the resident volumes of one cut plan"""

    def __init__(self, ctx, shape, cuts):
        from boa_hip import agg_shard as ag
        self.cuts, self.plane = cuts, shape[1] * shape[2]
        self.engines = {}
        for a, b in cuts:
            if b - a not in self.engines:
                self.engines[b - a] = ag.HipAggEngine(ctx, (b - a, shape[1], shape[2]))

    def engine(self, r):
        return self.engines[self.cuts[r][1] - self.cuts[r][0]]

    def view(self, dev, r, itemsize=1):
        a, b = self.cuts[r]
        return dev.view(a * self.plane * itemsize, (b - a) * self.plane * itemsize)

    def close(self):
        for e in self.engines.values():
            e.close()


# ---- the protocol with the HIP engine --------------------------------------------------------------------------------------------
_WHOLE = {}


def _whole_volume(ctx, name):
    """the single-GPU filters on the whole volume of a case, once per process: (label volume after boa_ccl26 + boa_ccl_filter_largest,
    {threshold: mask after boa_ccl_remove_small})"""
    if name not in _WHOLE:
        c = AC.all_cases()[name]
        m = c["mask"]
        n = m.size
        d_m = ctx.from_numpy(m.astype(np.uint8))
        d_roots, d_sizes = ctx.alloc(n * 4), ctx.alloc(n * 4)
        _check(ctx.lib.boa_ccl26(ctx.h, d_m.vp, *m.shape, d_roots.vp, d_sizes.vp, None), "boa_ccl26")
        d_seg = ctx.from_numpy(AC.seg_around(m))
        _check(ctx.lib.boa_ccl_filter_largest(ctx.h, d_roots.vp, d_sizes.vp, n, d_seg.vp, 255), "boa_ccl_filter_largest")
        small = {}
        for t in c["thresholds"]:
            d_w = ctx.from_numpy(m.astype(np.uint8))
            _check(ctx.lib.boa_ccl_remove_small(ctx.h, d_roots.vp, d_sizes.vp, n, t, d_w.vp), "boa_ccl_remove_small")
            small[t] = d_w.download(m.shape, np.uint8)
            d_w.free()
        _WHOLE[name] = (d_seg.download(m.shape, np.uint8), small)
        for b in (d_m, d_roots, d_sizes, d_seg):
            b.free()
    return _WHOLE[name]


@pytest.mark.parametrize("name,plan", AC.pairs(), ids=lambda v: v)
def test_protocol_hip_engine(ctx, name, plan):
    """filter_largest_sharded and remove_small_sharded (every threshold of the case) on BufferViews of one resident volume: equal to the
    whole-volume reference and to the single-GPU filters; nothing outside the volumes is written and the mask of filter_largest is
    left alone"""
    from boa_hip import agg_shard as ag
    c = AC.all_cases()[name]
    m = c["mask"]
    cuts = AC.cut_plans(m.shape[0])[plan]
    m8, seg = m.astype(np.uint8), AC.seg_around(m)
    want_big, want_small = AC.references(name)
    gpu_big, gpu_small = _whole_volume(ctx, name)
    want = seg.copy()
    want[want_big] = 255
    S = _Slabs(ctx, m.shape, cuts)
    d_mask, d_seg = _Dev(ctx, m8), _Dev(ctx, seg)
    try:
        AC.drive(len(cuts), lambda comm, r: ag.filter_largest_sharded(comm, S.engine(r), S.view(d_mask, r), S.view(d_seg, r), cuts[r][0], 255))
        got = d_seg.read()
        np.testing.assert_array_equal(got, want, err_msg=f"{name} {plan}")
        np.testing.assert_array_equal(got, gpu_big, err_msg=f"{name} {plan}: single-GPU filter")
        np.testing.assert_array_equal(d_mask.read(), m8)
        for t in c["thresholds"]:
            d_w = _Dev(ctx, m8)
            AC.drive(len(cuts), lambda comm, r: ag.remove_small_sharded(comm, S.engine(r), S.view(d_w, r), cuts[r][0], t))
            got = d_w.read()
            d_w.free()
            np.testing.assert_array_equal(got, want_small[t].astype(np.uint8), err_msg=f"{name} {plan} max_size {t}")
            np.testing.assert_array_equal(got, gpu_small[t], err_msg=f"{name} {plan} max_size {t}: single-GPU filter")
    finally:
        S.close()
        d_mask.free()
        d_seg.free()


def test_region_chain_hip_engine(ctx):
    """the four filters of postprocess_region_segmentation_sharded, filter by filter over all ranks, on slab views of the phantom: equal
    to _postprocess_region_segmentation_device_bytes and to the oracle, for balanced cuts, one plane per rank, more ranks than planes
    and the cuts around plane 16"""
    from boa_hip import agg_shard as ag
    from boa_hip import bca
    from oracle import bca as obca
    R = bca.REGION
    seg = AC.region_phantom(R)
    shape, n = seg.shape, seg.size
    d_whole = ctx.from_numpy(seg)
    bca._postprocess_region_segmentation_device_bytes(ctx, d_whole, shape)
    want = d_whole.download(shape, np.uint8)
    d_whole.free()
    np.testing.assert_array_equal(want, obca.postprocess_region_segmentation(seg))
    assert int((want == 255).sum()) == sum(np.zeros(shape, bool)[sl].size for sl, _ in AC.region_islands(R))      # the islands, all of them
    chain = AC.region_chain(ag, R)
    assert len(chain) == 4
    d_mask = ctx.alloc(n)
    for plan, cuts in AC.cut_plans(shape[0], every_plane=True).items():
        S = _Slabs(ctx, shape, cuts)
        d_seg = _Dev(ctx, seg)

        def select(view, n_slab, mode, vals):
            if n_slab:
                _check(ctx.lib.boa_label_select(ctx.h, view.vp, n_slab, mode, (C.c_int * 3)(*vals), d_mask.vp), "boa_label_select")
            return d_mask

        for mode, vals, fill in chain:
            AC.drive(len(cuts), lambda comm, r: ag.filter_largest_sharded(
                comm, S.engine(r), select(S.view(d_seg, r), S.engine(r).n, mode, vals), S.view(d_seg, r), cuts[r][0], fill))
        got = d_seg.read()
        S.close()
        d_seg.free()
        np.testing.assert_array_equal(got, want, err_msg=plan)
    d_mask.free()


# ---- the engine contract ---------------------------------------------------------------------------------------------------------
def _assert_same_tables(got, want, what):
    (rf, rl, roots, sizes), (wf, wl, wroots, wsizes) = got, want
    if wf is None:
        assert rf is None and rl is None, what
    else:
        np.testing.assert_array_equal(rf, wf, err_msg=what + ": first plane")
        np.testing.assert_array_equal(rl, wl, err_msg=what + ": last plane")
    order = np.argsort(wroots)
    assert roots.dtype == sizes.dtype == np.int64
    np.testing.assert_array_equal(roots, wroots[order], err_msg=what + ": roots (sorted)")
    np.testing.assert_array_equal(sizes, wsizes[order], err_msg=what + ": sizes")


CONTRACT_NAMES = ("u_shape_small", "corner_chain_small", "all_background_small", "single_component_small", "all_foreground_small",
                  "corner_chain_big", "threshold_merge_big", "full_empty_mixed", "lattice1_33x35x70", "boustrophedon", "full_tile_contacts")


@pytest.mark.parametrize("name", CONTRACT_NAMES)
def test_boundary_and_components_equal_the_numpy_engine(ctx, name):
    """every slab of every plan of the case: the same boundary planes (global root ids, -1 = background), ascending roots and sizes
    as the numpy engine on the same slab -- slabs of one plane (first plane = last plane), of no plane, without foreground, and
    z0 > 0 (the offsets)"""
    from boa_hip import agg_shard as ag
    m = AC.all_cases()[name]["mask"]
    d_mask = _Dev(ctx, m.astype(np.uint8))
    ref = ag.NumpyAggEngine()
    seen = set()
    for plan, cuts in AC.cut_plans(m.shape[0]).items():
        S = _Slabs(ctx, m.shape, cuts)
        for r, (a, b) in enumerate(cuts):
            if (a, b) in seen:
                continue
            seen.add((a, b))
            eng = S.engine(r)
            cc = eng.ccl(S.view(d_mask, r))
            got = eng.boundary_and_components(cc, a)
            assert cc["n"] == len(got[2])
            _assert_same_tables(got, ref.boundary_and_components(ref.ccl(m[a:b]), a), f"{name} {plan} slab [{a}, {b})")
        S.close()
    np.testing.assert_array_equal(d_mask.read(), m.astype(np.uint8))
    d_mask.free()
    if m.shape[0] <= 8:
        assert {b - a for a, b in seen} >= {0, 1} and any(a > 0 and b - a == 1 for a, b in seen)
    if name in ("all_background_small", "single_component_small"):
        assert any(b > a and not m[a:b].any() for a, b in seen)


def test_engine_is_reusable_after_a_filter(ctx):
    """ccl, filter_largest (which scatters MARK into the engine's size table), then ccl again on the same engine: the second
    labelling's tables are clean, for the same mask and for another one; likewise after remove_small's scatter of merged sizes"""
    from boa_hip import agg_shard as ag
    A = AC.interface_cases()["late_winner_small"]["mask"]
    B = AC.interface_cases()["tie_three_small"]["mask"]
    ref, eng = ag.NumpyAggEngine(), ag.HipAggEngine(ctx, A.shape)
    d_a, d_b = _Dev(ctx, A.astype(np.uint8)), _Dev(ctx, B.astype(np.uint8))
    want_a = ref.boundary_and_components(ref.ccl(A), 2)
    want_b = ref.boundary_and_components(ref.ccl(B), 2)
    cc = eng.ccl(d_a.body)
    got = eng.boundary_and_components(cc, 2)
    _assert_same_tables(got, want_a, "first ccl")
    seg = AC.seg_around(A)
    d_seg = _Dev(ctx, seg)
    keep = [int(got[2][-1])]                                     # the component that starts last (the larger one)
    eng.fill_all_but(cc, keep, 2, d_seg.body, 255)
    want_seg = seg.copy()
    ref.fill_all_but(ref.ccl(A), keep, 2, want_seg, 255)
    assert (want_seg == 255).any() and (want_seg == 3).any()
    np.testing.assert_array_equal(d_seg.read(), want_seg)
    sizes = eng.d_sizes.download((A.size,), np.uint32)
    assert (sizes == MARK).sum() == 1                            # the mark is there ...
    _assert_same_tables(eng.boundary_and_components(eng.ccl(d_a.body), 2), want_a, "ccl after filter_largest, same mask")     # ... and gone
    cc = eng.ccl(d_b.body)
    _assert_same_tables(eng.boundary_and_components(cc, 2), want_b, "ccl after filter_largest, other mask")
    d_w, want_w = _Dev(ctx, B.astype(np.uint8)), B.astype(np.uint8)
    changed = [(int(want_b[2][0]), 50)]                          # the first component counts as 50 voxels: it alone stays
    eng.remove_small(cc, changed, 2, 5, d_w.body)
    ref.remove_small(ref.ccl(B), changed, 2, 5, want_w)
    assert 0 < want_w.sum() < B.sum()
    np.testing.assert_array_equal(d_w.read(), want_w)
    _assert_same_tables(eng.boundary_and_components(eng.ccl(d_b.body), 2), want_b, "ccl after remove_small")
    eng.close()
    for d in (d_a, d_b, d_seg, d_w):
        d.free()


# ---- the three C entry points ----------------------------------------------------------------------------------------------------
ROOT_SENTINEL, SIZE_SENTINEL = -7, 0xDEADBEEF
PAD = 64


def _sizes_table(n, density, seed):
    """a per-voxel size table as boa_ccl26 leaves it: 0 but at the roots; among the values 1, MARK and MARK - 1"""
    rng = np.random.default_rng(seed)
    sizes = np.zeros(n, np.uint32)
    at = np.flatnonzero(rng.random(n) < density)
    vals = rng.integers(1, 1 << 32, size=len(at), dtype=np.uint64).astype(np.uint32)
    vals[vals == SIZE_SENTINEL] = 1
    vals[:3] = (1, MARK, MARK - 1)[:len(vals)]
    sizes[at] = vals
    if n:
        sizes[n - 1] = 12345                                     # the last element is a root
    return sizes


def _list_components(ctx, d_sizes, n, max_out):
    hr = np.full(max_out + PAD, ROOT_SENTINEL, np.int32)
    hs = np.full(max_out + PAD, SIZE_SENTINEL, np.uint32)
    cnt = C.c_int(-5)
    _check(ctx.lib.boa_ccl_list_components(ctx.h, d_sizes.vp, n, max_out, _vp(hr), _vp(hs), C.byref(cnt)), "boa_ccl_list_components")
    return hr, hs, cnt.value


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000, 70001])
def test_ccl_list_components(ctx, n):
    """the (root, size) pairs of the non-zero entries, in any order; with max_out below the count the count is still the true one,
    exactly max_out entries are written, each a true pair, no pair twice, and nothing lands past them"""
    sizes = _sizes_table(n, 0.5 if n < 300 else 0.03, n)
    true = {int(i): int(sizes[i]) for i in np.flatnonzero(sizes)}
    count = len(true)
    assert (n == 0) == (count == 0)
    d_sizes = _Dev(ctx, sizes)
    for max_out in sorted({count, count + 5, max(count - 1, 0), count // 2, min(count, 1), 0}):
        hr, hs, cnt = _list_components(ctx, d_sizes, n, max_out)
        k = min(count, max_out)
        assert cnt == count, f"n {n} max_out {max_out}"
        assert (hr[k:] == ROOT_SENTINEL).all() and (hs[k:] == SIZE_SENTINEL).all(), f"n {n} max_out {max_out}: written past the {k} entries"
        got = list(zip(hr[:k].tolist(), hs[:k].tolist()))
        assert len(set(p[0] for p in got)) == k and all(true.get(r) == s for r, s in got), f"n {n} max_out {max_out}"
        if max_out >= count:
            assert dict(got) == true
    np.testing.assert_array_equal(d_sizes.read(), sizes)
    d_sizes.free()


@pytest.mark.parametrize("m", [0, 1, 256, 257])
def test_scatter_u32(ctx, m):
    """dst[idx[i]] = val[i] for distinct indices, the first and the last element among them; every other element, and what lies
    before and after the array, keeps its content"""
    n = 1000
    rng = np.random.default_rng(m)
    dst = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    runs = []
    if m == 0:
        runs = [(None, None), (np.zeros(0, np.int32), np.zeros(0, np.uint32))]
    elif m == 1:
        runs = [(np.array([0], np.int32), np.array([MARK], np.uint32)), (np.array([n - 1], np.int32), np.array([7], np.uint32))]
    else:
        idx = rng.permutation(np.arange(1, n - 1))[:m - 2].astype(np.int32)
        idx = np.concatenate([idx[:5], np.array([n - 1, 0], np.int32), idx[5:]])
        val = rng.integers(0, 1 << 32, size=m, dtype=np.uint64).astype(np.uint32)
        val[:2] = (MARK, 0)
        runs = [(idx, val)]
    for idx, val in runs:
        assert idx is None or (len(idx) == m and len(set(idx.tolist())) == m)
        d_dst = _Dev(ctx, dst)
        _check(ctx.lib.boa_scatter_u32(ctx.h, d_dst.vp, None if idx is None else _vp(idx), None if val is None else _vp(val), m), "boa_scatter_u32")
        want = dst.copy()
        if m:
            want[idx] = val
        np.testing.assert_array_equal(d_dst.read(), want)
        d_dst.free()


def _forest(n, seed):
    """roots / sizes of a made-up labelling of n voxels: a third background, every other voxel points at one of up to six roots (each
    its own root); the roots' sizes are MARK, MARK - 1 (a true size that is NOT the mark), 1, MARK, 77 and 0x80000000 in turn"""
    rng = np.random.default_rng(seed)
    roots = np.full(n, -1, np.int32)
    fg = np.flatnonzero(rng.random(n) >= 0.33) if n > 1 else np.arange(n)
    sizes = np.zeros(n, np.uint32)
    if len(fg):
        heads = fg[:: max(1, len(fg) // 6)][:6]
        roots[fg] = heads[rng.integers(0, len(heads), size=len(fg))]
        roots[heads] = heads
        sizes[heads] = np.array([MARK, MARK - 1, 1, MARK, 77, 0x80000000], np.uint32)[:len(heads)]
    return roots, sizes


@pytest.mark.parametrize("fill", [0, 255])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_ccl_fill_unmarked(ctx, n, fill):
    """seg = fill on the voxels of every component whose size entry is not the mark; marked components and the background keep their
    labels (the background also where seg != 0); a size of 0xFFFFFFFE is not the mark"""
    variants = [_forest(n, n)]
    if n == 1:
        variants = [(np.array([0], np.int32), np.array([MARK], np.uint32)), (np.array([0], np.int32), np.array([MARK - 1], np.uint32)),
                    (np.array([-1], np.int32), np.array([0], np.uint32))]
    for roots, sizes in variants:
        seg = np.random.default_rng(n + fill).integers(1, 255, size=n).astype(np.uint8)
        want = seg.copy()
        hit = (roots >= 0) & (sizes[np.maximum(roots, 0)] != MARK)
        want[hit] = fill
        if n > 1:
            marked = (roots >= 0) & ~hit
            assert hit.any() and marked.any() and (roots < 0).any() and (sizes[roots[hit]] == MARK - 1).any()
        d_roots, d_sizes, d_seg = _Dev(ctx, roots), _Dev(ctx, sizes), _Dev(ctx, seg)
        _check(ctx.lib.boa_ccl_fill_unmarked(ctx.h, d_roots.vp, d_sizes.vp, n, MARK, d_seg.vp, fill), "boa_ccl_fill_unmarked")
        np.testing.assert_array_equal(d_seg.read(), want)
        np.testing.assert_array_equal(d_roots.read(), roots)
        np.testing.assert_array_equal(d_sizes.read(), sizes)
        for d in (d_roots, d_sizes, d_seg):
            d.free()


# ---- the halo claims of the sharded measurements ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", AC.ERODE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_erosion_on_slab_plus_halo(ctx, shape):
    """measurements.binary_erode on a slab plus ERODE_REACH planes towards its neighbours, owned planes only, equals the same planes
    of the whole volume's erosion (and the host reference) for every cut plan -- the volume's first and last planes included"""
    from boa_hip import measurements as M
    m = AC.erode_mask(shape)
    Z, Y, X = shape
    plane = Y * X
    d_m = _Dev(ctx, m.astype(np.uint8))
    d_o, d_t = _Dev(ctx, np.zeros(shape, np.uint8)), ctx.alloc(m.size)
    M.binary_erode(ctx, d_m.body, d_o.body, d_t, shape)
    whole = d_o.read()
    np.testing.assert_array_equal(whole.astype(bool), MC.erode_box_ref(m, *MC.erode_reach(6)))
    for plan, cuts in AC.cut_plans(Z).items():
        for a, b in cuts:
            if b == a:
                continue
            h0, h1 = AC.halo(Z, a, b)
            d_s = _Dev(ctx, np.full((h1 - h0, Y, X), 9, np.uint8))
            M.binary_erode(ctx, d_m.view(h0 * plane, (h1 - h0) * plane), d_s.body, d_t, (h1 - h0, Y, X))
            got = d_s.read()[a - h0:b - h0]
            d_s.free()
            np.testing.assert_array_equal(got, whole[a:b], err_msg=f"{plan} slab [{a}, {b}) of halo [{h0}, {h1})")
    np.testing.assert_array_equal(d_m.read(), m.astype(np.uint8))
    for d in (d_m, d_o, d_t):
        d.free()


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("shape", AC.HIST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_histogram_over_owned_views(ctx, shape, masked):
    """_label_hu_histogram_local over each slab's owned views, summed over the slabs of a plan, equals the whole volume's histogram
    and the host reference, for every cut plan; the plane has 35 voxels, so most views are not 16-byte aligned"""
    from boa_hip import measurements as M
    ct, lab, mask = AC.hist_inputs(shape)
    Z, plane = shape[0], shape[1] * shape[2]
    d_ct, d_lab, d_mask = _Dev(ctx, ct), _Dev(ctx, lab), _Dev(ctx, mask)
    want = AC.hist_ref(ct, lab, mask if masked else None, M.NBINS, M.HU_MIN)
    assert want[255, 0] >= 1 and want[255, M.NBINS - 1] >= 1 and want[0].sum() == 0
    whole = M._label_hu_histogram_local(ctx, d_ct.body, d_lab.body, ct.size, d_mask.body if masked else None)
    np.testing.assert_array_equal(whole, want)
    unaligned = 0
    for plan, cuts in AC.cut_plans(Z).items():
        total = np.zeros_like(want)
        for a, b in cuts:
            if b == a:
                continue
            v_ct, v_lab = d_ct.view(a * plane * 2, (b - a) * plane * 2), d_lab.view(a * plane, (b - a) * plane)
            v_mask = d_mask.view(a * plane, (b - a) * plane) if masked else None
            unaligned += v_lab.ptr % 16 != 0
            total += M._label_hu_histogram_local(ctx, v_ct, v_lab, (b - a) * plane, v_mask)
        assert np.array_equal(total, want), plan
    assert unaligned >= 4
    for d in (d_ct, d_lab, d_mask):
        d.read()
        d.free()
