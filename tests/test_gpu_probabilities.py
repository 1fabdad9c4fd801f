"""Class probabilities on the device (boa_logits_to_probabilities, csrc/prob.hip) and the layers above it
(HipPredictor.predict_segmentation(return_probabilities=True), SegmentationTask.predict_image(save_probabilities=...)).

The reference of the kernel tests is the numpy float64 restatement below of what
convert_predicted_logits_to_segmentation_with_correct_shape(..., return_probabilities=True) does (order-1 resampling rounded to
fp16, softmax, crop revert with background (1, 0, ..), transpose); the tolerance is the derived bound of tests/softmax_reference.py,
(C + 110) 2^-24 relative where p64 > 2^-100 and 2^-99 absolute elsewhere."""
import ctypes as C
import itertools
import os
import pickle

import numpy as np
import pytest

import softmax_reference as S
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

F16 = np.float16
PERMS = list(itertools.permutations(range(3)))
LUT = (np.arange(256) * 7 % 251 + 3).astype(np.uint8)          # lut[0] = 3: the label outside the box is not 0
BOA_EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


def _i3(v):
    return None if v is None else (C.c_int * 3)(*[int(x) for x in v])


def _call(ctx, d_lg, Cn, grid, off, dims, out, axis, lo, full, perm, d_prob, lut, d_lab):
    return ctx.lib.boa_logits_to_probabilities(ctx.h, d_lg.vp if d_lg is not None else None, Cn, _i3(grid), _i3(off), _i3(dims), _i3(out),
                                               axis, _i3(lo), _i3(full), _i3(perm), d_prob.vp if d_prob is not None else None,
                                               lut.ctypes.data_as(C.c_void_p) if lut is not None else None,
                                               d_lab.vp if d_lab is not None else None)


def _run(ctx, lg, off, dims, out, axis, lo, full, perm, lut=LUT, labels=True):
    """fp16 logits [C, *grid] -> (probabilities float32 [C, *full permuted], labels uint8 or None)."""
    from boa_hip._lib import check
    Cn, grid = lg.shape[0], lg.shape[1:]
    D = [full[p] for p in perm]
    n = int(np.prod(D))
    d_lg = ctx.from_numpy(np.ascontiguousarray(lg).view(np.uint16))
    d_prob = ctx.alloc(Cn * n * 4)
    d_lab = ctx.alloc(n) if labels else None
    try:
        check(_call(ctx, d_lg, Cn, grid, off, dims, out, axis, lo, full, perm, d_prob, lut, d_lab), "boa_logits_to_probabilities")
        return d_prob.download((Cn, *D), np.float32), (d_lab.download(tuple(D), np.uint8) if labels else None)
    finally:
        for b in (d_lg, d_prob, d_lab):
            if b is not None:
                b.free()


# ---- the float64 restatement ------------------------------------------------------------------------------------------------
def _axis_taps(n_in, n_out, linear):
    """-> (i0, i1, w0, w1) per output index: order 1 with the tap indices clamped (mode "nearest"), or order 0 along the slice axis."""
    o = np.arange(n_out, dtype=np.float64)
    if linear:
        cc = (o + 0.5) * (n_in / n_out) - 0.5
        fl = np.floor(cc)
        x = cc - fl
        return np.clip(fl, 0, n_in - 1).astype(int), np.clip(fl + 1, 0, n_in - 1).astype(int), 1.0 - x, x
    if n_in == n_out:
        i = np.arange(n_out)
    else:
        i = np.clip(np.floor((n_in / n_out) * (o + 0.5) - 0.5 + 0.5), 0, n_in - 1).astype(int)
    return i, None, None, None


def resample_order1_f16(box, out, axis):
    """resampling_fn_probabilities (order 1, order_z 0 along `axis`, -1 = none) of fp16 [C, *I] to `out` in float64, rounded to fp16."""
    x = box.astype(np.float64)
    taps = [_axis_taps(box.shape[1 + d], out[d], d != axis) for d in range(3)]
    res = np.zeros((box.shape[0], *out), dtype=np.float64)
    for p in range(2):
        for q in range(2):
            for r in range(2):
                sel, skip = [], False
                for d, k in enumerate((p, q, r)):
                    i0, i1, _, _ = taps[d]
                    skip = skip or (i1 is None and k == 1)          # one tap along an axis that is not interpolated
                    sel.append(i0 if (i1 is None or k == 0) else i1)
                if skip:
                    continue
                v = x[:, sel[0][:, None, None], sel[1][None, :, None], sel[2][None, None, :]]
                cf = v
                for d in range(3):                               # v * w0 * w1 * w2 in axis order, one rounding each, as in the kernel
                    if taps[d][1] is not None:
                        k = (p, q, r)[d]
                        shp = [1, 1, 1, 1]
                        shp[1 + d] = out[d]
                        cf = cf * (taps[d][3] if k else taps[d][2]).reshape(shp)
                res = res + cf
    return res.astype(F16)


def reference(lg, off, dims, out, axis, lo, full, perm):
    """-> (float64 probabilities [C, *full permuted], inside-the-box mask [*full permuted])."""
    Cn, grid = lg.shape[0], lg.shape[1:]
    off = off if off is not None else (0, 0, 0)
    dims = dims if dims is not None else grid
    box = lg[:, off[0]:off[0] + dims[0], off[1]:off[1] + dims[1], off[2]:off[2] + dims[2]]
    if out is not None and tuple(out) != tuple(dims):
        box = resample_order1_f16(box, tuple(out), axis)
    p = np.zeros((Cn, *full), dtype=np.float64)
    p[0] = 1.0
    inside = np.zeros(tuple(full), dtype=bool)
    sl = tuple(slice(lo[d], lo[d] + box.shape[1 + d]) for d in range(3))
    p[(slice(None),) + sl] = S.softmax64(box)
    inside[sl] = True
    return p.transpose([0] + [q + 1 for q in perm]), inside.transpose(perm)


def check_against_reference(got_p, got_lab, lg, off, dims, out, axis, lo, full, perm, what):
    Cn = lg.shape[0]
    p64, inside = reference(lg, off, dims, out, axis, lo, full, perm)
    assert got_p.shape == p64.shape and got_p.dtype == np.float32
    # outside the box: exactly (1, 0, ..., 0) and label lut[0]
    outside = ~inside
    assert (got_p[0][outside] == 1.0).all() and (got_p[1:][:, outside] == 0.0).all(), what
    nan = np.isnan(p64).any(axis=0)
    assert np.isnan(got_p[:, nan]).all(), what                         # a NaN logit: NaN probabilities at that voxel
    assert np.isfinite(got_p[:, ~nan]).all(), what
    rel = S.assert_within_bound(got_p[:, inside & ~nan], p64[:, inside & ~nan], Cn, what)
    if got_lab is not None:
        assert (got_lab[outside] == LUT[0]).all() and (got_lab[nan] == LUT[0]).all(), what
        inv = np.full(256, -1)
        inv[LUT[:Cn]] = np.arange(Cn)
        idx = inv[got_lab]
        assert (idx >= 0).all()
        S.assert_labels(idx, got_p, p64, Cn, what)
    return rel


def _volume(Cn, grid, seed=0, nan_at=None):
    lg = S.fill_volume(Cn, grid, seed)
    if nan_at is not None:
        lg[Cn // 2][tuple(nan_at)] = np.nan
    return lg


# ---- kernel, direct ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [2, 3, 25, 33, 118])
@pytest.mark.parametrize("perm", PERMS, ids=["".join(map(str, p)) for p in PERMS])
def test_box_in_padded_grid_into_larger_grid_every_permutation(ctx, Cn, perm):
    grid, off, dims, lo, full = (5, 6, 7), (1, 0, 2), (3, 5, 4), (2, 3, 0), (6, 9, 5)
    lg = _volume(Cn, grid, seed=Cn, nan_at=(2, 3, 4))                   # (inside the pad box)
    p, lab = _run(ctx, lg, off, dims, None, -1, lo, full, perm)
    check_against_reference(p, lab, lg, off, dims, None, -1, lo, full, perm, f"perm {perm}")
    # out_dims equal to the box is the same call; without a label plane the probabilities are the same bits
    p2, none = _run(ctx, lg, off, dims, dims, 0, lo, full, perm, labels=False)
    assert none is None
    np.testing.assert_array_equal(p2.view(np.uint32), p.view(np.uint32))


@pytest.mark.parametrize("Cn", [3, 25, 33])
@pytest.mark.parametrize("case", [
    # fastest extents of 65 and 257: one past a wave and one past a workgroup of the row kernel (one voxel per lane)
    dict(grid=(3, 4, 70), off=(1, 1, 3), dims=(2, 2, 65), lo=(0, 1, 0), full=(3, 3, 65)),
    dict(grid=(2, 3, 257), off=(0, 1, 0), dims=(2, 2, 257), lo=(1, 0, 0), full=(3, 2, 257)),
    # every fastest extent and offset a multiple of 4: four voxels per lane; 260 / 4 = 65 lanes per row
    dict(grid=(3, 3, 72), off=(1, 0, 8), dims=(2, 3, 64), lo=(0, 1, 4), full=(2, 5, 260)),
    dict(grid=(2, 2, 1028), off=(0, 0, 0), dims=(2, 2, 1028), lo=(0, 0, 0), full=(2, 3, 1028)),
    # the box is the grid (no pad, no crop): one voxel and four voxels per lane
    dict(grid=(3, 5, 7), off=None, dims=None, lo=(0, 0, 0), full=(3, 5, 7)),
    dict(grid=(4, 6, 64), off=None, dims=None, lo=(0, 0, 0), full=(4, 6, 64)),
], ids=["z65", "z257", "vec4-z260", "vec4-z1028", "box=grid", "vec4-box=grid"])
def test_row_kernel_edges(ctx, Cn, case):
    lg = _volume(Cn, case["grid"], seed=7 + Cn, nan_at=(1, 1, 1))
    args = (case["off"], case["dims"], None, -1, case["lo"], case["full"], (0, 1, 2))
    p, lab = _run(ctx, lg, *args)
    check_against_reference(p, lab, lg, *args, f"{case}")
    # the per-voxel kernel (a transposing call) gives the same bits as the row kernel
    args_t = args[:-1] + ((0, 2, 1),)
    pt, labt = _run(ctx, lg, *args_t)
    np.testing.assert_array_equal(pt.transpose(0, 1, 3, 2), p)
    np.testing.assert_array_equal(labt.transpose(0, 2, 1), lab)


# ---- resampled form ---------------------------------------------------------------------------------------------------------
RESAMPLED = [(out, axis) for out in ((4, 7, 5), (6, 3, 9)) for axis in (-1, 0)]


def _golden_resize():
    return np.load(os.path.join(GOLDEN, "prob_resize_argmax.npz"))


@pytest.mark.parametrize("Cn", [3, 25, 33])
@pytest.mark.parametrize("out,axis", RESAMPLED)
@pytest.mark.parametrize("perm", [(0, 1, 2), (2, 0, 1)])
def test_resampled_box(ctx, Cn, out, axis, perm):
    """The box (3, 5, 4) of the 5 x 6 x 7 grid resampled to `out`, put at (2, 3, 0) of 8 x 10 x 9."""
    from boa_hip._lib import check
    grid, off, dims, lo, full = (5, 6, 7), (1, 0, 2), (3, 5, 4), (2, 3, 0), (8, 10, 9)
    z = _golden_resize()
    lg = z[f"logits_C{Cn}"].view(F16)
    assert lg.shape == (Cn, *grid)
    p, lab = _run(ctx, lg, off, dims, out, axis, lo, full, perm)
    check_against_reference(p, lab, lg, off, dims, out, axis, lo, full, perm, f"out {out} axis {axis} perm {perm}")
    # boa_resize_logits_argmax on the same input: the result of the commit before this kernel existed, bit for bit ...
    d_lg = ctx.from_numpy(np.ascontiguousarray(lg).view(np.uint16))
    d_lab = ctx.zeros(int(np.prod(out)))
    check(ctx.lib.boa_resize_logits_argmax(ctx.h, d_lg.vp, Cn, _i3(grid), _i3(off), _i3(dims), _i3(out), axis,
                                           LUT.ctypes.data_as(C.c_void_p), 0, d_lab.vp), "boa_resize_logits_argmax")
    arg = d_lab.download(tuple(out), np.uint8)
    d_lg.free()
    d_lab.free()
    np.testing.assert_array_equal(arg, z[f"labels_C{Cn}_{out[0]}x{out[1]}x{out[2]}_axis{axis}"])
    # ... and the labels taken from the probabilities equal it wherever the returned top two probabilities differ
    sl = tuple(slice(lo[d], lo[d] + out[d]) for d in range(3))
    inv = np.argsort(perm)
    pb = p.transpose([0] + [int(q) + 1 for q in inv])[(slice(None),) + sl]
    lb = lab.transpose(inv)[sl]
    top2 = np.sort(pb, axis=0)[-2:]
    distinct = top2[1] > top2[0]
    assert distinct.mean() > 0.5
    np.testing.assert_array_equal(lb[distinct], arg[distinct])


# ---- argument refusals ------------------------------------------------------------------------------------------------------
GOOD = dict(Cn=3, grid=(5, 6, 7), off=(1, 0, 2), dims=(3, 5, 4), out=None, axis=-1, lo=(2, 3, 0), full=(6, 9, 5), perm=(0, 1, 2))
BAD = {
    "C=0": dict(Cn=0), "C=256": dict(Cn=256), "C<0": dict(Cn=-1),
    "box leaves the logits grid": dict(dims=(3, 7, 4)), "negative pad offset": dict(off=(-1, 0, 2)),
    "offset past the grid": dict(off=(1, 0, 8)), "pad box sum overflows": dict(off=(2 ** 31 - 1, 0, 2)),
    "box leaves the pre-crop grid": dict(lo=(2, 5, 0)), "negative bbox_lo": dict(lo=(2, 3, -1)),
    "resampled box leaves the pre-crop grid": dict(out=(4, 7, 5)),
    "perm repeats": dict(perm=(0, 0, 1)), "perm out of range": dict(perm=(0, 1, 3)), "perm negative": dict(perm=(-1, 1, 2)),
    "slice_axis -2": dict(axis=-2), "slice_axis 3": dict(axis=3),
    "zero grid extent": dict(grid=(5, 0, 7)), "zero box extent": dict(dims=(3, 0, 4)), "zero out extent": dict(out=(3, 0, 4)),
    "zero full extent": dict(full=(6, 9, 0)), "negative full extent": dict(full=(-6, 9, 5)),
    "logits plane of 2^31 voxels": dict(grid=(2048, 2048, 512)), "output plane of 2^31 voxels": dict(full=(32768, 16384, 4096)),
    "output rows of 2^31 voxels": dict(full=(65536, 32768, 8)),
    "NULL grid_dims": dict(grid=None), "NULL bbox_lo": dict(lo=None), "NULL full_dims": dict(full=None), "NULL perm": dict(perm=None),
}


@pytest.mark.parametrize("name", list(BAD))
def test_refusals_launch_nothing(ctx, name):
    a = dict(GOOD, **BAD[name])
    n = 3 * 6 * 9 * 5
    d_lg = ctx.from_numpy(np.zeros((3, 5, 6, 7), np.uint16))
    d_prob = ctx.from_numpy(np.full(n, 0x7f7f7f7f, np.uint32))
    d_lab = ctx.from_numpy(np.full(6 * 9 * 5, 0x7f, np.uint8))
    try:
        rc = _call(ctx, d_lg, a["Cn"], a["grid"], a["off"], a["dims"], a["out"], a["axis"], a["lo"], a["full"], a["perm"], d_prob, LUT, d_lab)
        assert rc == BOA_EINVAL, name
        assert b"boa_logits_to_probabilities" in ctx.lib.boa_last_error()
        ctx.sync()
        assert (d_prob.download((n,), np.uint32) == 0x7f7f7f7f).all() and (d_lab.download((6 * 9 * 5,), np.uint8) == 0x7f).all()
    finally:
        for b in (d_lg, d_prob, d_lab):
            b.free()


def test_null_buffers_are_refused(ctx):
    d = ctx.zeros(3 * 6 * 9 * 5 * 4)
    a = GOOD
    for lg, prob in ((None, d), (d, None)):
        assert _call(ctx, lg, a["Cn"], a["grid"], a["off"], a["dims"], a["out"], a["axis"], a["lo"], a["full"], a["perm"], prob, None, None) == BOA_EINVAL
    assert ctx.lib.boa_logits_to_probabilities(None, d.vp, 3, _i3(a["grid"]), None, None, None, -1, _i3((0, 0, 0)), _i3(a["grid"]),
                                               _i3((0, 1, 2)), d.vp, None, None) == BOA_EINVAL
    d.free()


# ---- predictor --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(ctx):
    """A 3-class PlainConvUNet toy (patch 32^3, two stages, two folds of random weights) and the two G3 volumes: 40 x 36 x 33, and
    12 x 40 x 20, which the sliding window pads."""
    from boa_hip import plans
    pj, dj = plans.synthetic_plans(patch=(32, 32, 32), features=(32, 64), num_classes=3)
    geom = plans.model_config_from_plans(pj, dj).geometry
    blobs = [plans.weight_blob_from_state_dict(geom, plans.synthetic_state_dict(geom, seed=s)) for s in (3, 4)]
    z = np.load(os.path.join(GOLDEN, "g3_sliding_window.npz"))
    return geom, blobs, {"a": z["a_x"], "b": z["b_x"]}


@pytest.mark.parametrize("vol", ["a", "b"])
@pytest.mark.parametrize("nfolds", [1, 2])
def test_predictor_probabilities(ctx, toy, vol, nfolds):
    from boa_hip.predictor import HipPredictor
    geom, blobs, vols = toy
    x = vols[vol]
    assert x.shape[1:] == {"a": (40, 36, 33), "b": (12, 40, 20)}[vol]
    p = HipPredictor(ctx, geom, tile_step_size=0.5, max_batch=4)
    p.set_parameters(blobs[:nfolds])
    try:
        before = p.predict_segmentation(x, lut=LUT)
        lab, prob = p.predict_segmentation(x, lut=LUT, return_probabilities=True)
        after = p.predict_segmentation(x, lut=LUT, return_probabilities=False)
        logits = p.predict_logits_from_preprocessed_data(x) if nfolds > 1 else p.predict_sliding_window_return_logits(x)
    finally:
        p.close()
    assert logits.dtype == F16 and prob.dtype == np.float32 and prob.shape == logits.shape and lab.shape == x.shape[1:]
    p64 = S.softmax64(logits)
    S.assert_within_bound(prob, p64, 3, f"predictor volume {vol}, {nfolds} fold(s)")
    inv = np.full(256, -1)
    inv[LUT[:3]] = np.arange(3)
    S.assert_labels(inv[lab], prob, p64, 3, "predictor")
    # the default path: the same labels with the keyword left out and set to False, and those of the probabilities wherever the top
    # two differ
    np.testing.assert_array_equal(before, after)
    top2 = np.sort(prob, axis=0)[-2:]
    distinct = top2[1] > top2[0]
    assert distinct.mean() > 0.9
    np.testing.assert_array_equal(before[distinct], lab[distinct])


# ---- task -------------------------------------------------------------------------------------------------------------------
def _write_model(root, tid, name, nc, seed, tf):
    from boa_hip import model_store, plans
    pj, dj = plans.synthetic_plans(patch=(32, 32, 32), features=(32, 64), num_classes=nc, spacing=(1.5, 1.5, 1.5))
    pj["transpose_forward"] = list(tf)
    pj["transpose_backward"] = [int(v) for v in np.argsort(tf)]
    geom = plans.model_config_from_plans(pj, dj).geometry
    folder = model_store.write_model_folder(str(root), tid, name, "nnUNetTrainerNoMirroring", pj, dj, [plans.synthetic_state_dict(geom, seed=seed)])
    cfg = plans.load_model_folder(folder, "3d_fullres")
    blob = plans.weight_blob_from_state_dict(cfg.geometry, plans.load_checkpoint(os.path.join(folder, "fold_0", "checkpoint_final.pth")))
    return tid, cfg, [blob]


def _ct():
    """30 x 26 x 22 (x, y, z) at 3 mm with a zero border of 3 voxels: the nonzero box 24 x 20 x 16 lies strictly inside, and at the plans'
    1.5 mm it is 48 x 40 x 32 (tile origins on multiples of 8)."""
    from boa_hip.synthetic import ct_phantom
    ct = np.zeros((30, 26, 22), dtype=np.int16)
    inner = ct_phantom((24, 20, 16), seed=4).astype(np.int16)
    inner[inner == 0] = 1
    ct[3:27, 3:23, 3:19] = inner
    return ct, np.diag([3.0, 3.0, 3.0, 1.0])


def _load(path):
    with np.load(path) as z:
        assert z.files == ["probabilities"]
        return z["probabilities"]


@pytest.mark.parametrize("tf", [(0, 1, 2), (2, 0, 1)], ids=["identity", "tf201"])
def test_task_saves_probabilities_on_the_image_grid(ctx, tmp_path, tf):
    from boa_hip import nnunet_resample as nr
    from boa_hip._lib import check
    from boa_hip.task import SegmentationTask
    model = _write_model(tmp_path / "results", 301, "toy", 3, 11, tf)
    cfg = model[1]
    ct, aff = _ct()
    t = SegmentationTask(ctx, "toy", [model], resample=None, multimodel=False, max_batch=4)
    path = tmp_path / "out" / "s01.npz"
    path.parent.mkdir()
    try:
        plain = t.predict_image(ct, aff)
        seg = t.predict_image(ct, aff, save_probabilities=path)
        # the predictor-level reconstruction: transpose_forward, crop to nonzero, normalise, resample to the plans' spacing,
        # probabilities resampled back to the crop's grid -- then the crop revert and transpose_backward in numpy
        zyx = np.ascontiguousarray(ct.transpose(2, 1, 0))
        work = np.ascontiguousarray(zyx.transpose(tf))
        nzb = [(int(np.flatnonzero((work != 0).any(axis=tuple(a for a in range(3) if a != ax)))[0]),
                int(np.flatnonzero((work != 0).any(axis=tuple(a for a in range(3) if a != ax)))[-1]) + 1) for ax in range(3)]
        crop = np.ascontiguousarray(work[tuple(slice(a, b) for a, b in nzb)])
        shape = list(crop.shape)
        sp_t = [3.0, 3.0, 3.0]
        new_shape = nr.compute_new_shape(shape, sp_t, cfg.spacing)
        assert sorted(new_shape) == [32, 40, 48] and all(a > 0 and b < n for (a, b), n in zip(nzb, work.shape))
        ip = cfg.intensity_properties["0"]
        d_ct, vol, vol_r = ctx.from_numpy(crop), ctx.alloc(crop.size * 4), ctx.alloc(int(np.prod(new_shape)) * 4)
        check(ctx.lib.boa_ct_normalize(ctx.h, d_ct.vp, 0, vol.vp, crop.size, ip["mean"], ip["std"], ip["percentile_00_5"], ip["percentile_99_5"]))
        ax_in = nr.slice_axis_for(nr.checked_kwargs(cfg.extra, "data"), sp_t, cfg.spacing)
        ax_out = nr.slice_axis_for(nr.checked_kwargs(cfg.extra, "probabilities"), cfg.spacing, sp_t)
        check(ctx.lib.boa_resize_skimage_f32(ctx.h, vol.vp, _i3(shape), vol_r.vp, _i3(new_shape), 3, ax_in))
        prob = ctx.alloc(3 * crop.size * 4)
        t.parts[0][2].predict_probabilities_device(vol_r, new_shape, prob, None, resample_to=(shape, ax_out))
        pc = prob.download((3, *shape), np.float32)
        for b in (d_ct, vol, vol_r, prob):
            b.free()
    finally:
        t.close()
    want = np.zeros((3, *work.shape), dtype=np.float32)
    want[0] = 1.0
    want[(slice(None),) + tuple(slice(a, b) for a, b in nzb)] = pc
    tb = [int(v) for v in np.argsort(tf)]
    want = want.transpose([0] + [i + 1 for i in tb])
    got = _load(path)
    assert got.dtype == np.float32 and got.shape == (3, 22, 26, 30)                      # [C, z, y, x] of the image
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # outside the nonzero box: (1, 0, 0)
    outside = np.ones((22, 26, 30), bool)
    outside[3:19, 3:23, 3:27] = False
    assert (got[0][outside] == 1).all() and (got[1:][:, outside] == 0).all()
    assert np.abs(got.sum(axis=0) - 1).max() < 1e-5 and (got[:, ~outside] < 1).any()
    with open(path.with_suffix(".pkl"), "rb") as f:
        props = pickle.load(f)
    assert props == {"spacing": [3.0, 3.0, 3.0], "shape_before_cropping": tuple(work.shape), "bbox_used_for_cropping": [list(b) for b in nzb],
                     "shape_after_cropping_and_before_resampling": tuple(shape)}
    # the labels are the first maximum of the saved probabilities, and those of the run without the keyword wherever the top two differ
    pxyz = got.transpose(0, 3, 2, 1)
    np.testing.assert_array_equal(seg, S.first_max(pxyz).astype(np.uint8))
    top2 = np.sort(pxyz, axis=0)[-2:]
    distinct = top2[1] > top2[0]
    assert distinct[3:27, 3:23, 3:19].mean() > 0.9
    np.testing.assert_array_equal(seg[distinct], plain[distinct])
    assert len(np.unique(seg)) > 1


def test_two_model_task_leaves_the_second_models_array_and_sharded_tasks_refuse(ctx, tmp_path):
    from boa_hip.task import SegmentationTask
    m1 = _write_model(tmp_path / "results", 291, "part1", 3, 21, (0, 1, 2))
    m2 = _write_model(tmp_path / "results", 292, "part2", 4, 22, (0, 1, 2))
    luts = {291: np.array([0, 5, 6], np.uint8), 292: np.array([0, 7, 8, 9], np.uint8)}
    ct, aff = _ct()
    paths = {k: tmp_path / f"{k}.npz" for k in ("both", "first", "second")}
    segs = {}
    for key, models in (("both", [m1, m2]), ("first", [m1]), ("second", [m2])):
        t = SegmentationTask(ctx, "total", models, resample=None, multimodel=True, max_batch=4, part_luts=luts)
        try:
            segs[key] = t.predict_image(ct, aff, save_probabilities=paths[key])
            if key == "both":
                plain = t.predict_image(ct, aff)
                for attr in ("shard", "model_shard"):
                    setattr(t, attr, object())
                    with pytest.raises(NotImplementedError):
                        t.predict_image(ct, aff, save_probabilities=tmp_path / "never.npz")
                    setattr(t, attr, None)
                assert not (tmp_path / "never.npz").exists()
        finally:
            t.close()
    both, first, second = (_load(paths[k]) for k in ("both", "first", "second"))
    assert both.shape == (4, 22, 26, 30) and first.shape == (3, 22, 26, 30)
    np.testing.assert_array_equal(both.view(np.uint32), second.view(np.uint32))
    # the merge of `total` is unchanged: later parts overwrite, background never does
    np.testing.assert_array_equal(segs["both"], np.where(segs["second"] != 0, segs["second"], segs["first"]))
    assert set(np.unique(segs["both"])) <= {0, 5, 6, 7, 8, 9} and len(np.unique(segs["both"])) > 2
    top = [np.sort(a.transpose(0, 3, 2, 1), axis=0)[-2:] for a in (first, second)]
    distinct = (top[0][1] > top[0][0]) & (top[1][1] > top[1][0])
    np.testing.assert_array_equal(segs["both"][distinct], plain[distinct])
