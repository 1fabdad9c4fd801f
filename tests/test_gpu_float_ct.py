"""GPU, product surface: measurements and body composition on CTs that are not int16-exact (float-valued, scaled, out of the
int16 range).  Such volumes take the float64 statistics path; the oracle (numpy on the same float64 values) is the reference.
Counts, volumes, min / max / median / percentiles, masks and tissue maps are exact; mean, std, cnr and mean HU per tissue are
fp64 sums in another order than numpy's and are held to rtol 1e-9.  The phantoms keep that bar meaningful: every
measured region has |mean| >= mean|x| / 100 and std >= 1, and numpy's own mean agrees with the exactly rounded `math.fsum / n`
to 1e-12 on every region (asserted below)."""
import json
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXACT_KEYS = ("present", "volume_ml", "min_hu", "max_hu", "median_hu", "25th_percentile_hu", "75th_percentile_hu")
FLOAT_KEYS = ("mean_hu", "std_hu", "cnr", "autochthon_mean", "autochthon_std")
RTOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


def _plain(d):
    return json.loads(json.dumps(d, default=float))


def _cmp(a, b, float_keys, path=""):
    """Same structure; leaves under a key in `float_keys` to rtol 1e-9, every other leaf identical."""
    if isinstance(a, dict):
        assert set(a) == set(b), (path, set(a) ^ set(b))
        for k in a:
            _cmp(a[k], b[k], float_keys, f"{path}/{k}")
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _cmp(x, y, float_keys, f"{path}[{i}]")
    elif a is None or b is None or isinstance(a, (bool, str)):
        assert a == b, (path, a, b)
    elif path.rsplit("/", 1)[-1] in float_keys:
        assert np.isclose(a, b, rtol=RTOL, atol=0), (path, a, b)
    else:
        assert a == b, (path, a, b)


# ---- a `total` phantom (z, y, x) ---------------------------------------------------------------------------------
SHAPE = (24, 40, 48)
SPACING = (0.8, 0.75, 2.0)     # sitk order (x, y, z)


def _total_labels():
    from boa_hip import label_maps
    from boa_hip import measurements as M
    lm = label_maps.measurement_label_map("total")
    seg = np.zeros(SHAPE, np.uint8)
    seg[2:22, 22:36, 4:20] = lm["autochthon_left"]
    seg[2:22, 22:36, 28:44] = lm["autochthon_right"]
    seg[2:22, 4:18, 18:30] = lm["aorta"]
    seg[4:10, 18:22, 21:27] = lm["spleen"]
    left = [nm for nm in M.LUNG_MASKS if nm.endswith("left")]
    right = [nm for nm in M.LUNG_MASKS if nm.endswith("right")]
    for nm, (z0, z1) in zip(left, [(2, 11), (12, 22)]):
        seg[z0:z1, 4:16, 2:14] = lm[nm]
    for nm, (z0, z1) in zip(right, [(2, 8), (9, 15), (16, 22)]):
        seg[z0:z1, 4:16, 34:46] = lm[nm]
    return seg, lm


def _total_hu(seg, lm, rng):
    """HU (float64, not yet fractional): soft tissue noise, homogeneous muscle / aorta outside the fat window (the 6^3 erosion
    leaves voxels), lungs around the fat window, a fat pocket inside the left autochthon."""
    from boa_hip import measurements as M
    hu = rng.normal(40.0, 120.0, size=SHAPE)
    for nm in ("autochthon_left", "autochthon_right", "aorta"):
        sel = seg == lm[nm]
        hu[sel] = rng.normal(60.0 if nm != "aorta" else 180.0, 12.0, size=int(sel.sum()))
    for nm in M.LUNG_MASKS:
        sel = seg == lm[nm]
        hu[sel] = rng.normal(-130.0, 70.0, size=int(sel.sum()))
    hu[10:13, 27:30, 10:13] = -100.0
    return hu


def _assert_reference_is_stable(ct, seg, lm):
    """The bar of 1e-9 is far above the reference's own rounding on these regions."""
    for nm, label in lm.items():
        x = ct[seg == label]
        if x.size == 0:
            continue
        mean = math.fsum(x) / x.size
        assert abs(np.mean(x) - mean) <= 1e-12 * abs(mean), nm
        assert abs(mean) >= math.fsum(np.abs(x)) / x.size / 100 and np.std(x) >= 1.0, nm


def _measure_files(ctx, tmp_path, ct_xyz, seg_zyx, affine, cnr=True):
    """compute_measurements on ct.nii.gz + total.nii.gz -> (dict, ct_pfav array in file order, loaded CT values (z,y,x))."""
    from boa_hip import nifti
    from boa_hip.compute.measurements import compute_measurements
    seg_dir = tmp_path / "seg"
    seg_dir.mkdir(exist_ok=True)
    if ct_xyz is not None:
        nifti.save(tmp_path / "ct.nii.gz", ct_xyz, affine)
    nifti.save(seg_dir / "total.nii.gz", np.ascontiguousarray(seg_zyx.transpose(2, 1, 0)), affine)
    got = compute_measurements(tmp_path / "ct.nii.gz", seg_dir, ["total"], cnr_adjustment=cnr, ctx=ctx)
    data, _, hdr = nifti.load(tmp_path / "ct.nii.gz")
    pfav = nifti.load(seg_dir / "ct_pfav.nii.gz")[0]
    return got, pfav, np.ascontiguousarray(nifti.fdata(data, hdr).transpose(2, 1, 0)), tuple(float(v) for v in hdr.get_zooms())


def _check_against_oracle(got, pfav, ct_zyx, seg, lm, spacing):
    from oracle import measurements as OM
    want, wfat = OM.total_measurements(ct_zyx, seg, lm, spacing, cnr_adjustment=True)
    assert want["info"]["autochthon_mean"] is not None                     # the erosion left voxels: cnr is exercised
    assert want["cnr_adjusted"]["aorta"]["present"] and want["segmentations"]["total"]["ct_pfav_lungs"]["present"]
    np.testing.assert_array_equal(pfav, wfat.transpose(2, 1, 0))
    _cmp(_plain(got), _plain(want), FLOAT_KEYS)


AFF = np.diag([SPACING[0], SPACING[1], SPACING[2], 1.0])


def test_c1_compute_measurements_on_a_float64_nifti(ctx, tmp_path):
    seg, lm = _total_labels()
    ct = np.round(_total_hu(seg, lm, np.random.default_rng(5)), 2) + 0.3125      # fractional HU
    _assert_reference_is_stable(ct, seg, lm)
    got, pfav, loaded, spacing = _measure_files(ctx, tmp_path, np.ascontiguousarray(ct.transpose(2, 1, 0)), seg, AFF)
    np.testing.assert_array_equal(loaded, ct)
    _check_against_oracle(got, pfav, ct, seg, lm, spacing)


@pytest.mark.parametrize("kind", ["float32", "int32"])
def test_c4_float32_and_out_of_range_int32_niftis(ctx, tmp_path, kind):
    seg, lm = _total_labels()
    hu = _total_hu(seg, lm, np.random.default_rng(6))
    if kind == "float32":
        ct = (np.round(hu, 1) + 0.25).astype(np.float32)
    else:
        ct = np.round(hu).astype(np.int32)
        ct[seg == lm["spleen"]] += 40000                                   # above the int16 range
        assert ct.max() > 32767
    got, pfav, loaded, spacing = _measure_files(ctx, tmp_path, np.ascontiguousarray(ct.transpose(2, 1, 0)), seg, AFF)
    assert loaded.dtype == np.float64
    np.testing.assert_array_equal(loaded, ct.astype(np.float64))
    _assert_reference_is_stable(loaded, seg, lm)
    _check_against_oracle(got, pfav, loaded, seg, lm, spacing)


def test_c4_dicom_series_with_a_fractional_rescale(ctx, tmp_path):
    """RescaleSlope 0.5 / RescaleIntercept -10.25: the DICOM reader hands over float64; get_image_info -> compute_measurements."""
    from dicom_writer import write_series
    from boa_hip import nifti
    from boa_hip.compute.io import get_image_info
    seg, lm = _total_labels()
    hu = _total_hu(seg, lm, np.random.default_rng(7))
    stored = np.clip(np.round((hu + 10.25) * 2.0), -30000, 30000).astype(np.int16)     # HU = 0.5 * stored - 10.25
    write_series(tmp_path / "dcm", stored, signed=True, slope=0.5, intercept=-10.25, bits_stored=16, spacing=(0.75, 0.8), dz=2.0)
    path, _ = get_image_info(tmp_path / "dcm", tmp_path)
    data, affine, hdr = nifti.load(path)
    assert data.dtype == np.float64
    ct = np.ascontiguousarray(nifti.fdata(data, hdr).transpose(2, 1, 0))
    assert ct.shape == SHAPE and (ct != np.round(ct)).any()
    _assert_reference_is_stable(ct, seg, lm)
    (tmp_path / "ct.nii.gz").write_bytes(path.read_bytes())
    got, pfav, loaded, spacing = _measure_files(ctx, tmp_path, None, seg, affine)
    np.testing.assert_array_equal(loaded, ct)
    _check_against_oracle(got, pfav, ct, seg, lm, spacing)


def test_non_finite_voxels_are_refused_by_file_name(ctx, tmp_path):
    from boa_hip import nifti
    from boa_hip.compute.measurements import compute_measurements
    seg, _ = _total_labels()
    ct = np.full(SHAPE[::-1], 30.5)
    ct[3, 4, 5] = np.nan
    nifti.save(tmp_path / "bad.nii.gz", ct, AFF)
    (tmp_path / "seg").mkdir()
    nifti.save(tmp_path / "seg" / "total.nii.gz", np.ascontiguousarray(seg.transpose(2, 1, 0)), AFF)
    with pytest.raises(ValueError, match=r"bad\.nii\.gz.*non-finite"):
        compute_measurements(tmp_path / "bad.nii.gz", tmp_path / "seg", ["total"], cnr_adjustment=True, ctx=ctx)


# ---- body composition ----------------------------------------------------------------------------------------------
BCA_SHAPE = (12, 40, 44)       # file axis order (x, y, z)
BCA_AFF = np.diag([1.25, 1.25, 5.0, 1.0])      # RAS: the LPS reload flips two axes


def _bca_volumes(rng):
    """(regions, parts) in file order: nested boxes of body regions, torso / extremity parts; CT noise is added by the caller."""
    regions = np.zeros(BCA_SHAPE, np.uint8)
    regions[1:11, 2:38, :] = 1                 # subcutaneous tissue
    regions[2:10, 5:35, :] = 2                 # muscle
    regions[3:6, 8:32, 2:42] = 3               # abdominal cavity: 40 slices of 5 mm
    regions[6:9, 8:32, 2:42] = 4               # thoracic cavity next to it (the groups need slices that hold both)
    regions[6:9, 12:28, 10:38] = 9             # mediastinum
    regions[7:9, 16:24, 20:30] = 7             # pericardium
    regions[2:4, 18:22, :] = 5                 # bone
    parts = np.zeros(BCA_SHAPE, np.uint8)
    parts[regions > 0] = 1
    parts[:, :8, :] = 2
    parts[regions == 0] = 0
    return regions, parts


def _bca_hu(rng):
    hu = rng.normal(-60.0, 90.0, size=BCA_SHAPE)
    hu[rng.random(BCA_SHAPE) < 0.02] = -29.5   # between the adipose and the muscle window
    return hu


def _run_pipe(ctx, ct, regions, parts, median):
    from boa_hip.pipeline import BcaPipelineHip
    pipe = BcaPipelineHip(ctx, None, None)
    try:
        return pipe.run(ct, BCA_AFF, done_parts=parts, done_regions=regions, median_filtering=median)
    finally:
        pipe.close()


@pytest.mark.parametrize("median", [False, True])
def test_c2_bca_post_network_stages_on_a_float_ct(ctx, median):
    """Given (already post-processed) region and part volumes: LPS reload, tissue map, slice tables, group statistics."""
    from boa_hip import pipeline
    from oracle import bca as obca
    rng = np.random.default_rng(8)
    regions, parts = _bca_volumes(rng)
    ct = np.round(_bca_hu(rng), 2) + 0.125
    out = _run_pipe(ctx, ct, regions, parts, median)
    ct_l, spacing = pipeline.to_lps_zyx(ct, BCA_AFF)
    rg_l, _ = pipeline.to_lps_zyx(regions, BCA_AFF)
    pt_l, _ = pipeline.to_lps_zyx(parts, BCA_AFF)
    ref_t = obca.subclassify_tissues(ct_l, rg_l, median_filtering=median, slice_axis=0)
    np.testing.assert_array_equal(out["tissues"], pipeline.from_lps_zyx(ref_t, BCA_AFF))
    if median:
        assert (ref_t != obca.subclassify_tissues(ct_l, rg_l)).any()
    assert (ref_t[(ct_l == -29.5) & (rg_l == 2)] == 0).all() or median
    ref = obca.bca_measurements_json(ct_l, rg_l, pt_l, ref_t, spacing, None)
    for k in range(1, 8):                       # the bar is meaningful: no tissue's HU sum cancels
        x = ct_l[ref_t == k]
        if x.size:
            assert abs(math.fsum(x)) >= math.fsum(np.abs(x)) / 100 and abs(np.mean(x) - math.fsum(x) / x.size) <= 1e-12 * abs(np.mean(x))
    got = _plain(out["bca_measurements"])
    want = _plain(ref)
    # slice volumes are count x constant and the describe() statistics of those columns follow pandas' arithmetic: identical;
    # mean HU per tissue is the fp64 sum
    _cmp(got["slices"], want["slices"], ())
    _cmp(got["slices_no_extremities"], want["slices_no_extremities"], ())
    _cmp(got["body_parts"], want["body_parts"], ())
    assert set(got["aggregated"]) == set(want["aggregated"]) and len(want["aggregated"]) >= 5
    for grp, w in want["aggregated"].items():
        g = got["aggregated"][grp]
        for key in ("num_slices", "min_slice_idx", "max_slice_idx"):
            assert g[key] == w[key]
        for tab in ("measurements", "measurements_no_extremities"):
            for col, stats in w[tab].items():
                for name, v in stats.items():
                    x = g[tab][col][name]
                    if v is None:
                        assert x is None, (grp, tab, col, name)
                    elif name == "mean_hu":
                        assert np.isclose(x, v, rtol=RTOL, atol=0), (grp, tab, col, x, v)
                    else:
                        assert x == v, (grp, tab, col, name, x, v)


def test_c3_float_path_equals_int16_path_on_an_int16_ct(ctx, monkeypatch):
    """One int16 phantom through today's path and, with BOA_STATS_FLOAT=1, through the float path: everything that is exact is
    identical, the floating-point sums agree to 1e-9."""
    from boa_hip import measurements as M
    seg, lm = _total_labels()
    ct = np.round(_total_hu(seg, lm, np.random.default_rng(9))).astype(np.int16)
    _assert_reference_is_stable(ct.astype(np.float64), seg, lm)
    rng = np.random.default_rng(10)
    regions, parts = _bca_volumes(rng)
    bct = np.round(_bca_hu(rng)).astype(np.int16)
    monkeypatch.delenv("BOA_STATS_FLOAT", raising=False)
    a_meas, a_fat = M.total_measurements(ctx, ct, seg, lm, SPACING, cnr_adjustment=True)
    a_bca = {m: _run_pipe(ctx, bct, regions, parts, m) for m in (False, True)}
    monkeypatch.setenv("BOA_STATS_FLOAT", "1")
    calls = []
    orig = M.group_stats_f64
    monkeypatch.setattr(M, "group_stats_f64", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    b_meas, b_fat = M.total_measurements(ctx, ct, seg, lm, SPACING, cnr_adjustment=True)
    assert calls                                                        # the float path ran
    b_bca = {m: _run_pipe(ctx, bct, regions, parts, m) for m in (False, True)}
    np.testing.assert_array_equal(a_fat, b_fat)
    assert a_meas["info"]["autochthon_mean"] is not None and a_meas["cnr_adjusted"]["aorta"]["present"]
    _cmp(_plain(b_meas), _plain(a_meas), FLOAT_KEYS)
    for m in (False, True):
        np.testing.assert_array_equal(a_bca[m]["tissues"], b_bca[m]["tissues"])
        assert (a_bca[m]["tissues"] > 0).any()
        _cmp(_plain(b_bca[m]["bca_measurements"]), _plain(a_bca[m]["bca_measurements"]), ("mean_hu",))
