"""`higher_order_resampling` without a GPU: the host decision (`boa_hip.nnunet_resample.onehot_plan`), the numpy references
(tests/onehot_reference.py) and the per-voxel arithmetic of csrc/resample_onehot.h on the host.

The fixtures tests/golden/g_onehot_*.npz come from the reference's own `resample_img_nnunet` / `resample_patient(None, seg, ...)`
(tests/golden/make_golden_onehot.py).  skimage is not installed where they were made: `skimage.transform.resize` was replaced by
`oracle.nnunet_resample.skimage_resize`, the project's documented stand-in (scipy.ndimage.zoom(grid_mode=True, mode="nearest") +
clip).  They pin the spacing arithmetic, the axis choice, the slice loop and the label rule, not skimage itself.

The header is compiled into tools/onehot_host.cpp with -ffp-contract=off and the address and undefined-behaviour sanitizers and run
as a child process."""
import glob
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import onehot_reference as R
from boa_hip import nnunet_resample as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "g_onehot_*.npz")))
NAMES = [os.path.basename(p)[len("g_onehot_"):-len(".npz")] for p in GOLDEN]
WANT = {"iso_x2", "nondyadic", "down", "noise", "sepz_target_ax0", "sepz_target_ax1", "sepz_target_ax2", "sepz_original",
        "two_equal_axes"}


def _load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _plan(g):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return nr.onehot_plan(g["seg"].shape, g["target"], g["zooms"])


def test_every_case_of_the_generator_is_there():
    assert set(NAMES) == WANT
    seen = {(bool(_load(p)["do_separate_z"]), int(_load(p)["axis"])) for p in GOLDEN}
    assert seen == {(False, -1), (True, 0), (True, 1), (True, 2)}


@pytest.mark.parametrize("path", GOLDEN, ids=NAMES)
def test_plan_reproduces_the_reference_decision(path):
    g = _load(path)
    sep, axis, new_shape = _plan(g)
    assert sep == bool(g["do_separate_z"])
    assert (-1 if axis is None else axis) == int(g["axis"])
    assert list(new_shape) == g["new_shape"].tolist()
    t = g["target"].tolist()
    assert list(new_shape) == [t[2], t[0], t[1]]


def test_two_equal_axes_warn_and_fall_back():
    g = _load(GOLDEN[NAMES.index("two_equal_axes")])
    with pytest.warns(UserWarning, match="axis has len 2"):
        sep, axis, _ = nr.onehot_plan(g["seg"].shape, g["target"], g["zooms"])
    assert (sep, axis) == (False, None)


def test_threshold_is_strictly_above_three():
    # original spacing (x, y, z) = (1, 1, 3): ratio exactly 3 -> no separate z; the next float32 above 3 -> separate z on axis 0
    # of [z, x, y].  The target shape keeps the zoom at 1.25 so the target spacing (0.8, 0.8, 2.4) has the same ratio.
    shape, target = (8, 8, 4), (10, 10, 5)
    assert nr.onehot_plan(shape, target, (1.0, 1.0, 3.0))[:2] == (False, None)
    above = np.nextafter(np.float32(3.0), np.float32(4.0))
    assert nr.onehot_plan(shape, target, (1.0, 1.0, above))[:2] == (True, 0)
    # the same on the TARGET spacing: isotropic original 1.5, zoom (2, 2, 2/3) -> target (0.75, 0.75, 2.25): ratio exactly 3
    assert nr.onehot_plan((6, 6, 6), (12, 12, 4), (1.5, 1.5, 1.5))[:2] == (False, None)
    # zoom (2, 2, 0.5) -> target (0.75, 0.75, 3.0): ratio 4
    assert nr.onehot_plan((6, 6, 6), (12, 12, 3), (1.5, 1.5, 1.5))[:2] == (True, 0)
    # x coarse -> axis 1, y coarse -> axis 2 of [z, x, y]
    assert nr.onehot_plan((6, 6, 6), (3, 12, 12), (1.5, 1.5, 1.5))[:2] == (True, 1)
    assert nr.onehot_plan((6, 6, 6), (12, 3, 12), (1.5, 1.5, 1.5))[:2] == (True, 2)


def test_every_level_takes_the_keyword_default_off():
    import inspect
    from boa_hip import task, totalseg
    for fn in (task.SegmentationTask.predict_image, task.run_roi_subset, task.run_with_body_crop, task.run_cascade_task,
               totalseg.TotalSegmentatorHip.predict):
        assert inspect.signature(fn).parameters["higher_order_resampling"].default is False, fn.__qualname__
    assert inspect.signature(task.SegmentationTask.predict_roi_subset).parameters["options"].kind is inspect.Parameter.VAR_KEYWORD


def test_the_spacing_is_taken_as_float32():
    """get_zooms() is float32: 3.0000001 as a Python float is 3.0 in the header, hence no separate z."""
    assert nr.onehot_plan((8, 8, 4), (10, 10, 5), (1.0, 1.0, 3.0000001))[:2] == (False, None)


@pytest.mark.parametrize("path", GOLDEN, ids=NAMES)
def test_loop_reference_reproduces_the_golden_output(path):
    g = _load(path)
    got = R.resample_xyz(g["seg"], g["target"], int(g["axis"]), R.resample_seg_loop)
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, g["out"])


@pytest.mark.parametrize("path", GOLDEN, ids=NAMES)
def test_tap_formulation_reproduces_the_golden_output(path):
    g = _load(path)
    np.testing.assert_array_equal(R.resample_xyz(g["seg"], g["target"], int(g["axis"]), R.resample_seg_taps), g["out"])


def _volumes():
    """(name, seg [z, x, y], new shape, sep axis): random volumes, white noise among them (8 distinct labels in most cells)."""
    rng = np.random.default_rng(7)
    out = []
    for k, (shp, new) in enumerate([((5, 6, 7), (10, 12, 14)), ((5, 6, 7), (20, 24, 28)), ((6, 5, 4), (13, 9, 11)),
                                     ((9, 8, 7), (4, 5, 3)), ((1, 6, 5), (1, 11, 9)), ((4, 1, 5), (9, 3, 5)), ((2, 2, 2), (7, 7, 7)),
                                     ((6, 4, 8), (3, 2, 4))]):      # halving: x = 0.5 on every axis, exact ties at 0.5
        noise = rng.integers(0, 256, size=shp).astype(np.uint8)
        few = np.array([0, 1, 127, 255], dtype=np.uint8)[rng.integers(0, 4, size=shp)]
        checker = (np.indices(shp).sum(0) % 2 * 200 + 3).astype(np.uint8)
        for nm, seg in (("noise", noise), ("few", few), ("checker", checker)):
            for sep in (-1, 0, 1, 2):
                tgt = list(new)
                if sep >= 0 and k % 2:
                    tgt[sep] = shp[sep]               # no change of extent along the separate axis
                out.append((f"{nm}-{shp}-{tuple(tgt)}-sep{sep}", seg, tuple(tgt), sep))
    return out


VOLUMES = _volumes()


@pytest.mark.parametrize("name,seg,new,sep", VOLUMES, ids=[v[0] for v in VOLUMES])
def test_tap_formulation_equals_the_loop(name, seg, new, sep):
    np.testing.assert_array_equal(R.resample_seg_taps(seg, new, sep), R.resample_seg_loop(seg, new, sep))


def test_eight_distinct_labels_in_one_cell():
    seg = np.arange(1, 9, dtype=np.uint8).reshape(2, 2, 2) * 31
    for new in ((4, 4, 4), (7, 5, 6), (8, 8, 8)):
        got = R.resample_seg_taps(seg, new)
        np.testing.assert_array_equal(got, R.resample_seg_loop(seg, new))
        assert len(np.unique(got)) >= 8                  # every label survives somewhere; 0 appears where no mask reaches 0.5


# ---------------------------------------------------------------------------------------------- the header on the host
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("onehot_host") / "onehot_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "body-and-organ-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tools", "onehot_host.cpp"), "-o", str(exe)])

    def ask(*requests, status=0):
        r = subprocess.run([str(exe)], input="\n".join(requests) + "\n", capture_output=True, text=True)
        assert r.returncode == status, r.stderr[-4000:]
        return [np.array(ln.split(), dtype=np.uint64) for ln in r.stdout.splitlines()]
    return ask


def _host_volume(host, seg_xyz, out_xyz, sep_ref):
    sep = -1 if sep_ref is None or sep_ref < 0 else (2, 0, 1)[sep_ref]
    req = "vol {} {} {} {} {} {} {} {}".format(*seg_xyz.shape, *out_xyz, sep, " ".join(map(str, seg_xyz.ravel().tolist())))
    return host(req)[0].astype(np.uint8).reshape(out_xyz)


def test_host_tables_equal_the_blueprint(host):
    for n_in, n_out in [(5, 10), (5, 20), (13, 20), (20, 7), (1, 1), (1, 9), (9, 1), (4096, 3)]:
        for active in (1, 0):
            got = host(f"tab {n_in} {n_out} {active}")[0].reshape(n_out, 4)
            i0, i1, w0, w1 = R.axis_taps(n_in, n_out, bool(active))
            np.testing.assert_array_equal(got[:, 0], i0)
            np.testing.assert_array_equal(got[:, 1], i1)
            np.testing.assert_array_equal(got[:, 2], np.ascontiguousarray(w0, dtype=np.float64).view(np.uint64))
            np.testing.assert_array_equal(got[:, 3], np.ascontiguousarray(w1, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("path", GOLDEN, ids=NAMES)
def test_host_voxels_reproduce_the_golden_output(host, path):
    g = _load(path)
    np.testing.assert_array_equal(_host_volume(host, g["seg"], tuple(g["target"].tolist()), int(g["axis"])), g["out"])


def test_host_voxels_on_noise_checkerboard_and_equal_dims(host):
    for name, seg, new, sep in VOLUMES[::5]:
        got = _host_volume(host, R.from_ref(seg), (new[1], new[2], new[0]), sep)
        np.testing.assert_array_equal(got, R.from_ref(R.resample_seg_loop(seg, new, sep)), err_msg=name)
    seg = np.random.default_rng(1).integers(0, 256, size=(3, 4, 5)).astype(np.uint8)
    np.testing.assert_array_equal(_host_volume(host, seg, seg.shape, -1), seg)


def test_host_requests_outside_the_admitted_ranges_end_the_program(host):
    for bad in ("tab 0 1 1", "tab 1 4097 1", "tab 3 3 2", "vol 1 1 1 1 1 1 3 0", "vol 1 1 1 1 1 1 -2 0", "vol 2 1 1 1 1 1 -1 0",
                "vol 1 1 1 1 1 1 -1 256", "vol 1 1 1 0 1 1 -1 0", "vol 1 1 1 1 1 1 -1 x", "what"):
        host(bad, status=2)
