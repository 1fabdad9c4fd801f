"""Cases of get_basic_statistics (TS/statistics.py:91-141) shared by tests/golden/make_golden_statistics.py (which runs the reference's own
function on them), tests/test_basic_statistics_reference_cpu.py and the GPU tests.  Label volumes use the ids of the `total` class map."""
import numpy as np

TASK = "total"


def blocks(shape=(22, 19, 25), seed=1):
    """Boxes of `total` labels: some inside, some reaching into the 3-voxel border slabs on one face each, one label absent; HU noise."""
    rng = np.random.default_rng(seed)
    seg = np.zeros(shape, np.uint8)
    seg[4:9, 5:9, 6:11] = 1            # spleen, inside (even count)
    seg[10:13, 4:7, 4:7] = 2           # kidney_right, inside (odd count: 27)
    seg[3:7, 10:14, 14:19] = 5         # liver, first index 3 on axis 0: the first voxel that does not touch
    seg[2:5, 3:5, 12:14] = 6           # stomach, index 2 on axis 0: touches
    seg[14:19, 12:16, 3:8] = 7         # pancreas, last index 18 = dim - 4 on axis 0: inside
    seg[14:20, 3:6, 12:15] = 10        # lung_upper_lobe_left, last index 19 = dim - 3 on axis 0: touches
    seg[9:12, 15:17, 12:16] = 51       # heart, last index 16 = dim - 3 on axis 1: touches
    seg[9:12, 9:12, 21:23] = 52        # aorta, last index 22 = dim - 3 on axis 2: touches
    seg[9:12, 9:12, 3:5] = 90          # brain, first index 3 on axis 2: inside
    seg[8, 8, 8] = 117                 # the last label of the map, one voxel
    ct = rng.integers(-1024, 1500, size=shape).astype(np.int16)
    ct[seg == 2] = rng.integers(-3, 4, size=27)            # small values around zero: the rounding of the mean
    return seg, ct


def thin(shape=(5, 30, 40), seed=2):
    """Axis 0 shorter than twice the border: every voxel lies in `mask[:3]` or `mask[-3:]`, every present label touches."""
    rng = np.random.default_rng(seed)
    seg = np.zeros(shape, np.uint8)
    seg[2, 10:20, 10:30] = 5
    seg[1:4, 4:8, 4:8] = 1
    return seg, rng.integers(-200, 300, size=shape).astype(np.int16)


def float_ct(seed=3):
    """A float-valued CT (`get_fdata()` of a scaled file): the reference truncates with astype(np.int16)."""
    seg, ct = blocks(seed=seed)
    rng = np.random.default_rng(seed)
    return seg, ct.astype(np.float64) + rng.uniform(-0.99, 0.99, size=ct.shape)


def extremes(shape=(12, 12, 16)):
    """int16 extremes under one label (sum and mean of -32768 / 32767), the normalisation range at its widest that int16 holds."""
    seg = np.zeros(shape, np.uint8)
    seg[4:8, 4:8, 4:12] = 3
    ct = np.zeros(shape, np.int16)
    ct[4:8, 4:8, 4:8] = 32767
    ct[4:8, 4:8, 8:12] = -32768
    seg[4:6, 8, 4:7] = 4
    ct[4:6, 8, 4:7] = [[-5, 7, 7], [9, -32768, 32767]]
    return seg, ct


ZOOMS = {"blocks": (0.78125, 0.78125, 1.5), "thin": (1.5, 1.5, 1.5), "float_ct": (0.9765625, 0.9765625, 2.5), "extremes": (1.0, 0.7, 3.3),
         "narrow": (1.5, 1.5, 1.5)}


def narrow(seed=4):
    """HU range below 32768 wide (the reference normalises in int16: `ct - ct.min()` must not wrap) with a plain mixture of labels."""
    seg, _ = blocks(seed=seed)
    rng = np.random.default_rng(seed)
    return seg, rng.integers(-1024, 3071, size=seg.shape).astype(np.int16)


VOLUMES = {"blocks": blocks, "thin": thin, "float_ct": float_ct, "extremes": extremes, "narrow": narrow}

# (volume, keyword arguments of get_basic_statistics)
CALLS = [
    ("blocks", dict(metric="mean", exclude_masks_at_border=True)),
    ("blocks", dict(metric="mean", exclude_masks_at_border=False)),
    ("blocks", dict(metric="median", exclude_masks_at_border=True)),
    ("blocks", dict(metric="median", exclude_masks_at_border=False)),
    ("blocks", dict(metric="mean", exclude_masks_at_border=True, roi_subset=["liver", "heart", "kidney_right", "colon"])),
    ("blocks", dict(metric="median", exclude_masks_at_border=False, roi_subset=["sternum", "spleen"])),
    ("thin", dict(metric="mean", exclude_masks_at_border=True)),
    ("thin", dict(metric="median", exclude_masks_at_border=False)),
    ("float_ct", dict(metric="mean", exclude_masks_at_border=False)),
    ("float_ct", dict(metric="median", exclude_masks_at_border=True)),
    ("extremes", dict(metric="mean", exclude_masks_at_border=False)),
    ("extremes", dict(metric="median", exclude_masks_at_border=False)),
    ("narrow", dict(metric="mean", exclude_masks_at_border=True, normalized_intensities=True)),
    ("narrow", dict(metric="median", exclude_masks_at_border=False, normalized_intensities=True)),
    ("narrow", dict(metric="mean", exclude_masks_at_border=False, normalized_intensities=True, roi_subset=["spleen", "aorta"])),
]


def call_key(k):
    vol, kw = CALLS[k]
    return f"{k:02d}.{vol}"


_CACHE = {}


def volume(name):
    """(seg uint8, ct, float32 zooms) of a case, built once per process"""
    if name not in _CACHE:
        seg, ct = VOLUMES[name]()
        _CACHE[name] = (seg, ct, np.asarray(ZOOMS[name], dtype=np.float32))
    return _CACHE[name]
