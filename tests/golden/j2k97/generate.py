"""Writes the irreversible (9/7) JPEG 2000 fixtures of this folder: codestreams written by OpenJPEG through Pillow with
irreversible=True, and OpenJPEG's own decode of each, which is what the decoder has to reproduce bit for bit (`meta` records the
OpenJPEG version).  The smallest cases at which each thing can go wrong: 2 x 2 with one level, two layers in LRCP, a signed
stream, odd sizes at every level with values to 65535, precincts with RPCL, three resolutions with 16 x 16 blocks, one resolution
(no transform), a checkerboard that clamps at both ends, and two 512 x 512 slices of the CT phantom with Pillow's defaults.
For phantom frames the file holds `residual_<k>` = decoded - source; the source is regenerated from the seed
(boa_hip.synthetic.ct_phantom), as for the fixtures of tests/golden/j2k.
Pillow refuses some tiny shapes with many resolutions ("broken data stream"); of the shapes below it refused none: 2 x 2 is
written with two resolutions, all others with Pillow's six or what the case names.
A file whose content would not change is left alone.
Run from the repository root, where Pillow with OpenJPEG imports:  python tests/golden/j2k97/generate.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "body-and-organ-analysis_amd")]

import j2k97_fixtures as FX  # noqa: E402
import j2k_writer as JW  # noqa: E402
from boa_hip import jpeg2000 as J  # noqa: E402

RATES = "rates"
PHANTOM = dict(shape=[512, 512, 2], seed=20260928, offset=1024)
CROP = [128, 128]                                 # top-left corner of the 129 x 97 crop of phantom slice 0
CASES = [  # file, name, shape, bits, signed, content, Pillow options
    ("small", "2x2_u16_1level", (2, 2), 16, False, "random", dict(num_resolutions=2)),
    ("small", "40x33_u8_lrcp_2layers", (40, 33), 8, False, "smooth", dict(progression="LRCP", quality_layers=[20, 4],
                                                                        quality_mode=RATES)),
    ("small", "40x33_s8_random", (40, 33), 8, True, "random", {}),
    ("small", "61x75_u16_noise", (61, 75), 16, False, "random", {}),
    ("small", "40x33_u16_1res", (40, 33), 16, False, "smooth", dict(num_resolutions=1)),
    ("small", "40x33_u16_checkerboard_rate20", (40, 33), 16, False, "checkerboard", dict(quality_layers=[20], quality_mode=RATES)),
    ("crop", "129x97_u16_ct_rate10_rpcl_precincts_cb32", (129, 97), 16, False, "phantomcrop", dict(
        quality_layers=[10], quality_mode=RATES, progression="RPCL", precinct_size=(64, 64), codeblock_size=(32, 32))),
    ("crop", "129x97_u16_ct_rate10_3res_cb16", (129, 97), 16, False, "phantomcrop", dict(
        quality_layers=[10], quality_mode=RATES, num_resolutions=3, codeblock_size=(16, 16))),
    ("phantom0", "512x512_ct_phantom_z0", (512, 512), 16, False, "phantom0", {}),
    ("phantom1", "512x512_ct_phantom_z1", (512, 512), 16, False, "phantom1", {}),
]


def smooth(shape, bits, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    hi = (1 << bits) - 1
    v = hi * (0.5 + 0.35 * np.sin(xx / 7.0 + seed) * np.cos(yy / 11.0)) + rng.normal(0, hi / 400.0, shape)
    return np.clip(np.round(v), 0, hi).astype(np.int64)


def random(shape, bits, seed):
    return np.random.default_rng(seed).integers(0, 1 << bits, shape)


def checkerboard(shape, bits, seed):
    """Squares of 2 x 2 samples, 0 and full scale: at rate 20 the ringing overshoots the range at both ends (one-sample squares
    do not: they are damped)."""
    yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    return ((yy // 2 + xx // 2) & 1) * ((1 << bits) - 1)


CONTENT = dict(smooth=smooth, random=random, checkerboard=checkerboard)


def main():
    from PIL import features
    files = {}
    for i, (fname, name, shape, bits, signed, content, kw) in enumerate(CASES):
        meta = dict(name=name, rows=shape[0], cols=shape[1], bits=bits, signed=signed, openjpeg=features.version("jpg_2000"),
                    options={k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()})
        if content.startswith("phantom"):
            meta["phantom"] = dict(PHANTOM, z=0, crop=CROP) if content == "phantomcrop" else dict(PHANTOM, z=int(content[-1]))
            src = FX.phantom_source(meta["phantom"], *shape)
        else:
            src = CONTENT[content](shape, bits, 100 + i) - ((1 << (bits - 1)) if signed else 0)
        assert src.shape == shape
        try:
            stream = FX.stream_of(src, bits, signed, **kw)
        except OSError as e:                                  # Pillow's "broken data stream" on a tiny shape
            print(f"{name}: refused by Pillow ({e})")
            continue
        got = JW.openjpeg_decode(stream)
        assert got.shape == shape
        fr = J.parse_frame(stream, rows=shape[0], cols=shape[1], name=name)
        assert fr.transform == 0 and fr.levels == kw.get("num_resolutions", 6) - 1 and fr.signed == signed, name
        lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
        if content == "checkerboard":                         # the clamp of the last stage is reached at both ends
            import j2k97_reference as M
            plane, ok = M.reconstruct(fr)
            v = np.rint(plane) + (0 if signed else 1 << (bits - 1))
            assert ok and v.min() < lo and v.max() > hi and got.min() == lo and got.max() == hi, (name, v.min(), v.max())
        if "noise" in name:                                   # values up to the top of the range
            assert src.max() > 65500 and got.max() > 65500, name
        store = files.setdefault(fname, {"meta": []})
        k = len(store["meta"])
        store["meta"].append(meta)
        store[f"stream_{k}"] = np.frombuffer(stream, dtype=np.uint8)
        if "phantom" in meta:
            res = got - src
            assert np.abs(res).max() < 1 << 15
            store[f"residual_{k}"] = res.astype(np.int16)
        else:
            store[f"decoded_{k}"] = got.astype(f"{'i' if signed else 'u'}{bits // 8}")
        print(f"{name}: {len(stream)} bytes, {len(fr.blocks)} blocks, {int((got != src).sum())} of {src.size} samples differ from the "
              f"source, max |difference| {int(np.abs(got - src).max())}")
    total = 0
    for fname, store in files.items():
        store["meta"] = np.array(json.dumps(store["meta"]))
        path = os.path.join(HERE, f"{fname}.npz")
        if os.path.exists(path):
            with np.load(path) as g:
                if set(g.files) == set(store) and all(np.array_equal(g[k], store[k]) and g[k].dtype == np.asarray(store[k]).dtype
                                                      for k in store):
                    print(f"{path}: unchanged")
                    total += os.path.getsize(path)
                    continue
        np.savez_compressed(path, **store)
        size = os.path.getsize(path)
        assert size <= 256 * 1024, (path, size)
        total += size
        print(f"{path}: {size} bytes")
    assert total <= 1 << 20, total


if __name__ == "__main__":
    main()
