"""RLE Lossless series decode on the device (csrc/rle.hip) on a 512 x 512 x 600 series:
  * the seeded CT-like phantom (boa_hip.synthetic.ct_phantom, stored = HU + 1024), every slice encoded plane by plane by libtiff's
    PackBits encoder (through Pillow, which must report libtiff): the strips of a plane, in order, are one Annex G segment;
  * the compressed size, the host read and header parse time of all frames;
  * the batched decode call (device events around rle_lossless.decode_frames: the upload of the frames, the kernels, the status
    read-back and the output download), parallel and serial alternated; the kernels alone: run with --decode-only under
    `rocprofv3 --kernel-trace --stats`;
  * get_image_info wall time on the RLE series against the uncompressed series of the same volume, alternated (medians).
Prints one JSON line and writes it to --out.
  python tools/rle_decode_time.py --out profiles/rle_decode.json
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/rle_decode_time.py --decode-only"""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "body-and-organ-analysis_amd"), os.path.join(ROOT, "tests")]


def _packbits(plane):
    """uint8 [rows, cols] -> the plane's libtiff PackBits strips, concatenated."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(plane).save(buf, format="TIFF", compression="packbits")
    raw = buf.getvalue()
    tif = Image.open(io.BytesIO(raw))
    assert tif.tag_v2[259] == 32773
    return b"".join(raw[o:o + n] for o, n in zip(tif.tag_v2[273], tif.tag_v2[279]))


def _write(args):
    folder, z, sl, compressed = args
    import rle_writer as R
    from dicom_writer import write_slice
    ipp = (-200.0, -180.0, 1.25 * z)
    p = os.path.join(folder, "IM%04d.dcm" % z)
    if compressed:
        R.write_slice(p, sl, R.frame_of([_packbits(plane) for plane in R.planes_of(sl, 16)]), ipp=ipp, instance=z + 1)
    else:
        write_slice(p, sl, ipp=ipp, instance=z + 1)
    return os.path.getsize(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--io-reps", type=int, default=3, help="alternated repetitions of get_image_info per series")
    ap.add_argument("--chunk-bytes", type=int, default=1024)
    ap.add_argument("--decode-only", action="store_true", help="decode timing only (for a rocprofv3 run)")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from PIL import features
    if not features.check("libtiff"):
        sys.exit("this Pillow has no libtiff: no PackBits encoder")
    from boa_hip.synthetic import ct_phantom
    n, size = a.slices, 512
    stored = (ct_phantom((size, size, n)).transpose(2, 1, 0).astype(np.int32) + 1024).astype(np.int64)
    tmp = tempfile.mkdtemp(prefix="rle_")
    res = {"what": "RLE Lossless series decode", "slices": n, "rows": size, "cols": size, "chunk_bytes": a.chunk_bytes,
           "series": f"boa_hip.synthetic.ct_phantom 512x512x{n} + 1024, each byte plane encoded by libtiff PackBits (Pillow)"}
    t0 = time.perf_counter()
    jobs = [(os.path.join(tmp, "rle"), z, stored[z], True) for z in range(n)]
    if not a.decode_only:
        jobs += [(os.path.join(tmp, "raw"), z, stored[z], False) for z in range(n)]
    for d in {j[0] for j in jobs}:
        os.makedirs(d, exist_ok=True)
    with ProcessPoolExecutor(max_workers=a.workers) as ex:       # (CPU only: before this process opens the device)
        sizes = list(ex.map(_write, jobs, chunksize=8))
    res["encode_and_write_s"] = round(time.perf_counter() - t0, 2)
    res["compressed_files_mb"] = round(sum(sizes[:n]) / 1e6, 1)
    res["uncompressed_pixels_mb"] = round(n * size * size * 2 / 1e6, 1)

    from boa_hip import dicom, rle_lossless as RL
    from boa_hip.compute.inference import get_context
    files = dicom.series_file_names(os.path.join(tmp, "rle"))
    t0 = time.perf_counter()
    sl = [dicom.read_file(p) for p in files]
    t1 = time.perf_counter()
    frames = [RL.parse_frame(d["PixelData"], rows=size, cols=size, name=d["_path"]) for d in sl]
    t2 = time.perf_counter()
    res["host_read_s"] = round(t1 - t0, 3)
    res["host_parse_s"] = round(t2 - t1, 3)
    in_bytes = sum(len(f.data) for f in frames)
    seg_bytes = [[hi - lo for lo, hi in f.bounds] for f in frames]
    res["frame_data_mb"] = round(in_bytes / 1e6, 2)
    res["high_plane_mb"] = round(sum(s[0] for s in seg_bytes) / 1e6, 2)
    res["low_plane_mb"] = round(sum(s[1] for s in seg_bytes) / 1e6, 2)
    res["chunks"] = int(sum(-(-b // a.chunk_bytes) for s in seg_bytes for b in s))
    res["bits_per_sample"] = round(8.0 * in_bytes / (n * size * size), 3)
    ctx = get_context("gpu")
    want = (stored & 0xFFFF).astype(np.uint16)
    times, ok = {"parallel": [], "serial": []}, True
    for rep in range(a.reps + 1):                               # rep 0: warm-up (code objects, pool)
        for kind in ("parallel", "serial"):
            ctx.timer_start(0)
            px, st = RL.decode_frames(ctx, frames, serial=kind == "serial", chunk_bytes=a.chunk_bytes)
            ms = ctx.timer_stop(0)
            ok = ok and bool((st == 0).all()) and bool(np.array_equal(px, want))
            if rep:
                times[kind].append(ms)
    res["decoded_equal_source"] = ok
    for kind, ts in times.items():
        res[f"call_ms_{kind}"] = {"median": round(float(np.median(ts)), 3), "all": [round(t, 3) for t in ts]}
    res["output_gbps"] = round(n * size * size * 2 / float(np.median(times["parallel"])) / 1e6, 1)
    res["note"] = ("call time = device events around decode_frames (frame upload, the kernels, the status read-back, the output "
                   "download); kernel times: rocprofv3 --kernel-trace --stats on --decode-only")
    if not a.decode_only:
        from boa_hip.compute.io import get_image_info
        io_t = {"rle": [], "uncompressed": []}
        for rep in range(a.io_reps):
            for kind, d in (("rle", "rle"), ("uncompressed", "raw")):
                t0 = time.perf_counter()
                get_image_info(os.path.join(tmp, d), os.path.join(tmp, "out_" + d))
                io_t[kind].append(time.perf_counter() - t0)
        for kind, ts in io_t.items():
            res[f"get_image_info_{kind}_s"] = {"median": round(float(np.median(ts)), 3), "all": [round(t, 3) for t in ts]}
        res["get_image_info_ratio"] = round(float(np.median(io_t["rle"]) / np.median(io_t["uncompressed"])), 3)
    shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
