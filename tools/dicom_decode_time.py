"""JPEG Lossless series decode on the device (csrc/jpeg_ll.hip): a seeded CT-like 512 x 512 x 600 series (boa_hip.synthetic
.ct_phantom, stored = HU + 1024) encoded with predictor 1 by tests/ljpeg_writer.py, then
  * the batched decode of all frames, parallel and serial decoders alternated in this process (device-event time of the
    `boa_ljpeg_decode` call: table uploads + kernel + status read-back; kernel time alone: run with --decode-only under
    `rocprofv3 --kernel-trace --stats`), output GB/s and compressed-input GB/s;
  * get_image_info wall time on the compressed series against the uncompressed series of the same volume, alternated.
Prints one JSON line and writes it to --out.
  python tools/dicom_decode_time.py --out profiles/dicom_decode_r07.json
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/dicom_decode_time.py --decode-only --slices 600"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "body-and-organ-analysis_amd"), os.path.join(ROOT, "tests")]


def _write(args):
    folder, z, sl, compressed = args
    import ljpeg_writer as W
    from dicom_writer import write_slice
    ipp = (-200.0, -180.0, 1.25 * z)
    p = os.path.join(folder, "IM%04d.dcm" % z)
    if compressed:
        W.write_compressed_slice(p, sl, W.encode(sl, precision=16, predictor=1), ipp=ipp, instance=z + 1)
    else:
        write_slice(p, sl, ipp=ipp, instance=z + 1)
    return os.path.getsize(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=600)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5, help="alternated repetitions of each decoder")
    ap.add_argument("--io-reps", type=int, default=3, help="alternated repetitions of get_image_info per series")
    ap.add_argument("--subseq-bytes", type=int, default=128)
    ap.add_argument("--decode-only", action="store_true", help="decode timing only (for a rocprofv3 run)")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from boa_hip.synthetic import ct_phantom
    hu = ct_phantom((a.size, a.size, a.slices)).transpose(2, 1, 0)            # (z, y, x)
    stored = (hu.astype(np.int32) + 1024).astype(np.uint16)
    tmp = tempfile.mkdtemp(prefix="ljpeg_")
    res = {"what": "JPEG Lossless (predictor 1) series decode", "slices": a.slices, "rows": a.size, "cols": a.size,
           "subseq_bytes": a.subseq_bytes}
    t0 = time.perf_counter()
    jobs = [(os.path.join(tmp, "jpg"), z, stored[z], True) for z in range(a.slices)]
    if not a.decode_only:
        jobs += [(os.path.join(tmp, "raw"), z, stored[z], False) for z in range(a.slices)]
    for d in {j[0] for j in jobs}:
        os.makedirs(d, exist_ok=True)
    with ProcessPoolExecutor(max_workers=a.workers) as ex:       # (CPU only: before this process opens the device)
        sizes = list(ex.map(_write, jobs, chunksize=8))
    res["encode_and_write_s"] = round(time.perf_counter() - t0, 2)
    res["compressed_files_mb"] = round(sum(sizes[:a.slices]) / 1e6, 1)

    from boa_hip import dicom, jpeg_lossless as J
    from boa_hip.compute.inference import get_context
    files = dicom.series_file_names(os.path.join(tmp, "jpg"))
    t0 = time.perf_counter()
    sl = [dicom.read_file(p) for p in files]
    frames = [J.parse_frame(d["PixelData"], rows=a.size, cols=a.size, name=d["_path"]) for d in sl]
    res["host_read_parse_s"] = round(time.perf_counter() - t0, 3)
    in_bytes = sum(len(f.data) for f in frames)
    out_bytes = a.slices * a.size * a.size * 2
    res["entropy_coded_mb"] = round(in_bytes / 1e6, 2)
    res["bits_per_sample"] = round(8.0 * in_bytes / (a.slices * a.size * a.size), 3)
    ctx = get_context("gpu")
    want = stored.astype(np.uint16)
    times = {"parallel": [], "serial": []}
    ok = True
    for rep in range(a.reps + 1):                               # rep 0: warm-up (code objects, pool)
        for mode in ("parallel", "serial"):
            ctx.timer_start(0)
            px, st = J.decode_frames(ctx, frames, serial=mode == "serial", subseq_bytes=a.subseq_bytes)
            ms = ctx.timer_stop(0)
            ok = ok and bool((st == 0).all()) and bool(np.array_equal(px, want))
            if rep:
                times[mode].append(ms)
    res["decoded_equal_source"] = ok
    for mode, ts in times.items():
        med = float(np.median(ts))
        res[f"{mode}_call_ms"] = {"median": round(med, 3), "all": [round(t, 3) for t in ts]}
        res[f"{mode}_output_gbps"] = round(out_bytes / med / 1e6, 1)
        res[f"{mode}_input_gbps"] = round(in_bytes / med / 1e6, 2)
    res["serial_over_parallel"] = round(float(np.median(times["serial"]) / np.median(times["parallel"])), 2)
    res["note"] = ("call time = device events around boa_ljpeg_decode (uploads of the frame / segment / subsequence / table "
                   "arrays, the kernel, the status read-back); the compressed bytes are uploaded before it")
    if not a.decode_only:
        from boa_hip.compute.io import get_image_info
        io_t = {"compressed": [], "uncompressed": []}
        for rep in range(a.io_reps):
            for kind, d in (("compressed", "jpg"), ("uncompressed", "raw")):
                t0 = time.perf_counter()
                get_image_info(os.path.join(tmp, d), os.path.join(tmp, "out_" + d))
                io_t[kind].append(time.perf_counter() - t0)
        for kind, ts in io_t.items():
            res[f"get_image_info_{kind}_s"] = {"median": round(float(np.median(ts)), 3), "all": [round(t, 3) for t in ts]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
