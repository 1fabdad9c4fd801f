"""Lossy DCT JPEG series decode on the device (csrc/jpeg_dct.hip) on a 512 x 512 x 600 series at P = 12 (transfer syntax .51):
  * the two committed phantom slices of tests/golden/jpeg_dct/phantom12.npz (boa_hip.synthetic.ct_phantom, stored = HU + 1024,
    encoded by libjpeg-turbo's 12-bit entry points at quality 90), cycled; every decoded slice is compared with libjpeg-turbo's
    own decode through the SHA-256 the fixture holds;
  * host read + marker parse time of all frames, compressed bytes and bits per sample;
  * the batched decode call (device events around jpeg_dct.decode_frames: the upload of the entropy-coded data and the tables,
    the entropy decode, the inverse DCT, the status read-back and the output download), with the parallel and with the serial
    entropy decoder; the kernels alone: run with --decode-only under `rocprofv3 --kernel-trace --stats`;
  * get_image_info wall time on the compressed series against the uncompressed series of the same pixels, alternated (medians).
Prints one JSON line and writes it to --out.
  python tools/jpeg_dct_decode_time.py --out profiles/jpeg_dct_decode.json
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/jpeg_dct_decode_time.py --decode-only"""
import argparse
import hashlib
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
    folder, z, sl, stream = args
    import ljpeg_writer as LW
    from dicom_writer import write_slice
    ipp = (-200.0, -180.0, 1.25 * z)
    p = os.path.join(folder, "IM%04d.dcm" % z)
    if stream is None:
        write_slice(p, sl, ipp=ipp, instance=z + 1, bits_stored=12)
    else:
        LW.write_compressed_slice(p, sl, stream, transfer_syntax="1.2.840.10008.1.2.4.51", ipp=ipp, instance=z + 1, bits_stored=12)
    return os.path.getsize(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--io-reps", type=int, default=3, help="alternated repetitions of get_image_info per series")
    ap.add_argument("--decode-only", action="store_true", help="decode timing only (for a rocprofv3 run)")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    n, size = a.slices, 512
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_dct", "phantom12.npz"))
    names = [str(v) for v in g["names"]]
    streams = [g["stream_" + v].tobytes() for v in names]
    digests = [str(g["sha256_" + v]) for v in names]
    res = {"what": "DCT JPEG (extended, P = 12) series decode", "slices": n, "rows": size, "cols": size,
           "series": "the two committed 512x512 phantom slices of tests/golden/jpeg_dct (libjpeg-turbo 12-bit, quality 90), cycled"}

    from boa_hip import dicom, jpeg_dct as J
    from boa_hip.compute.inference import get_context
    frames2 = [J.parse_frame(s, rows=size, cols=size, bits_stored=12, name=v) for s, v in zip(streams, names)]
    frames = [frames2[z % 2] for z in range(n)]
    in_bytes = sum(len(f.data) for f in frames)
    res["entropy_coded_mb"] = round(in_bytes / 1e6, 2)
    res["bits_per_sample"] = round(8.0 * in_bytes / (n * size * size), 3)
    ctx = get_context("gpu")
    ok = True
    px = None
    for kind, kw in (("parallel", {}), ("serial", {"serial": True})):
        times = []
        for rep in range(a.reps + 1):                               # rep 0: warm-up (code objects, pool)
            ctx.timer_start(0)
            px, st = J.decode_frames(ctx, frames, **kw)
            ms = ctx.timer_stop(0)
            ok = ok and bool((st == 0).all())
            if rep == 0:
                ok = ok and all(hashlib.sha256(px[z].astype("<u2").tobytes()).hexdigest() == digests[z] for z in (0, 1))
                ok = ok and all(np.array_equal(px[z], px[z % 2]) for z in range(2, n))
            else:
                times.append(ms)
        med = float(np.median(times))
        res[f"call_ms_{kind}"] = {"median": round(med, 3), "all": [round(t, 3) for t in times]}
    res["decoded_equal_libjpeg"] = ok
    res["output_gbps_parallel"] = round(n * size * size * 2 / res["call_ms_parallel"]["median"] / 1e6, 1)
    res["note"] = ("call time = device events around decode_frames (data and table uploads, the kernels, the status read-back, the "
                   "output download); kernel times: rocprofv3 --kernel-trace --stats on --decode-only")
    if not a.decode_only:
        tmp = tempfile.mkdtemp(prefix="jdct_")
        stored = px[:2].astype(np.int64)                            # libjpeg's pixels (checked above): the uncompressed series holds them
        t0 = time.perf_counter()
        jobs = [(os.path.join(tmp, "jpg"), z, stored[z % 2], streams[z % 2]) for z in range(n)]
        jobs += [(os.path.join(tmp, "raw"), z, stored[z % 2], None) for z in range(n)]
        for d in {j[0] for j in jobs}:
            os.makedirs(d, exist_ok=True)
        with ProcessPoolExecutor(max_workers=a.workers) as ex:
            sizes = list(ex.map(_write, jobs, chunksize=8))
        res["write_s"] = round(time.perf_counter() - t0, 2)
        res["compressed_files_mb"] = round(sum(sizes[:n]) / 1e6, 1)
        files = dicom.series_file_names(os.path.join(tmp, "jpg"))
        t0 = time.perf_counter()
        sl = [dicom.read_file(p) for p in files]
        t1 = time.perf_counter()
        [J.parse_frame(d["PixelData"], rows=size, cols=size, bits_stored=12, name=d["_path"]) for d in sl]
        t2 = time.perf_counter()
        res["host_read_s"] = round(t1 - t0, 3)
        res["host_parse_s"] = round(t2 - t1, 3)
        from boa_hip.compute.io import get_image_info
        io_t = {"jpeg": [], "uncompressed": []}
        for rep in range(a.io_reps):
            for kind, d in (("jpeg", "jpg"), ("uncompressed", "raw")):
                t0 = time.perf_counter()
                get_image_info(os.path.join(tmp, d), os.path.join(tmp, "out_" + d))
                io_t[kind].append(time.perf_counter() - t0)
        for kind, ts in io_t.items():
            res[f"get_image_info_{kind}_s"] = {"median": round(float(np.median(ts)), 3), "all": [round(t, 3) for t in ts]}
        res["get_image_info_ratio"] = round(res["get_image_info_jpeg_s"]["median"] / res["get_image_info_uncompressed_s"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
