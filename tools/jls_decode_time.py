"""JPEG-LS series decode on the device (csrc/jls.hip) on a 512 x 512 x 600 series:
  * the two 512 x 512 slices of the seeded CT-like phantom that CharLS encoded (tests/golden/jls/charls_phantom{0,1}.npz; stored =
    HU + 1024, 12 bit, NEAR 0, SPIFF header), cycled to 600 slices: no JPEG-LS encoder is assumed where this runs;
  * the compressed size, the host read and marker parse time of all frames;
  * the batched decode call (device events around jpeg_ls.decode_frames: the upload of the scans, the kernel, the status read-back
    and the output download), one wave per frame and one lane per frame alternated; the kernels alone: run with --decode-only
    under `rocprofv3 --kernel-trace --stats`;
  * get_image_info wall time on the JPEG-LS series against the uncompressed series of the same volume, alternated (medians).
Prints one JSON line and writes it to --out.
  python tools/jls_decode_time.py --out profiles/jls_decode.json
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/jls_decode_time.py --decode-only
--charls LIB: no device; CharLS itself (libcharls through ctypes, which releases the interpreter lock) decoding the same 600
frames on this host with 1 and 16 threads."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jls")
sys.path[:0] = [ROOT, os.path.join(ROOT, "body-and-organ-analysis_amd"), os.path.join(ROOT, "tests")]


def _streams():
    return [np.load(os.path.join(GOLDEN, f"charls_phantom{i}.npz"))["stream_phantom"].tobytes() for i in range(2)]


def _write(args):
    folder, z, sl, stream = args
    import jls_writer as W
    from dicom_writer import write_slice
    ipp = (-200.0, -180.0, 1.25 * z)
    p = os.path.join(folder, "IM%04d.dcm" % z)
    if stream is not None:
        W.write_slice(p, sl, stream + b"\0" * (len(stream) % 2), bits_stored=12, ipp=ipp, instance=z + 1)
    else:
        write_slice(p, sl, bits_stored=12, ipp=ipp, instance=z + 1)
    return os.path.getsize(p)


def charls_times(lib_path, n, reps):
    import jls_writer
    generate = jls_writer.golden_generator()
    lib = generate.load(lib_path)
    streams = _streams()
    want = [generate.charls_decode(lib, s) for s in streams]
    jobs = [streams[z % 2] for z in range(n)]
    res = {"what": "CharLS decoding the same frames on this host (not the GPU machine's)", "slices": n, "host_cpus": os.cpu_count()}
    for threads in (1, 16):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=threads) as ex:
                out = list(ex.map(lambda s: generate.charls_decode(lib, s), jobs))
            ts.append(time.perf_counter() - t0)
            assert all(np.array_equal(o, want[z % 2]) for z, o in enumerate(out))
        res[f"charls_ms_{threads}_threads"] = {"median": round(1e3 * float(np.median(ts)), 1), "all": [round(1e3 * t, 1) for t in ts]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--io-reps", type=int, default=3, help="alternated repetitions of get_image_info per series")
    ap.add_argument("--decode-only", action="store_true", help="decode timing only (for a rocprofv3 run)")
    ap.add_argument("--charls", default=None, help="path of libcharls.so: time CharLS on this host instead, no device")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, size = a.slices, 512

    if a.charls:
        res, ok = charls_times(a.charls, n, a.reps), True
    else:
        import jls_writer
        generate = jls_writer.golden_generator()
        vol = generate.phantom_slices()
        stored = [vol[z].astype(np.int64) for z in generate.PHANTOM_Z]
        streams = _streams()
        tmp = tempfile.mkdtemp(prefix="jls_")
        res = {"what": "JPEG-LS series decode", "slices": n, "rows": size, "cols": size,
               "series": "slices 4 and 11 of boa_hip.synthetic.ct_phantom 512x512x16 + 1024, encoded by CharLS 2.2 (NEAR 0), "
                         f"cycled to {n}"}
        t0 = time.perf_counter()
        jobs = [(os.path.join(tmp, "jls"), z, stored[z % 2], streams[z % 2]) for z in range(n)]
        if not a.decode_only:
            jobs += [(os.path.join(tmp, "raw"), z, stored[z % 2], None) for z in range(n)]
        for d in {j[0] for j in jobs}:
            os.makedirs(d, exist_ok=True)
        with ProcessPoolExecutor(max_workers=a.workers) as ex:       # (CPU only: before this process opens the device)
            sizes = list(ex.map(_write, jobs, chunksize=8))
        res["write_s"] = round(time.perf_counter() - t0, 2)
        res["compressed_files_mb"] = round(sum(sizes[:n]) / 1e6, 1)
        res["uncompressed_pixels_mb"] = round(n * size * size * 2 / 1e6, 1)

        from boa_hip import dicom, jpeg_ls as JL
        from boa_hip.compute.inference import get_context
        files = dicom.series_file_names(os.path.join(tmp, "jls"))
        t0 = time.perf_counter()
        sl = [dicom.read_file(p) for p in files]
        t1 = time.perf_counter()
        frames = [JL.parse_frame(d["PixelData"], rows=size, cols=size, bits_stored=12, name=d["_path"]) for d in sl]
        t2 = time.perf_counter()
        res["host_read_s"] = round(t1 - t0, 3)
        res["host_parse_s"] = round(t2 - t1, 3)
        in_bytes = sum(len(f.data) for f in frames)
        res["scan_data_mb"] = round(in_bytes / 1e6, 2)
        res["bits_per_sample"] = round(8.0 * in_bytes / (n * size * size), 3)
        ctx = get_context("gpu")
        want = np.stack([stored[z % 2] for z in range(n)]).astype(np.uint16)
        times, ok = {"wave": [], "serial": []}, True
        for rep in range(a.reps + 1):                               # rep 0: warm-up (code objects, pool)
            for kind in ("wave", "serial"):
                ctx.timer_start(0)
                px, st = JL.decode_frames(ctx, frames, serial=kind == "serial")
                ms = ctx.timer_stop(0)
                ok = ok and bool((st == 0).all()) and bool(np.array_equal(px, want))
                if rep:
                    times[kind].append(ms)
        res["decoded_equal_source"] = ok
        for kind, ts in times.items():
            res[f"call_ms_{kind}"] = {"median": round(float(np.median(ts)), 3), "all": [round(t, 3) for t in ts]}
        res["note"] = ("call time = device events around decode_frames (scan upload, the kernel, the status read-back, the output "
                       "download); kernel times: rocprofv3 --kernel-trace --stats on --decode-only")
        if not a.decode_only:
            from boa_hip.compute.io import get_image_info
            io_t = {"jls": [], "uncompressed": []}
            for rep in range(a.io_reps):
                for kind, d in (("jls", "jls"), ("uncompressed", "raw")):
                    t0 = time.perf_counter()
                    get_image_info(os.path.join(tmp, d), os.path.join(tmp, "out_" + d))
                    io_t[kind].append(time.perf_counter() - t0)
            for kind, ts in io_t.items():
                res[f"get_image_info_{kind}_s"] = {"median": round(float(np.median(ts)), 3), "all": [round(t, 3) for t in ts]}
            res["get_image_info_ratio"] = round(float(np.median(io_t["jls"]) / np.median(io_t["uncompressed"])), 3)
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
