"""Loading a .nii.gz: the host path (`nifti.load(path)`: one zlib call for a foreign file, --threads zlib calls for a file with this
project's member index) against the device inflate (csrc/inflate.hip, `nifti.load(path, ctx=ctx)`), on the int16 `ct_phantom` at
--size^3 written twice:
  foreign   one gzip member, zlib level 6 (what nibabel, ITK, dcm2niix write)
  indexed   this project's file (`nifti.save`: members of 4 MiB with the index field)
  * wall time of `nifti.load`, median of --reps, host and device alternated in this process after one warm-up of each;
  * that both paths return the same array;
  * inside the device path: upload of the file's bytes, the `boa_inflate_streams` call with the device-event times of its passes
    (find, count, store, windows, resolve), download of the payload; and the chunk / candidate / rejected / round counts.
Kernel times alone: run with --kernel-only under `rocprofv3 --kernel-trace --stats`, in a run of its own.
Prints one JSON line and writes it to --out.
  python tools/load_time.py --out profiles/r11_inflate.json
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/load_time.py --kernel-only"""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "body-and-organ-analysis_amd")]


def _breakdown(ctx, nifti, path, chunk_bytes):
    """The steps of `nifti.device_inflate` timed one by one (every step ends synchronised)."""
    with open(path, "rb") as f:
        raw = f.read()
    t0 = time.perf_counter()
    src = ctx.from_numpy(np.frombuffer(raw, dtype=np.uint8))
    ctx.sync()
    upload = time.perf_counter() - t0
    src.free()
    t0 = time.perf_counter()
    out, info = nifti.device_inflate(ctx, raw, chunk_bytes=chunk_bytes)
    whole = time.perf_counter() - t0
    n = 0 if out is None else out.nbytes
    buf = ctx.alloc(max(n, 16))
    t0 = time.perf_counter()
    buf.download((n,), np.uint8)
    download = time.perf_counter() - t0
    buf.free()
    return {"file_bytes": len(raw), "payload_bytes": n, "upload_ms": round(upload * 1e3, 2), "download_ms": round(download * 1e3, 2),
            "device_inflate_ms": round(whole * 1e3, 2), "passes_ms": {k: round(v, 2) for k, v in info["ms"].items()},
            "info": {k: info[k] for k in ("chunks", "candidates", "rejected", "rounds", "live", "streams", "host")},
            "status": sorted(set(info["status"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--depth", type=int, default=0, help="z extent (default: --size)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=8, help="host inflate threads of the indexed file")
    ap.add_argument("--chunk-bytes", type=int, default=0, help="compressed bytes per chunk (default: the library's)")
    ap.add_argument("--kernel-only", action="store_true", help="two device loads per file, nothing else (for a rocprofv3 run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from boa_hip import nifti, synthetic
    from boa_hip.compute.inference import get_context
    ctx = get_context("gpu")
    tmp = tempfile.mkdtemp(prefix="load_time_")
    aff = np.diag([-1.5, -1.5, 1.5, 1.0])
    shape = (a.size, a.size, a.depth or a.size)
    vol = synthetic.ct_phantom(shape, seed=5)
    paths = {"foreign": os.path.join(tmp, "foreign.nii.gz"), "indexed": os.path.join(tmp, "indexed.nii.gz")}
    nifti.save(os.path.join(tmp, "plain.nii"), vol, aff)
    with open(os.path.join(tmp, "plain.nii"), "rb") as f, open(paths["foreign"], "wb") as g:
        g.write(gzip.compress(f.read(), 6))
    nifti.save(paths["indexed"], vol, aff, threads=a.threads)
    chunk = a.chunk_bytes or None
    if chunk:
        real = nifti.device_inflate
        nifti.device_inflate = lambda c, raw, chunk_bytes=None: real(c, raw, chunk_bytes=chunk)
    res = {"what": "nifti.load of an int16 CT: zlib on the host vs the device inflate", "shape": list(shape), "host_threads": a.threads,
           "reps": a.reps, "chunk_bytes": chunk or int(ctx.lib.boa_inflate_default_chunk()), "files": {}}
    ok = True
    for name, path in paths.items():
        runs = {"host": lambda: nifti.load(path, threads=a.threads), "device": lambda: nifti.load(path, threads=a.threads, ctx=ctx)}
        if a.kernel_only:
            runs["device"]()
            runs["device"]()
            continue
        times = {k: [] for k in runs}
        got = {}
        for rep in range(a.reps + 1):                       # rep 0: warm-up (code objects, pools, page cache)
            for k, fn in runs.items():
                t0 = time.perf_counter()
                got[k] = fn()[0]
                if rep:
                    times[k].append(time.perf_counter() - t0)
        same = bool((got["host"] == got["device"]).all() and (got["host"] == vol).all())
        r = {f"{k}_s": {"median": round(float(np.median(ts)), 4), "all": [round(t, 4) for t in ts]} for k, ts in times.items()}
        r["equal"] = same
        r["host_over_device_time"] = round(float(np.median(times["host"]) / np.median(times["device"])), 3)
        r["device_breakdown"] = _breakdown(ctx, nifti, path, chunk)
        ok = ok and same and not r["device_breakdown"]["info"]["host"]
        res["files"][name] = r
    res["ok"] = ok
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
