"""Saving uint8 label volumes as .nii.gz: the CPU path (zlib level 1 on --threads host threads, what `nifti.save` does without a
context) against the device encoder (csrc/deflate.hip, `nifti.save(..., ctx=ctx)`), on the three label phantoms of
boa_hip.synthetic at --size^3:
  * wall time of `nifti.save`, median of --reps, the paths alternated in this process after one warm-up of each:
      cpu                the volume is a host array (what the file-level callers hold today)
      cpu_from_device    the volume is on the device: download, then the CPU path
      device_from_host   host array -> upload -> device encoder
      device             the volume is on the device in file order -> device encoder, nothing but compressed bytes comes back
  * output sizes of both encoders, and that both files decompress to the same bytes;
  * inside the device path: upload, the `boa_deflate_members` call (device events: table upload, the three kernels, the offset /
    CRC read-back), download of the compressed bytes, container + file write.
Kernel times alone: run with --kernel-only under `rocprofv3 --kernel-trace --stats`, in a run of its own.
Prints one JSON line and writes it to --out.
  python tools/save_time.py --out profiles/r09_deflate.json
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/save_time.py --kernel-only"""
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

PHANTOMS = ("total", "regions", "parts")


def _breakdown(ctx, nifti, vol, path):
    """The steps of `nifti.save(path, vol, aff, ctx=ctx)` for a host array, timed one by one (every step ends synchronised)."""
    t = [time.perf_counter()]
    buf, addr, nbytes, row = nifti._device_body(ctx, vol)
    t.append(time.perf_counter())
    import ctypes as C
    from boa_hip import _lib
    mb = nifti._GZ_BLOCK
    cap = int(ctx.lib.boa_deflate_bound(nbytes, mb))
    n_mem = max(1, -(-nbytes // mb))
    offs, crcs = (C.c_size_t * (n_mem + 1))(), (C.c_uint32 * n_mem)()
    out = ctx.alloc(cap)
    ctx.timer_start(0)
    _lib.check(ctx.lib.boa_deflate_members(ctx.h, C.c_void_p(addr), nbytes, mb, row, out.vp, cap, offs, crcs), "boa_deflate_members")
    call_ms = ctx.timer_stop(0)
    t.append(time.perf_counter())
    comp = memoryview(out.download((int(offs[n_mem]),), np.uint8))
    t.append(time.perf_counter())
    with open(path, "wb") as f:
        nifti.write_wrapped_members(f, [(comp[offs[m]:offs[m + 1]], int(crcs[m]), min(mb, nbytes - m * mb)) for m in range(n_mem)])
    t.append(time.perf_counter())
    out.free()
    buf.free()
    d = np.diff(t) * 1e3
    return {"upload_ms": round(d[0], 2), "encode_call_ms": round(d[1], 2), "encode_call_device_events_ms": round(call_ms, 2),
            "download_compressed_ms": round(d[2], 2), "container_and_write_ms": round(d[3], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=8, help="host deflate threads of the CPU path")
    ap.add_argument("--phantoms", default=",".join(PHANTOMS))
    ap.add_argument("--kernel-only", action="store_true", help="two device saves per phantom and nothing else (for a rocprofv3 run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from boa_hip import nifti, synthetic
    from boa_hip.compute.inference import get_context
    from boa_hip.devarray import DevArray
    ctx = get_context("gpu")
    tmp = tempfile.mkdtemp(prefix="save_time_")
    aff = np.diag([-1.5, -1.5, 1.5, 1.0])
    shape = (a.size,) * 3
    res = {"what": "nifti.save of uint8 label volumes: zlib level 1 on host threads vs the device deflate encoder", "shape": list(shape),
           "cpu_threads": a.threads, "reps": a.reps, "member_bytes": nifti._GZ_BLOCK, "phantoms": {}}
    ok = True
    for name in a.phantoms.split(","):
        vol = getattr(synthetic, f"label_phantom_{name}")(shape)
        d_vol = DevArray.from_numpy(ctx, np.ascontiguousarray(vol.transpose(2, 1, 0))).transpose((2, 1, 0))    # file order on the device
        paths = {k: os.path.join(tmp, f"{name}_{k}.nii.gz") for k in ("cpu", "cpu_from_device", "device_from_host", "device")}
        runs = {
            "cpu": lambda: nifti.save(paths["cpu"], vol, aff, threads=a.threads),
            "cpu_from_device": lambda: nifti.save(paths["cpu_from_device"], d_vol.download(), aff, threads=a.threads),
            "device_from_host": lambda: nifti.save(paths["device_from_host"], vol, aff, ctx=ctx),
            "device": lambda: nifti.save(paths["device"], d_vol, aff, ctx=ctx),
        }
        if a.kernel_only:
            runs["device"]()
            runs["device"]()
            d_vol.free()
            continue
        times = {k: [] for k in runs}
        for rep in range(a.reps + 1):                       # rep 0: warm-up (code objects, pools, page cache)
            for k, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                if rep:
                    times[k].append(time.perf_counter() - t0)
        r = {f"{k}_s": {"median": round(float(np.median(ts)), 4), "all": [round(t, 4) for t in ts]} for k, ts in times.items()}
        raw = {k: open(p, "rb").read() for k, p in paths.items()}
        want = gzip.decompress(raw["cpu"])
        same = all(gzip.decompress(raw[k]) == want for k in ("device_from_host", "device"))
        ok = ok and same and raw["device"] == raw["device_from_host"]
        r.update({"payload_bytes": int(vol.size), "cpu_file_bytes": len(raw["cpu"]), "device_file_bytes": len(raw["device"]),
                  "device_over_cpu_size": round(len(raw["device"]) / len(raw["cpu"]), 3), "decompressed_equal": same,
                  "cpu_over_device_time": round(float(np.median(times["cpu"]) / np.median(times["device"])), 2),
                  "cpu_from_device_over_device_time": round(float(np.median(times["cpu_from_device"]) / np.median(times["device"])), 2),
                  "device_from_host_breakdown": _breakdown(ctx, nifti, vol, os.path.join(tmp, f"{name}_b.nii.gz"))})
        res["phantoms"][name] = r
        d_vol.free()
        for p in paths.values():
            os.remove(p)
    res["ok"] = ok
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
