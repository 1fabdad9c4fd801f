"""Saving volumes as .nii.gz: the CPU path (zlib level 1 on --threads host threads, what `nifti.save` does without a
context) against the device encoder (csrc/deflate.hip, `nifti.save(..., ctx=ctx)`) in its --modes (fixed: fixed Huffman codes;
dynamic: `dynamic=True`), on the three uint8 label phantoms of boa_hip.synthetic and the int16 `ct_phantom` ("ct") at --size^3:
  * wall time of `nifti.save`, median of --reps, the paths alternated in this process after one warm-up of each:
      cpu                       the volume is a host array (what the file-level callers hold today)
      cpu_from_device           the volume is on the device: download, then the CPU path
      device_from_host_<mode>   host array -> upload -> device encoder
      device_<mode>             the volume is on the device in file order -> device encoder, nothing but compressed bytes comes back
  * output sizes of both encoders, and that both files decompress to the same bytes;
  * inside the device path, per mode: upload, the `boa_deflate_members2` call (device events: table upload, the three kernels, the offset /
    CRC read-back), download of the compressed bytes, container + file write.
Kernel times alone: run with --kernel-only under `rocprofv3 --kernel-trace --stats`, in a run of its own.
Prints one JSON line and writes it to --out.
  python tools/save_time.py --out profiles/r10_deflate_dynamic.json
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

PHANTOMS = ("total", "regions", "parts", "ct")
MODES = ("fixed", "dynamic")


def _breakdown(ctx, nifti, vol, path, dynamic):
    """The steps of `nifti.save(path, vol, aff, ctx=ctx, dynamic=dynamic)` for a host array, timed one by one (every step ends
    synchronised)."""
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
    near, flags = (vol.dtype.itemsize, _lib.BOA_DEFLATE_DYNAMIC) if dynamic else (1, 0)
    _lib.check(ctx.lib.boa_deflate_members2(ctx.h, C.c_void_p(addr), nbytes, mb, row, near, flags, out.vp, cap, offs, crcs),
               "boa_deflate_members2")
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
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--kernel-only", action="store_true", help="two device saves per phantom and mode, nothing else (for a rocprofv3 run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from boa_hip import nifti, synthetic
    from boa_hip.compute.inference import get_context
    from boa_hip.devarray import DevArray
    ctx = get_context("gpu")
    tmp = tempfile.mkdtemp(prefix="save_time_")
    aff = np.diag([-1.5, -1.5, 1.5, 1.0])
    shape = (a.size,) * 3
    modes = a.modes.split(",")
    res = {"what": "nifti.save of uint8 label volumes and an int16 CT: zlib level 1 on host threads vs the device deflate encoder",
           "shape": list(shape), "cpu_threads": a.threads, "reps": a.reps, "member_bytes": nifti._GZ_BLOCK, "modes": modes, "phantoms": {}}
    ok = True
    for name in a.phantoms.split(","):
        vol = synthetic.ct_phantom(shape, seed=5) if name == "ct" else getattr(synthetic, f"label_phantom_{name}")(shape)
        d_vol = DevArray.from_numpy(ctx, np.ascontiguousarray(vol.transpose(2, 1, 0))).transpose((2, 1, 0))    # file order on the device
        keys = ["cpu", "cpu_from_device"] + [f"{k}_{m}" for m in modes for k in ("device_from_host", "device")]
        paths = {k: os.path.join(tmp, f"{name}_{k}.nii.gz") for k in keys}
        runs = {
            "cpu": lambda: nifti.save(paths["cpu"], vol, aff, threads=a.threads),
            "cpu_from_device": lambda: nifti.save(paths["cpu_from_device"], d_vol.download(), aff, threads=a.threads),
        }
        for m in modes:
            runs[f"device_from_host_{m}"] = lambda m=m: nifti.save(paths[f"device_from_host_{m}"], vol, aff, ctx=ctx, dynamic=m == "dynamic")
            runs[f"device_{m}"] = lambda m=m: nifti.save(paths[f"device_{m}"], d_vol, aff, ctx=ctx, dynamic=m == "dynamic")
        if a.kernel_only:
            for m in modes:
                runs[f"device_{m}"]()
                runs[f"device_{m}"]()
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
        r.update({"payload_bytes": int(vol.nbytes), "dtype": str(vol.dtype), "cpu_file_bytes": len(raw["cpu"])})
        for m in modes:
            same = all(gzip.decompress(raw[f"{k}_{m}"]) == want for k in ("device_from_host", "device"))
            ok = ok and same and raw[f"device_{m}"] == raw[f"device_from_host_{m}"]
            dev = float(np.median(times[f"device_{m}"]))
            r[m] = {"device_file_bytes": len(raw[f"device_{m}"]), "device_over_cpu_size": round(len(raw[f"device_{m}"]) / len(raw["cpu"]), 3),
                    "decompressed_equal": same, "cpu_over_device_time": round(float(np.median(times["cpu"])) / dev, 2),
                    "cpu_from_device_over_device_time": round(float(np.median(times["cpu_from_device"])) / dev, 2),
                    "cpu_over_device_from_host_time": round(float(np.median(times["cpu"]) / np.median(times[f"device_from_host_{m}"])), 2),
                    "device_from_host_breakdown": _breakdown(ctx, nifti, vol, os.path.join(tmp, f"{name}_b.nii.gz"), m == "dynamic")}
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
