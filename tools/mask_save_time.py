"""One binary mask file per structure (TotalSegmentator's `ml=False` output) from a resident label volume: the fused writer
(`nifti.save_label_masks`: presence pass, encode of the present (label, member) pairs only, canned zero members) against the two
ways there were before it, on `synthetic.label_phantom_total` (117 labels) at SIZE^3, all three writing the same 117 files:
  new      nifti.save_label_masks on the device volume
  device   per label: materialise the mask on the device (boa_label_select), nifti.save(mask, ctx=ctx)
  host     per label: (volume == k) on the host, nifti.save on --threads host threads (zlib level 1)
Wall time, median of --reps, the three alternated after one warm-up round; the new call split into the presence pass, the encode
calls, the download of the compressed bytes and the file writes; the share of (label, member) pairs that hold a voxel; the bytes
written; and that the new files equal the device route's byte for byte and the host route's after gunzip.  Prints a report.
  python tools/mask_save_time.py 512 > profiles/mask_save_time_512.txt"""
import argparse
import ctypes as C
import gzip
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "body-and-organ-analysis_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("size", type=int, nargs="?", default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=8, help="host deflate threads of the host route (nifti.SAVE_THREADS)")
    ap.add_argument("--dynamic", action="store_true", help="dynamic Huffman codes in both device routes")
    a = ap.parse_args()

    from boa_hip import _lib, label_maps, nifti, synthetic
    from boa_hip.compute.inference import get_context
    from boa_hip.devarray import DevArray
    ctx = get_context("gpu")
    shape = (a.size,) * 3
    vol = synthetic.label_phantom_total(shape)
    names = {k: v for k, v in label_maps.CLASS_MAP_TOTAL.items() if k <= int(vol.max())}
    aff = np.diag([-1.5, -1.5, 1.5, 1.0])
    d_vol = DevArray.from_numpy(ctx, np.ascontiguousarray(vol.transpose(2, 1, 0))).transpose((2, 1, 0))    # file order on the device
    n = vol.size
    tmp = tempfile.mkdtemp(prefix="mask_save_time_")
    dirs = {k: os.path.join(tmp, k) for k in ("new", "device", "host")}
    for d in dirs.values():
        os.makedirs(d)
    infos = []

    def run_new():
        info = {}
        nifti.save_label_masks(dirs["new"], d_vol, aff, names, ctx, dynamic=a.dynamic, info=info)
        infos.append(info)

    def run_device():
        mask = DevArray.from_numpy(ctx, np.zeros(shape[::-1], np.uint8)).transpose((2, 1, 0))
        for k, name in names.items():
            _lib.check(ctx.lib.boa_label_select(ctx.h, d_vol.buf.vp, n, 0, (C.c_int * 3)(k, 0, 0), mask.buf.vp), "boa_label_select")
            nifti.save(os.path.join(dirs["device"], f"{name}.nii.gz"), mask, aff, ctx=ctx, dynamic=a.dynamic)
        mask.free()

    def run_host():
        for k, name in names.items():
            nifti.save(os.path.join(dirs["host"], f"{name}.nii.gz"), (vol == k).astype(np.uint8), aff, threads=a.threads)

    runs = {"new": run_new, "device": run_device, "host": run_host}
    times = {k: [] for k in runs}
    for rep in range(a.reps + 1):                       # rep 0: warm-up (code objects, pools, page cache)
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            print(f"[rep {rep}] {k}: {dt:.3f} s", file=sys.stderr, flush=True)
            if rep:
                times[k].append(dt)
    same_device = same_host = True
    for name in names.values():
        raw = {k: open(os.path.join(d, f"{name}.nii.gz"), "rb").read() for k, d in dirs.items()}
        same_device = same_device and raw["new"] == raw["device"]
        same_host = same_host and gzip.decompress(raw["new"]) == gzip.decompress(raw["host"])
    host_bytes = sum(os.path.getsize(os.path.join(dirs["host"], f)) for f in os.listdir(dirs["host"]))
    shutil.rmtree(tmp)
    d_vol.free()

    med = {k: float(np.median(v)) for k, v in times.items()}
    info = infos[1:]
    part = {k: float(np.median([i.get(k, 0.0) for i in info])) for k in ("presence", "encode", "download", "write")}
    i0 = info[0]
    print(f"mask_save_time: {len(names)} structures of label_phantom_total at {shape}, {n} voxels, members of {nifti._GZ_BLOCK} bytes, "
          f"{'dynamic' if a.dynamic else 'fixed'} codes, median of {a.reps} after one warm-up, routes alternated")
    print(f"  (label, member) pairs            {i0['pairs']}, present {i0['present']} = {i0['present'] / i0['pairs']:.3f} of all")
    print(f"  bytes written                    new / device route {i0['compressed_bytes']}, host route (zlib level 1) {host_bytes}")
    print(f"  new   save_label_masks           {med['new']:.3f} s   {[round(t, 3) for t in times['new']]}")
    print(f"          presence pass            {part['presence'] * 1e3:9.2f} ms   (one call, table download included)")
    print(f"          encode calls             {part['encode'] * 1e3:9.2f} ms   (pair tables up, three kernels, offsets and CRCs down)")
    print(f"          download of the bodies   {part['download'] * 1e3:9.2f} ms")
    print(f"          file writes              {part['write'] * 1e3:9.2f} ms")
    print(f"          the rest                 {(med['new'] - sum(part.values())) * 1e3:9.2f} ms   (zero members, header, pair lists, slicing)")
    print(f"  device  select + nifti.save(ctx) {med['device']:.3f} s   {[round(t, 3) for t in times['device']]}   = {med['device'] / med['new']:.1f} x new")
    print(f"  host    numpy + zlib, {a.threads} threads  {med['host']:.3f} s   {[round(t, 3) for t in times['host']]}   = {med['host'] / med['new']:.1f} x new")
    print(f"  files: new == device route byte for byte: {same_device}; new == host route after gunzip: {same_host}")
    return 0 if same_device and same_host else 1


if __name__ == "__main__":
    sys.exit(main())
