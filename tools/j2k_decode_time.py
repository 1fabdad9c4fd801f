"""JPEG 2000 series decode on the device (csrc/j2k.hip) on a 512 x 512 x 600 series, lossless (reversible 5/3) or, with
--irreversible, lossy (9/7: the decode is compared with OpenJPEG's own decode of every slice, not with the source):
  * where Pillow with OpenJPEG imports: the seeded CT-like phantom (boa_hip.synthetic.ct_phantom, stored = HU + 1024), every
    slice encoded by OpenJPEG with its defaults (64 x 64 blocks, 6 resolutions, one layer; --rate R: one layer of compression
    ratio R); otherwise the two committed phantom slices of tests/golden/j2k (tests/golden/j2k97 with --irreversible) cycled
    (the JSON line says which);
  * host read + codestream parse + tier-2 time of all frames;
  * the batched decode call (device events around jpeg2000.decode_frames: the upload of the code-block data and the tables,
    tier-1, the inverse transform, the status read-back and the output download); the kernels alone: run with --decode-only under
    `rocprofv3 --kernel-trace --stats`;
  * get_image_info wall time on the J2K series against the uncompressed series of the same volume, alternated (medians).
Prints one JSON line and writes it to --out.
  python tools/j2k_decode_time.py --out profiles/j2k_decode.json
  python tools/j2k_decode_time.py --irreversible --rate 10 --decode-only
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/j2k_decode_time.py --decode-only"""
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
    folder, z, sl, stream = args
    import j2k_writer as JW
    from dicom_writer import write_slice
    ipp = (-200.0, -180.0, 1.25 * z)
    p = os.path.join(folder, "IM%04d.dcm" % z)
    want = None
    if stream is None:
        write_slice(p, sl, ipp=ipp, instance=z + 1)
    else:
        if isinstance(stream, dict):                     # Pillow's options: encode here, in the worker
            kw = {k: v for k, v in stream.items() if k != "irreversible"}
            if stream["irreversible"]:
                import j2k97_fixtures as FX
                stream = FX.encode(sl.astype(np.uint16), **kw)
            else:
                stream = JW.encode(sl.astype(np.uint16), **kw)
            if kw or args[3]["irreversible"]:            # not lossless: OpenJPEG's own decode is what the decoder has to give
                want = JW.openjpeg_decode(stream).astype(np.uint16)
        JW.write_slice(p, sl, stream, transfer_syntax=JW.J2K if want is not None else JW.J2K_LOSSLESS, ipp=ipp, instance=z + 1)
    return os.path.getsize(p), want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--io-reps", type=int, default=3, help="alternated repetitions of get_image_info per series")
    ap.add_argument("--decode-only", action="store_true", help="decode timing only (for a rocprofv3 run)")
    ap.add_argument("--fixtures", action="store_true", help="cycle the committed phantom slices even where Pillow imports")
    ap.add_argument("--irreversible", action="store_true", help="lossy 9/7 streams (irreversible=True), checked against OpenJPEG")
    ap.add_argument("--rate", type=float, default=None, help="one quality layer of this compression ratio (Pillow's 'rates')")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import j2k_writer as JW
    n, size = a.slices, 512
    pillow = JW.have_pillow_j2k() and not a.fixtures
    if pillow:
        from boa_hip.synthetic import ct_phantom
        stored = (ct_phantom((size, size, n)).transpose(2, 1, 0).astype(np.int32) + 1024).astype(np.int64)
        opts = dict(irreversible=a.irreversible)
        if a.rate:
            opts.update(quality_layers=[a.rate], quality_mode="rates")
        streams = [opts] * n
        source = ("boa_hip.synthetic.ct_phantom 512x512x600 + 1024, encoded by OpenJPEG (Pillow) with "
                  + ("irreversible=True, " if a.irreversible else "") + (f"rate {a.rate:g}" if a.rate else "its defaults"))
    elif a.irreversible:
        import j2k97_fixtures as FX
        fx = [f for f in FX.load_fixtures() if f["name"].startswith("512x512_ct_phantom")]
        stored = np.stack([fx[z % 2]["decoded"] for z in range(n)])
        streams = [fx[z % 2]["stream"] for z in range(n)]
        source = "the two committed 512x512 phantom slices of tests/golden/j2k97 (Pillow's defaults, irreversible), cycled"
    else:
        fx = [f for f in JW.load_fixtures() if f["name"].startswith("512x512_ct_phantom")]
        stored = np.stack([fx[z % 2]["source"] for z in range(n)])
        streams = [fx[z % 2]["stream"] for z in range(n)]
        source = "the two committed 512x512 phantom slices of tests/golden/j2k, cycled"
    tmp = tempfile.mkdtemp(prefix="j2k_")
    res = {"what": "JPEG 2000 %s series decode" % ("lossy (9/7)" if a.irreversible else "lossless"), "slices": n, "rows": size,
           "cols": size, "series": source}
    t0 = time.perf_counter()
    jobs = [(os.path.join(tmp, "j2k"), z, stored[z], streams[z]) for z in range(n)]
    if not a.decode_only:
        jobs += [(os.path.join(tmp, "raw"), z, stored[z], None) for z in range(n)]
    for d in {j[0] for j in jobs}:
        os.makedirs(d, exist_ok=True)
    with ProcessPoolExecutor(max_workers=a.workers) as ex:       # (CPU only: before this process opens the device)
        done = list(ex.map(_write, jobs, chunksize=8))
    sizes = [d[0] for d in done]
    want = (stored & 0xFFFF).astype(np.uint16)          # lossless: the source; the committed lossy fixtures: OpenJPEG's decode
    if done[0][1] is not None:                          # lossy streams encoded here: OpenJPEG's own decode of every slice
        want = np.stack([d[1] for d in done[:n]])
    res["encode_and_write_s"] = round(time.perf_counter() - t0, 2)
    res["compressed_files_mb"] = round(sum(sizes[:n]) / 1e6, 1)

    from boa_hip import dicom, jpeg2000 as J
    from boa_hip.compute.inference import get_context
    files = dicom.series_file_names(os.path.join(tmp, "j2k"))
    t0 = time.perf_counter()
    sl = [dicom.read_file(p) for p in files]
    t1 = time.perf_counter()
    frames = [J.parse_frame(d["PixelData"], rows=size, cols=size, name=d["_path"]) for d in sl]
    t2 = time.perf_counter()
    res["host_read_s"] = round(t1 - t0, 3)
    res["host_parse_tier2_s"] = round(t2 - t1, 3)
    res["code_blocks"] = int(sum(len(f.blocks) for f in frames))
    res["coding_passes"] = int(sum(int(f.blocks[:, 6].sum()) for f in frames))
    in_bytes = sum(len(f.data) for f in frames)
    res["code_block_data_mb"] = round(in_bytes / 1e6, 2)
    res["bits_per_sample"] = round(8.0 * in_bytes / (n * size * size), 3)
    ctx = get_context("gpu")
    res["transforms"] = sorted({"9/7" if f.transform == 0 else "5/3" for f in frames})
    times, ok = [], True
    for rep in range(a.reps + 1):                               # rep 0: warm-up (code objects, pool)
        ctx.timer_start(0)
        px, st = J.decode_frames(ctx, frames)
        ms = ctx.timer_stop(0)
        ok = ok and bool((st == 0).all()) and all(np.array_equal(p, w) for p, w in zip(px, want))
        if rep:
            times.append(ms)
    res["decoded_equal_openjpeg" if a.irreversible or a.rate else "decoded_equal_source"] = ok
    med = float(np.median(times))
    res["call_ms"] = {"median": round(med, 3), "all": [round(t, 3) for t in times]}
    res["output_gbps"] = round(n * size * size * 2 / med / 1e6, 1)
    res["note"] = ("call time = device events around decode_frames (data and table uploads, the kernels, the status read-back, the "
                   "output download); kernel times: rocprofv3 --kernel-trace --stats on --decode-only")
    if not a.decode_only:
        from boa_hip.compute.io import get_image_info
        io_t = {"j2k": [], "uncompressed": []}
        for rep in range(a.io_reps):
            for kind, d in (("j2k", "j2k"), ("uncompressed", "raw")):
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
