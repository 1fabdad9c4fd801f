"""Generator of p8_libjpeg_turbo.npz: 8-bit JPEG Lossless streams written by tests/ljpeg_writer.py and the arrays libjpeg-turbo
(through Pillow, which decodes 8-bit SOF3) made of them -- a third-party decode the GPU tests compare against where Pillow is
absent.  Every predictor, point transforms 0-2, restart intervals of 1-3 rows, sizes down to 1 x 1.
Run: python tests/golden/ljpeg/generate.py"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ljpeg_writer  # noqa: E402


def cases():
    rng = np.random.default_rng(20261016)
    sizes = [(1, 1), (1, 37), (41, 1), (23, 29), (64, 64)]
    k = 0
    for pred in range(1, 8):
        for pt in (0, 1, 2):
            h, w = sizes[k % len(sizes)]
            k += 1
            smooth = np.clip(np.cumsum(rng.integers(-4, 5, (h, w)), axis=1) + rng.integers(60, 200), 0, 255)
            x = smooth if k % 2 else rng.integers(0, 256, (h, w))
            rr = (k % 4) if (k % 4) < h else 0
            yield x.astype(np.int64), pred, pt, rr


def main():
    from PIL import Image
    streams, arrays, params = [], [], []
    for x, pred, pt, rr in cases():
        s = ljpeg_writer.encode(x, precision=8, predictor=pred, pt=pt, restart_rows=rr)
        got = np.asarray(Image.open(io.BytesIO(s)))
        streams.append(np.frombuffer(s, dtype=np.uint8))
        arrays.append(got.astype(np.uint8).reshape(x.shape))
        params.append((x.shape[0], x.shape[1], pred, pt, rr))
    out = {"params": np.asarray(params, dtype=np.int32)}
    for i, (s, a) in enumerate(zip(streams, arrays)):
        out[f"stream_{i}"] = s
        out[f"decoded_{i}"] = a
    np.savez_compressed(os.path.join(HERE, "p8_libjpeg_turbo.npz"), **out)
    print(f"{len(streams)} streams, {sum(len(s) for s in streams)} bytes")


if __name__ == "__main__":
    main()
