"""The test-only JPEG Lossless encoder (tests/ljpeg_writer.py) pinned against libjpeg-turbo: Pillow decodes 8-bit SOF3 streams;
the committed fixture tests/golden/ljpeg/p8_libjpeg_turbo.npz holds what it decoded, so the pin holds where Pillow is absent."""
import io
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
import ljpeg_writer as W


def test_fixture_streams_are_the_writer_output_and_libjpeg_turbo_decodes_them_to_the_source():
    sys.path.insert(0, os.path.join(GOLDEN, "ljpeg"))
    try:
        import generate
    finally:
        sys.path.pop(0)
    g = np.load(os.path.join(GOLDEN, "ljpeg", "p8_libjpeg_turbo.npz"))
    cases = list(generate.cases())
    assert len(cases) == len(g["params"]) == 21
    for i, (x, pred, pt, rr) in enumerate(cases):
        assert tuple(g["params"][i]) == (x.shape[0], x.shape[1], pred, pt, rr)
        assert W.encode(x, precision=8, predictor=pred, pt=pt, restart_rows=rr) == g[f"stream_{i}"].tobytes()
        np.testing.assert_array_equal(g[f"decoded_{i}"], (x >> pt) << pt)


@pytest.mark.parametrize("pred", range(1, 8))
def test_pillow_decodes_writer_output(pred):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(pred)
    for pt in (0, 1, 2):
        for rr in (0, 1, 2, 3):
            h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
            x = rng.integers(0, 256, (h, w)) if pt % 2 else np.clip(np.cumsum(rng.integers(-3, 4, (h, w)), 1) + 128, 0, 255)
            s = W.encode(x, precision=8, predictor=pred, pt=pt, restart_rows=rr if rr < h else 0)
            np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(s))), (x >> pt) << pt)


def test_optimal_table_limits_codes_to_16_bits():
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    counts, values = W.optimal_table(np.array(fib[::-1]))
    assert sum(counts) == 17 and counts[15] > 0
    lengths = sorted(ln for _, ln in W.canonical_codes(counts, values).values())
    assert sum(2.0 ** -ln for ln in lengths) < 1.0                     # the all-1 code point stays free
