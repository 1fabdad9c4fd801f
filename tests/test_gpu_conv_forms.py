"""Single-layer fp64 parity of every conv kernel form and tile plan (cases: tests/conv_form_cases.py, proven on the CPU by
tests/test_conv_form_cases_cpu.py).

Each case launches ONE layer through boa_conv_layer_test / boa_convt_layer_test -- the production packers and launchers, the plan of
boa_conv_plan or an override of it -- on unit-normal sources, (scale, shift) tables in 1 +- 0.3 / +- 0.5 and weights scaled by
1 / sqrt(K), and compares the kernel's own output buffer with tests/layer_reference.py: the consumer's input transform bit for bit
(norm_act8_pk for k_conv_ws / k_conv_ns and every fp16 transposed conv given the packed table, norm_act8 for k_conv_mfma and for
k_convt_mfma given the fp32 table alone, norm_act_x3 for the split-precision kernels), conv3d64 / convt64 and abs_bound, under the project's bars
    fp16 : |c - c64| <= TAU_FP16 A + FP16_STORE |c64| + 2^-25        split precision: |c - c64| <= tau_x3(K) A
the (scale, shift) bars of layer_reference.ss_bars and ss16 == ss16_pack(ss) bit for bit.  Further: the plan the seam reports is the
one predicted on the CPU; every output / table buffer is prefilled with 0xFF bytes and followed by a guard region, which must stay
untouched while every element in front of it is written; k_norm_finalize leaves the partials table zero; and a conv run at N = 3 with
sample 0 repeated gives sample 0 (and its copies) the bits of the N = 1 run -- the batch independence TILE_REF_BATCH exists for."""
import ctypes as C
import zlib

import numpy as np
import pytest

import conv_form_cases as cf
import layer_reference as lr

pytestmark = pytest.mark.gpu

GUARD = 4096
ROWS = []


@pytest.fixture(scope="module")
def ctx():
    import torch
    from boa_hip.device import Context
    torch.set_num_threads(16)
    c = Context(0)
    assert c.info()["cu_count"] == cf.TEST_CU, "the cases are generated for the MI355X's 256 compute units"
    yield c
    c.close()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _seam(rc, what):
    """A refused argument fails the test; a HIP error ends the session: nothing more is started on a device that has faulted."""
    from boa_hip import _lib
    if rc not in (_lib.BOA_OK, _lib.BOA_EINVAL):
        pytest.exit(f"{what}: {_lib.lib().boa_last_error().decode('utf-8', 'replace')}", returncode=3)
    _lib.check(rc, what)


class _Guarded:
    """A device buffer of `nbytes` + a guard region, all 0xFF (zero=True: the body zeroed, as the partials table must be)."""

    def __init__(self, ctx, nbytes, zero=False):
        from boa_hip._lib import check
        self.ctx, self.nbytes = ctx, int(nbytes)
        self.buf = ctx.alloc(self.nbytes + GUARD)
        check(ctx.lib.boa_memset(ctx.h, self.buf.vp, 0xFF, self.nbytes + GUARD))
        if zero:
            check(ctx.lib.boa_memset(ctx.h, self.buf.vp, 0, self.nbytes))
        self.vp = self.buf.vp

    def read(self, dtype):
        """The body as `dtype`; asserts the guard is untouched."""
        raw = self.buf.download((self.nbytes + GUARD,), np.uint8)
        self.buf.free()
        assert (raw[self.nbytes:] == 0xFF).all(), "guard region written"
        return np.array(raw[:self.nbytes]).view(dtype)


def _unplane(flat, N, Cc, dims, per):
    """[N][C/per][vox][per] -> [N][C][D][H][W]"""
    vox = int(np.prod(dims))
    return flat.reshape(N, Cc // per, vox, per).transpose(0, 1, 3, 2).reshape(N, Cc, *dims)


def _all_written(a):
    bits = a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)
    return not (bits == (0xFFFF if a.dtype.itemsize == 2 else 0xFFFFFFFF)).any()


def _rng(case):
    return np.random.default_rng(zlib.crc32(case["id"].encode()))


def _tables(rng, Cc, norm, fp16):
    if not norm:
        return None, None
    ss = np.stack([1 + 0.3 * rng.uniform(-1, 1, Cc), 0.5 * rng.uniform(-1, 1, Cc)], 1).astype(np.float32)
    return ss, (lr.ss16_pack(ss) if fp16 else None)


def _source_input(mode, pk, x, ss, ss16):
    """What the kernel builds from a source (tests/layer_reference.py), in float64."""
    if mode == "split":
        return (x if ss is None else lr.norm_act_x3(x, ss)).astype(np.float64)
    x16 = x.astype(np.float16)
    if ss is None:
        return x16.astype(np.float64)
    if pk:
        return lr.norm_act8_pk(x16, lr.ss16_unpack(ss16)).astype(np.float64)
    return lr.norm_act8(x16, ss).astype(np.float64)


def _bound(mode, K, A, c64):
    if mode == "fp16":
        extra = lr.FP16_STORE * np.abs(c64) + 2.0 ** -25
        return lr.TAU_FP16 * A + extra, A + extra / lr.TAU_FP16, lr.TAU_FP16
    tau = lr.tau_x3(K)
    return tau * A, A, tau


def _upload_tiled(ctx, a, N):
    return None if a is None else ctx.from_numpy(np.ascontiguousarray(np.broadcast_to(a[None], (N,) + a.shape)))


# ---- convs -----------------------------------------------------------------------------------------------------------------------------
def _conv_inputs(case):
    rng = _rng(case)
    fp16 = case["mode"] == "fp16"
    cins = [c for c in (case["cin0"], case["cin1"]) if c]
    src = [rng.standard_normal((c, *case["dims"])).astype(np.float32) for c in cins]
    tabs = [_tables(rng, c, n, fp16) for c, n in zip(cins, case["norms"])]
    K = sum(cins) * int(np.prod(case["k"]))
    w = (rng.standard_normal((case["cout"], sum(cins), *case["k"])) / np.sqrt(K)).astype(np.float32)
    b = (0.1 * rng.standard_normal(case["cout"])).astype(np.float32)
    gam = (1 + 0.2 * rng.standard_normal(case["cout"])).astype(np.float32)
    bet = (0.2 * rng.standard_normal(case["cout"])).astype(np.float32)
    return dict(src=src, tabs=tabs, K=K, w=w, b=b, gam=gam, bet=bet)


def _conv_launch(ctx, case, d, N):
    from boa_hip._lib import check
    fp16 = case["mode"] == "fp16"
    plan = case["plan"]
    dout, cout, nblk = tuple(plan[24:27]), case["cout"], plan[23]
    vout = int(np.prod(dout))
    keep = []
    args = []
    for i in range(2):
        if i < len(d["src"]):
            ss, ss16 = d["tabs"][i]
            bufs = [_upload_tiled(ctx, d["src"][i], N), _upload_tiled(ctx, ss, N), _upload_tiled(ctx, ss16, N)]
            keep += bufs
            args += [bufs[0].vp, d["src"][i].shape[0]] + [None if x is None else x.vp for x in bufs[1:]]
        else:
            args += [None, 0, None, None]
    raw = _Guarded(ctx, N * cout * vout * (2 if fp16 else 4))
    ss = _Guarded(ctx, N * cout * 2 * 4)
    ss16 = _Guarded(ctx, N * cout * 4) if fp16 else None
    part = _Guarded(ctx, N * cout * 2 * nblk * 4, zero=True)
    got_plan = (C.c_int * cf.PLAN_WORDS)()
    ov = None if case["override"] is None else (C.c_int * 8)(*case["override"])
    _seam(ctx.lib.boa_conv_layer_test(ctx.h, cf.MODES[case["mode"]], N, cf._int3(case["dims"]), *args, _vp(d["w"]), _vp(d["b"]), _vp(d["gam"]),
                                      _vp(d["bet"]), cout, cf._int3(case["k"]), cf._int3(case["s"]), ov, raw.vp, ss.vp,
                                      None if ss16 is None else ss16.vp, part.vp, got_plan), "boa_conv_layer_test")
    for x in keep:
        if x is not None:
            x.free()
    out = dict(plan=list(got_plan))
    flat = raw.read(np.float16 if fp16 else np.float32)
    assert _all_written(flat), "output elements left unwritten"
    out["raw"] = _unplane(flat, N, cout, dout, 16 if fp16 else 8)
    out["ss"] = ss.read(np.float32).reshape(N, cout, 2)
    assert _all_written(out["ss"]), "(scale, shift) entries left unwritten"
    if fp16:
        words = ss16.read(np.uint32)
        assert _all_written(words), "packed fp16 (scale, shift) entries left unwritten"
        out["ss16"] = words.view(np.uint16).reshape(N, cout * 2)
    assert not part.read(np.uint8).any(), "k_norm_finalize did not leave the partials table zero"
    return out


@pytest.mark.parametrize("case", cf.conv_cases(), ids=lambda c: c["id"])
def test_conv_form(ctx, case):
    d = _conv_inputs(case)
    fp16 = case["mode"] == "fp16"
    one = _conv_launch(ctx, case, d, 1)
    assert one["plan"][:29] == case["plan"][:29], "the seam ran another plan than the one predicted on the CPU"
    pk = case["key"][0] in ("ws", "ns")
    xin = np.concatenate([_source_input(case["mode"], pk, x, *t) for x, t in zip(d["src"], d["tabs"])], 0)
    w = d["w"].astype(np.float16).astype(np.float32) if fp16 else d["w"]   # pack_conv_weights: fp16 weights
    L = lr.Layer("case", 0, 0, 0, [], "", None, tuple(case["k"]), tuple(case["s"]))
    c64 = lr.conv3d64(xin, w, d["b"], case["s"])
    A = lr.abs_bound(L, xin, w, d["b"]).astype(np.float64)
    c = one["raw"][0].astype(np.float64)
    assert c.shape == c64.shape
    bound, denom, tau = _bound(case["mode"], d["K"], A, c64)
    err = np.abs(c - c64)
    r = float((err / denom).max())
    ss64, mean, var = lr.norm_reference(one["raw"][0], d["gam"], d["bet"])
    rs, rt, _ = lr.ss_bars(one["raw"][0], one["ss"][0], ss64, mean, var, fp16)
    row = dict(id=case["id"], mode=case["mode"], family=case["key"][0], key=case["key"], plan=one["plan"], err=r, tau=tau, ss=rs, sh=rt)
    ROWS.append(row)
    print(f"\n{case['id']}: max err/A {r:.3g} (tau {tau:.3g}), scale/bar {rs:.3g}, shift/bar {rt:.3g}")
    assert (err <= bound).all(), f"conv error over the bar: max err/A {r:.3g}, tau {tau:.3g}, at {np.unravel_index(int(np.argmax(err / denom)), err.shape)}"
    assert rs <= 1 and rt <= 1, f"(scale, shift) over their bars: {rs:.3g}, {rt:.3g}"
    if fp16:
        assert np.array_equal(one["ss16"][0], lr.ss16_pack(one["ss"][0])), "ss16 is not the fp16 rounding of ss"
    # batch independence: sample 0 of the N = 3 run, and its copies, carry the bits of the N = 1 run
    three = _conv_launch(ctx, case, d, cf.BATCH)
    assert three["plan"][:29] == one["plan"][:29]
    u = np.uint16 if fp16 else np.uint32
    for n in range(cf.BATCH):
        assert np.array_equal(three["raw"][n].view(u), one["raw"][0].view(u)), f"sample {n} of the batch differs from the single run"
        assert np.array_equal(three["ss"][n].view(np.uint32), one["ss"][0].view(np.uint32)), f"(scale, shift) of sample {n} differ"
        if fp16:
            assert np.array_equal(three["ss16"][n], one["ss16"][0]), f"ss16 of sample {n} differs"


def _trim_cases():
    """The fewest-MAC case of (ws, fp16), (ns, fp16), (ws, split) and of the ws cases in which a workgroup's run crosses a sample boundary."""
    cases = cf.conv_cases()
    picks = [lambda c: c["key"][0] == "ws" and c["mode"] == "fp16", lambda c: c["key"][0] == "ns" and c["mode"] == "fp16",
             lambda c: c["key"][0] == "ws" and c["mode"] == "split", lambda c: c["key"][0] == "ws" and c["crossing"]]
    chosen = [min((c for c in cases if pick(c)), key=lambda c: c["macs"]) for pick in picks]
    return list({c["id"]: c for c in chosen}.values())


@pytest.mark.parametrize("case", _trim_cases(), ids=lambda c: c["id"])
def test_conv_tables_rebuilt_after_trim(ctx, case):
    """boa_trim releases the descriptor tables of the launches so far (the run tables stay): a launch after it, at the same batch and at
    another, builds them again and gives every sample the bits of the first run."""
    from boa_hip._lib import check
    d = _conv_inputs(case)
    fp16 = case["mode"] == "fp16"
    u = np.uint16 if fp16 else np.uint32
    first = None
    for step in (1, "trim", 1, cf.BATCH, "trim", cf.BATCH):
        if step == "trim":
            check(ctx.lib.boa_trim(ctx.h))
            continue
        got = _conv_launch(ctx, case, d, step)
        first = first or got
        assert got["plan"][:29] == case["plan"][:29]
        for n in range(step):
            assert np.array_equal(got["raw"][n].view(u), first["raw"][0].view(u)), f"N = {step}: sample {n} differs from the first run"
            assert np.array_equal(got["ss"][n].view(np.uint32), first["ss"][0].view(np.uint32)), f"N = {step}: (scale, shift) of sample {n} differ"
            if fp16:
                assert np.array_equal(got["ss16"][n], first["ss16"][0]), f"N = {step}: ss16 of sample {n} differs"


# ---- transposed convs ------------------------------------------------------------------------------------------------------------------
# Over the bar by the bar's derivation, not by the kernel: tau_x3 was measured on layers of K >= 32.  At K = Cin = 16 a voxel whose
# normalised inputs mostly sit on the LeakyReLU's negative side (|y| ~ 0.01 |x|, below 2^-3) has A = sum |w| |y| of a few 1e-2 while the
# lo parts of those activations are fp16 subnormals, an absolute floor of 2^-25 per operand.  layer_reference.x3_dot_emulate -- the
# specified arithmetic in numpy -- gives the same figures on the same inputs (tests/test_conv_form_cases_cpu.py), so k_convt_x3 computes
# what it is meant to.  The 4 096-voxel cases see such a voxel, the 64-voxel ones of the same form do not.
_X3_K16 = ("open: split-precision product at K = 16 with normalised inputs, err/A {gpu} on MI355X (numpy model of the arithmetic: {model}; bar "
           "9.5e-7): fp16-subnormal lo parts of activations below 2^-3.  Fix: scale the activations before the split (a kernel change)")
XFAIL = {
    "split-k_convt_x3<2>-16to32-16x16x16-s122-norm-N1": _X3_K16.format(gpu="2.21e-6", model="2.22e-6"),
    "split-k_convt_x3<2>-16to32-16x16x16-s221-norm-N1": _X3_K16.format(gpu="1.26e-6", model="1.29e-6"),
    "split-k_convt_x3<2>-16to32-16x16x16-s222-norm-N1": _X3_K16.format(gpu="1.44e-6", model="1.42e-6"),
}


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"], marks=[pytest.mark.xfail(strict=True, reason=XFAIL[c["id"]])] if c["id"] in XFAIL else [])
                                  for c in cf.convt_cases()])
def test_convt_form(ctx, case):
    from boa_hip._lib import check
    rng = _rng(case)
    fp16 = case["mode"] == "fp16"
    N, cin, cout, dims, s = case["N"], case["cin"], case["cout"], case["dims"], case["s"]
    x = rng.standard_normal((cin, *dims)).astype(np.float32)
    ss, ss16 = _tables(rng, cin, bool(case["norm"]), fp16 and case["norm"] is True)
    w = (rng.standard_normal((cin, cout, *s)) / np.sqrt(cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    dout = tuple(a * b_ for a, b_ in zip(dims, s))
    bufs = [_upload_tiled(ctx, x, N), _upload_tiled(ctx, ss, N), _upload_tiled(ctx, ss16, N)]
    raw = _Guarded(ctx, N * cout * int(np.prod(dout)) * (2 if fp16 else 4))
    got_plan = (C.c_int * cf.PLAN_WORDS)()
    _seam(ctx.lib.boa_convt_layer_test(ctx.h, cf.MODES[case["mode"]], N, cf._int3(dims), bufs[0].vp, cin, *[None if t is None else t.vp for t in bufs[1:]],
                                       _vp(w), _vp(b), cout, cf._int3(s), raw.vp, got_plan), "boa_convt_layer_test")
    for t in bufs:
        if t is not None:
            t.free()
    assert list(got_plan)[:8] == case["plan"][:8], "the seam ran another form than the one predicted on the CPU"
    flat = raw.read(np.float16 if fp16 else np.float32)
    assert _all_written(flat), "output elements left unwritten"
    got = _unplane(flat, N, cout, dout, 16 if fp16 else 8)
    pk = ss16 is not None   # every fp16 transposed conv prefers the packed table (k_convt_mfma too: norm_act8 only without one)
    xin = _source_input(case["mode"], pk, x, ss, ss16)
    wr = w.astype(np.float16).astype(np.float32) if fp16 else w
    L = lr.Layer("case", 1, 0, 0, [], "", None, tuple(s), tuple(s), transposed=True)
    c64 = lr.convt64(xin, wr, b, s)
    A = lr.abs_bound(L, xin, wr, b).astype(np.float64)
    bound, denom, tau = _bound(case["mode"], cin, A, c64)
    worst = 0.0
    for n in range(N):
        err = np.abs(got[n].astype(np.float64) - c64)
        worst = max(worst, float((err / denom).max()))
        assert (err <= bound).all(), f"sample {n}: max err/A {float((err / denom).max()):.3g}, tau {tau:.3g}"
    ROWS.append(dict(id=case["id"], mode=case["mode"], family=case["key"][0], key=case["key"], plan=list(got_plan), err=worst, tau=tau))
    print(f"\n{case['id']}: max err/A {worst:.3g} (tau {tau:.3g})")


def test_zz_report():
    """The instantiations that ran, as the seam reported them, and the worst err/A per family (`pytest -m gpu -s` prints the table)."""
    assert ROWS, "no case ran before the report"
    inst = {}
    for r in ROWS:
        p = r["plan"]
        if r["family"] in ("mfma", "ws", "ns"):
            k = r["key"]
            name = {"mfma": f"k_conv_mfma<{k[1]}>", "ws": f"k_conv_ws<{k[1]},{k[2]},3,3,{'true' if k[3] else 'false'},{'true' if k[4] else 'false'}>",
                    "ns": f"k_conv_ns<2,{k[10]},{k[10]},{'true' if k[4] else 'false'}>"}[r["family"]]
        else:
            name = r["family"]
        e = inst.setdefault(name, dict(n=0, err=0.0, tau=r["tau"], resident=set(), cy_fast=set(), vw8=set()))
        e["n"] += 1
        e["err"] = max(e["err"], r["err"])
        if r["family"] == "ws":
            e["resident"].add(p[17]); e["cy_fast"].add(p[18]); e["vw8"].add(p[19] % 8 == 0)
    print(f"\n{'instantiation':<40}{'cases':>6}{'worst err/A':>13}{'tau':>11}  resident cy_fast vw%8==0")
    for name in sorted(inst):
        e = inst[name]
        print(f"{name:<40}{e['n']:>6}{e['err']:>13.3g}{e['tau']:>11.3g}  {sorted(e['resident'])} {sorted(e['cy_fast'])} {sorted(e['vw8'])}")
    for fam in sorted({(r['mode'], r['family'].split('<')[0]) for r in ROWS}):
        rows = [r for r in ROWS if (r["mode"], r["family"].split("<")[0]) == fam]
        print(f"family {fam[0]} {fam[1]}: {len(rows)} cases, worst err/A {max(r['err'] for r in rows):.3g} (tau {rows[0]['tau']:.3g}), "
              f"worst scale/bar {max(r.get('ss', 0) for r in rows):.3g}, shift/bar {max(r.get('sh', 0) for r in rows):.3g}")
