"""boa_finalize_labels / boa_finalize_labels_planes in both kernel forms, and boa_accumulate_tile at its edges, against
head_cases.finalize_ref / oracle.sliding_window.accumulate_tile (tests/test_head_cases_cpu.py pins finalize_ref to the golden vectors).

k_finalize_labels<8> needs the voxel count, the first voxel and the count of the plane range to be multiples of 8 and 16-byte aligned
buffers; k_finalize_labels<1> takes everything else.  The counter `finalize_vec8` says which ran, head_cases.finalize_form restates the
rule, and every call asserts that the two agree.  Inputs are fp16 BIT PATTERNS (normals, subnormals, +-0, exact ties for the first
place; +-inf and NaN in the cases marked special); outputs are compared bit for bit with every NaN mapped to one pattern
(head_cases.canon_nan).  Every device array lies between sentinel runs that must come back untouched."""
import ctypes as C
import itertools

import numpy as np
import pytest

import head_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


def _i3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


class _Dev:
    """an array in the middle of a sentinel-filled allocation, `shift` elements past the guard (shift 1: 2 bytes off 16-byte alignment)"""

    def __init__(self, ctx, arr, shift=0, salt=0):
        from boa_hip.device import BufferView
        arr = np.ascontiguousarray(arr)
        self.shape, self.dtype, self.lo, self.n = arr.shape, arr.dtype, hc.GUARD + shift, arr.size
        self.host = np.concatenate([hc.sentinel(self.lo, salt).astype(arr.dtype), arr.reshape(-1), hc.sentinel(hc.GUARD, salt + 1).astype(arr.dtype)])
        self.buf = ctx.from_numpy(self.host)
        assert self.buf.ptr % 256 == 0
        self.view = BufferView(self.buf, self.lo * arr.itemsize, arr.nbytes)
        self.align = (self.lo * arr.itemsize) % 16

    @property
    def vp(self):
        return self.view.vp

    def read(self):
        got = self.buf.download(self.host.shape, self.dtype)
        np.testing.assert_array_equal(got[:self.lo], self.host[:self.lo], err_msg="wrote in front of the buffer")
        np.testing.assert_array_equal(got[self.lo + self.n:], self.host[self.lo + self.n:], err_msg="wrote behind the buffer")
        return got[self.lo:self.lo + self.n].reshape(self.shape).copy()

    def free(self):
        self.buf.free()


def _finalize(ctx, acc, n, fold, labels, V, fold_mode=None, n_folds_final=0, write_logits=1, lut=None, merge=0, crop=None, planes=None,
              shifts=(0, 0, 0)):
    """One device call on fresh buffers.  Returns ((acc, fold, labels, flag) after the call, launches of the vec8 form, the form
    head_cases.finalize_form predicts)."""
    from boa_hip._lib import check
    Cn = acc.shape[0]
    d_acc, d_n = _Dev(ctx, acc, shifts[0], 10), _Dev(ctx, n, shifts[1], 20)
    d_fold = _Dev(ctx, fold, shifts[2], 30) if fold is not None else None
    d_lab = _Dev(ctx, labels, 0, 40) if labels is not None else None
    flag = ctx.zeros(4)
    lut_p = np.ascontiguousarray(lut).ctypes.data_as(C.c_void_p) if lut is not None else None
    lo, hi = planes if planes is not None else (0, V[0])
    ctx.counters(reset=True)
    try:
        check(ctx.lib.boa_finalize_labels_planes(ctx.h, d_acc.vp, d_n.vp, Cn, _i3(V), d_fold.vp if d_fold else None, fold_mode or 0, n_folds_final,
                                                 write_logits, lut_p, merge, d_lab.vp if d_lab else None, _i3(crop[0]) if crop else None,
                                                 _i3(crop[1]) if crop else None, flag.vp, lo, hi), "boa_finalize_labels_planes")
        ctx.sync()
        vec8 = ctx.counters()["finalize_vec8"]
        np.testing.assert_array_equal(d_n.read(), n, err_msg="the weight plane is read only")
        out = (d_acc.read(), d_fold.read() if d_fold else None, d_lab.read() if d_lab else None, int(flag.download((1,), np.int32)[0]))
    finally:
        for b in (d_acc, d_n, d_fold, d_lab, flag):
            if b is not None:
                b.free()
    form = hc.finalize_form(V, planes, d_acc.align, d_n.align, d_fold.align if d_fold else 0)
    assert vec8 == (0 if lo == hi else 1 if form == 8 else 0), (V, planes, shifts, vec8, form)
    return out, vec8, form


def _same(got, want, what):
    g_acc, g_fold, g_lab, g_flag = got
    w_acc, w_fold, w_lab, w_flag = want
    np.testing.assert_array_equal(hc.canon_nan(g_acc), hc.canon_nan(w_acc), err_msg=f"{what}: accumulators")
    assert (g_fold is None) == (w_fold is None)
    if w_fold is not None:
        np.testing.assert_array_equal(hc.canon_nan(g_fold), hc.canon_nan(w_fold), err_msg=f"{what}: fold buffer")
    if w_lab is not None:
        np.testing.assert_array_equal(g_lab, w_lab, err_msg=f"{what}: labels")
    assert g_flag == w_flag, (what, g_flag, w_flag)


def _ref(acc, n, fold, labels, **kw):
    """finalize_ref; a call that writes no labels leaves the label volume as it was"""
    kw = dict(kw, fold_mode=kw.get("fold_mode") or 0)
    a, f, lab, flag = hc.finalize_ref(acc, n, fold_bits=fold, labels_in=labels, **kw)
    return a, f, (lab if lab is not None else labels), flag


def _opts(case):
    return dict(fold_mode=case.fold_mode, n_folds_final=case.n_folds_final, write_logits=case.write_logits, merge=case.merge, crop=case.crop)


@pytest.mark.parametrize("case", hc.finalize_cases(), ids=lambda c: c.name)
def test_finalize_forms_and_options(ctx, case):
    """Both forms at 1 / 2 / 255 classes, with and without inf / NaN inputs, and the options in combination (pairwise cover: fold_mode 0 / 1,
    n_folds_final 0 / 1 / 3, write_logits, LUT, merge into a pre-filled label volume, crop with offsets on all three axes)."""
    acc, n, fold, lut, labels = hc.finalize_inputs(case)
    got, vec8, form = _finalize(ctx, acc, n, fold, labels, case.V, lut=lut, **_opts(case))
    assert form == case.vec
    want = _ref(acc, n, fold, labels, lut=lut, **_opts(case))
    _same(got, want, case.name)
    if case.special:
        assert want[3] == 1
    if not case.write_logits:
        np.testing.assert_array_equal(got[0], acc)
    if case.labels and case.C > 2:
        assert len(np.unique(got[2])) > 2


@pytest.mark.parametrize("which", ["acc", "n", "fold"])
def test_a_pointer_two_bytes_off_takes_the_scalar_form(ctx, which):
    """A vec8-sized volume whose acc, n or fold pointer sits 2 bytes into its 16-byte line: the scalar form, the aligned call's results."""
    case = hc.FinalizeCase("offset", (2, 4, 8), 7, 8, 1, 3, 1, True, 1, ((0, 1, 2), (2, 2, 5)), special=True)
    acc, n, fold, lut, labels = hc.finalize_inputs(case)
    shifts = tuple(int(which == k) for k in ("acc", "n", "fold"))
    aligned, v8, _ = _finalize(ctx, acc, n, fold, labels, case.V, lut=lut, **_opts(case))
    shifted, v1, form = _finalize(ctx, acc, n, fold, labels, case.V, lut=lut, shifts=shifts, **_opts(case))
    assert (v8, v1, form) == (1, 0, 1)
    want = _ref(acc, n, fold, labels, lut=lut, **_opts(case))
    _same(aligned, want, "aligned")
    _same(shifted, want, f"{which} + 2 bytes")


@pytest.mark.parametrize("V", [(4, 3, 6), (4, 2, 4), (3, 5, 7)], ids=lambda v: "x".join(map(str, v)))
def test_plane_ranges(ctx, V):
    """boa_finalize_labels_planes: [0, k) then [k, V0) is the whole volume for every k, and a call leaves the planes outside its range alone
    (accumulators, fold planes, labels).  (4, 3, 6): 72 voxels in planes of 18 -- a vec8 volume whose ranges start or end off a multiple
    of 8 (scalar form) except [0, 4); (4, 2, 4): planes of 8, every range vec8; (3, 5, 7): always scalar."""
    crop = ((1, 1, 1), (V[0] - 1, V[1] - 1, V[2] - 2))
    case = hc.FinalizeCase("planes", V, 6, hc.finalize_form(V), 1, 3, 1, True, 1, crop, special=True)
    acc, n, fold, lut, labels = hc.finalize_inputs(case)
    kw = dict(lut=lut, **_opts(case))
    whole, _, _ = _finalize(ctx, acc, n, fold, labels, V, **kw)
    _same(whole, _ref(acc, n, fold, labels, **kw), "whole")
    forms = set()
    for k in range(V[0] + 1):
        first, _, f1 = _finalize(ctx, acc, n, fold, labels, V, planes=(0, k), **kw)
        _same(first, _ref(acc, n, fold, labels, planes=(0, k), **kw), f"[0, {k})")
        np.testing.assert_array_equal(first[0][:, k:], acc[:, k:])                     # outside the range: untouched
        np.testing.assert_array_equal(first[1][:, k:], fold[:, k:])
        out_planes = slice(max(k - crop[0][0], 0), None)
        np.testing.assert_array_equal(first[2][out_planes], labels[out_planes])
        second, _, f2 = _finalize(ctx, first[0], n, first[1], first[2], V, planes=(k, V[0]), **kw)
        np.testing.assert_array_equal(second[0][:, :k], first[0][:, :k])
        np.testing.assert_array_equal(second[1][:, :k], first[1][:, :k])
        _same((second[0], second[1], second[2], first[3] | second[3]), whole, f"[0, {k}) + [{k}, {V[0]})")
        forms.update(f for f, (lo, hi) in ((f1, (0, k)), (f2, (k, V[0]))) if lo != hi)
    assert forms == {(4, 3, 6): {1, 8}, (4, 2, 4): {8}, (3, 5, 7): {1}}[V]
    if V == (4, 3, 6):    # the range the issue names: vtot % 8 == 0, v_begin % 8 != 0
        assert hc.finalize_form(V, (1, 4)) == 1 and (18 % 8, (3 * 18) % 8) == (2, 6)
        mid, v8, f = _finalize(ctx, acc, n, fold, labels, V, planes=(1, 3), **kw)
        assert (v8, f) == (0, 1)
        _same(mid, _ref(acc, n, fold, labels, planes=(1, 3), **kw), "[1, 3)")


@pytest.mark.parametrize("V", [(3, 5, 7), (2, 4, 8)], ids=["scalar", "vec8"])
def test_zero_and_subnormal_weights(ctx, V):
    """n == 0 with acc == 0 (0 / 0 = NaN in every class: the first NaN wins, no inf flag), n == 0 with acc != 0 (+-inf: the flag; next to
    a 0 / 0 class the NaN still wins), and subnormal n (quotients that are large, or overflow)."""
    rng = np.random.default_rng(V[2])
    Cn, nv = 4, int(np.prod(V))
    acc = (rng.standard_normal((Cn, nv)) * 2).astype(np.float16)
    n = rng.uniform(0.5, 9, nv).astype(np.float16)
    v = rng.permutation(nv)
    nan_v, inf_v, mix_v, sub_small, sub_big = v[0:6], v[6:12], v[12:18], v[18:24], v[24:30]
    n[nan_v] = 0
    acc[:, nan_v] = 0
    acc[1, nan_v[:3]] = np.float16(-0.0)                                    # -0 / 0 is NaN as well
    n[inf_v] = 0
    acc[:, inf_v] = np.where(acc[:, inf_v] == 0, np.float16(1), acc[:, inf_v])
    n[mix_v] = 0
    acc[:, mix_v] = np.float16(3)
    acc[2, mix_v] = 0                                                      # class 2: 0 / 0 among +inf classes
    nb = n.view(np.uint16)
    nb[sub_small] = rng.integers(1, 0x0400, 6)
    acc.view(np.uint16)[:, sub_small] = rng.integers(1, 0x0400, (Cn, 6))   # subnormal / subnormal: finite
    nb[sub_big] = rng.integers(1, 0x0400, 6)                               # normal / subnormal: overflows fp16
    acc_b, n_b = acc.view(np.uint16).reshape(Cn, *V), nb.reshape(V)
    labels = np.full(V, 200, np.uint8)
    flat = lambda a: a.reshape(-1)
    # without the voxels that must raise the flag, it must stay down
    quiet_acc, quiet_n = acc_b.copy(), n_b.copy()
    for idx in (inf_v, mix_v, sub_big):
        flat(quiet_n)[idx] = 0x3C00
    for name, a, w, flag in (("quiet", quiet_acc, quiet_n, 0), ("inf", acc_b, n_b, 1)):
        got, _, form = _finalize(ctx, a, w, None, labels, V)
        assert form == hc.finalize_form(V)
        want = _ref(a, w, None, labels)
        assert want[3] == flag
        _same(got, want, name)
        assert (flat(got[2])[nan_v] == 0).all()                              # NaN in every class: the first one
        f = got[0].view(np.float16).reshape(Cn, -1)
        assert np.isnan(f[:, nan_v]).all() and np.isfinite(f[:, sub_small]).all()
    assert (flat(got[2])[mix_v] == 2).all() and np.isinf(f[:, inf_v]).all() and np.isinf(f[:, sub_big]).any()


@pytest.mark.parametrize("Cn", [1, 40])
@pytest.mark.parametrize("P", [(1, 1, 1), (3, 5, 7)], ids=["P1x1x1", "P3x5x7"])
def test_accumulate_tile_edges(ctx, P, Cn):
    """boa_accumulate_tile (the step behind the unaligned MFMA path and the mirrored path): one-voxel and odd patches, with and without
    the Gaussian, at the origin and flush against the far corner, bit exact against the oracle and contained."""
    from boa_hip._lib import check
    rng = np.random.default_rng([Cn, *P])
    PV = (P[0] + 2, P[1] + 3, P[2] + 5)
    far = tuple(v - p for v, p in zip(PV, P))
    for g16, starts in itertools.product((None, hc.gaussian(P)), (((0, 0, 0), far), (far, (1, 1, 2), (0, 0, 0)))):
        acc0 = rng.uniform(-4, 4, (Cn, *PV)).astype(np.float16)
        n0 = rng.uniform(0, 4, PV).astype(np.float16)
        d_acc, d_n = _Dev(ctx, acc0.view(np.uint16), 0, 1), _Dev(ctx, n0.view(np.uint16), 0, 2)
        d_g = ctx.from_numpy(g16.view(np.uint16)) if g16 is not None else None
        o_acc, o_n = acc0.copy(), n0.copy()
        bufs = [d_acc, d_n] + ([d_g] if d_g is not None else [])
        try:
            for s in starts:
                pred = (rng.standard_normal((Cn, *P)) * rng.choice([1e-3, 1.0, 300.0], (Cn, 1, 1, 1))).astype(np.float32)
                d_p = ctx.from_numpy(pred)
                bufs.append(d_p)
                check(ctx.lib.boa_accumulate_tile(ctx.h, d_p.vp, d_g.vp if d_g is not None else None, d_acc.vp, d_n.vp, Cn, _i3(P), _i3(PV),
                                                  _i3(s)), "boa_accumulate_tile")
                hc.accumulate_tile(o_acc, o_n, pred, g16, s)
            ctx.sync()
            np.testing.assert_array_equal(d_n.read().reshape(PV), o_n.view(np.uint16))
            np.testing.assert_array_equal(hc.canon_nan(d_acc.read().reshape(Cn, *PV)), hc.canon_nan(o_acc.view(np.uint16)))
        finally:
            for b in bufs:
                b.free()
        assert (o_acc != acc0).any() and (o_n != n0).any()
