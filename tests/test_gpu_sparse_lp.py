"""The sparse 3-D middle on 16-bit MFMA operands (dal3_sp_conv_lp_pack / dal3_sp_conv_lp; `sparse_precision` of sparse.py
and the detector classes), for "fp16" and "bf16":

  impulses      bit for bit: one non-zero channel at the centre of a 3 x 3 x 3 block of sites lands on every site as
                relu(fl32(q(v) q(W')[tap] + b')): the tap orientation, the weight rounding, and (values just above a rounding
                tie and on ties whose even neighbour is below / above) the activation rounding; q(v) q(W') has at most 22
                significant bits, so it is exact in float32 and the sum is one float32 addition.
  single layers against the float64 evaluation of the ROUNDED operands (sparse_lp_model.layer_rows on the rulebook) under
                the fp32 kernel's own bars (sparse_ref.BARS), the fp32 evaluation of the same operands as the yardstick.
                Site counts 1, 31, 32, 33, about 300, and the seams of the kernel's tiles: a wave holds 2 x 32 sites (63, 64,
                65) and a workgroup 256 (255, 256, 257). Every output sits in a guarded buffer behind a device count.
  same bits     the float32 input against the stored 16-bit one, max_workgroups 0 | 1 | 3, every choice of outputs, and
                y16 == q(y) exactly.
  the backbone  against tests/sparse_lp_model.py: its error against the unrounded float64 truth <= emu16.RMS_SLACK x the
                model's (rms) and <= emu16.MODEL_SLACK x (maxima); the sites are the fp32 route's exactly.
  non-finite inputs, the refusals, and the detector door.

With DAL3_SPARSE_LP_RECORD=<path> every error and ratio is written to <path> (how profiles/sparse_lp_measured.json is made)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import rpn_lp_model as M
import rpn_ref as R
import sparse_gpu
import sparse_lp_model as L
import sparse_ref as S
from emu16 import MODEL_SLACK, RMS_SLACK
from sparse_gpu import SENTINEL, Guarded, _dev, _hold, backbone_module, backbone_truth, bn_module, conv_module, hip, sparse, tensor
from test_gpu_rpn_lp import TIES

pytestmark = pytest.mark.gpu
PRECS = ("fp16", "bf16")
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
FORMS = {"subm": ((3, 3, 3), (1, 1, 1), (1, 1, 1), True), "k3s2p1": ((3, 3, 3), (2, 2, 2), (1, 1, 1), False),
         "k311s211": ((3, 1, 1), (2, 1, 1), (0, 0, 0), False)}
_LP_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _lp_record_file():
    yield
    path = os.environ.get("DAL3_SPARSE_LP_RECORD")
    if path:
        rows = dict(_LP_RECORD, **{k: v for k, v in sparse_gpu._RECORD.items() if k.startswith("lp/")})
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(rows, f, indent=1, sort_keys=True)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _host16(t):
    """a 16-bit tensor's bit patterns on the host"""
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@torch.no_grad()
def lp_layer(x, w, b, bn, form, relu, prec, residual=False, canvas=False, route="x", outs=("y", "y16"), mw=0):
    """pack + the bookkeeping + one dal3_sp_conv_lp launch with every output in a guarded, sentinel-filled buffer ->
    dict(y, y16 (bit patterns), bev, indices, n, shape) on the host. route: "x" (float32 rows) | "x16" (their 16-bit twin)"""
    kernel, stride, padding, subm = FORMS[form]
    conv = conv_module(w, b, kernel, stride, padding, subm)
    packed = sparse.pack_layer(conv, bn_module(bn), precision=prec)
    assert packed.dtype == torch.uint8 and packed.numel() == hip.lib().dal3_sp_conv_lp_pack_bytes(int(np.prod(kernel)), w.shape[3], w.shape[4])
    if subm:
        table, indices, n_out, shape, center, cap = sparse.subm_table(x, None, mw), x.indices, x.n, x.spatial_shape, 13, x.capacity
    else:
        indices, keys, n_out, cap, shape = sparse.downsample(x, kernel, stride, padding, None, mw)
        table, center = sparse.neighbour_table(x, indices, n_out, cap, shape, kernel, stride, padding, mw), -1
    c_in, c_out = w.shape[3], w.shape[4]
    feats, f16 = (x.features, None) if route == "x" else (None, x.features.to(T16[prec]))
    gy = Guarded(cap, c_out, torch.float32) if "y" in outs else None
    g16 = Guarded(cap, c_out, T16[prec]) if "y16" in outs else None
    gc, bev = None, None
    if canvas:
        D, H, W = shape
        gc = Guarded(x.batch_size * c_out * D * H * W, 0, torch.float32)
        bev = gc.view.view(x.batch_size, c_out * D, H, W)
    sparse.conv(feats, table, n_out, packed, c_in, c_out, x.status, relu=relu, residual=x.features if residual else None,
                center_tap=center, canvas=bev, out_indices=indices if canvas else None, canvas_shape=shape if canvas else None,
                out=gy.view if gy else None, max_workgroups=mw, precision=prec, features16=f16,
                out16=g16.view if g16 else False, rows=gy is not None)
    n = cap if n_out is None else int(n_out.item())
    assert int(x.status.item()) == 0
    out = dict(indices=indices.cpu().numpy()[:n], n=n, shape=shape, y=None, y16=None, bev=None)
    for g in (gy, g16, gc):
        assert g is None or g.intact(), "a guard row was written"
    if gy:
        assert bool((gy.view[n:] == SENTINEL).all()), "a float32 row beyond the count was written"
        out["y"] = gy.view[:n].cpu().numpy()
    if g16:
        assert bool((g16.view[n:] == SENTINEL).all()), "a 16-bit row beyond the count was written"
        out["y16"] = _host16(g16.view[:n])
    if gc:
        out["bev"] = bev.cpu().numpy()
    return out


def sites(tag, n, B=2):
    """n clustered sites of sparse_ref.GRID in sample B - 1 (the samples before it are empty), in a scrambled order"""
    c = S.clustered(f"lp/{tag}", S.GRID, 2, 260, 2.5)
    assert c.shape[0] >= n
    return np.concatenate([np.full((n, 1), B - 1, np.int32), c[:n]], 1)


# ------------------------------------------------------------------------------------- impulses
def _q1(value, prec):
    return np.float32(M.q(np.asarray([value], np.float32), prec)[0])


def _impulse_want(idx, oidx, osh, centre, c, value, wq, bf, form, relu, B, prec):
    kernel, stride, padding, _ = FORMS[form]
    t = S.table(oidx, idx, B, (9, 9, 9), osh, kernel, stride, padding)
    qv, wt = _q1(value, prec), wq.reshape(-1, wq.shape[3], wq.shape[4])
    want = np.repeat(bf[None, :], oidx.shape[0], 0).astype(np.float32)
    seen = 0
    for tap, o in zip(*np.nonzero(t == centre)):
        p = (qv * wt[tap, c]).astype(np.float32)
        assert np.array_equal(p.astype(np.float64), np.float64(qv) * wt[tap, c].astype(np.float64))      # exact in float32
        want[o] = p + bf                                        # one float32 addition
        seen += 1
    if relu:
        want = np.where(want > 0, want, np.float32(0))
    return want, seen


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c_in,c_out", [(5, 16), (5, 128), (16, 16), (16, 128)])
@pytest.mark.parametrize("form", ("subm", "k3s2p1", "canvas"))
def test_impulses_bit_for_bit(form, c_in, c_out, prec):
    canvas = form == "canvas"
    form = "k311s211" if canvas else form
    kernel, stride, padding, subm = FORMS[form]
    B, shape = 1, (9, 9, 9)
    # the block sits where the centre is seen through the most taps: an odd centre for the padded stride-2 window (two
    # outputs an axis), an even z for the unpadded (3, 1, 1) one (two outputs)
    o = 4 if form == "k3s2p1" else 3
    idx = np.asarray([[0, z, y, x] for z in (o, o + 1, o + 2) for y in (o, o + 1, o + 2) for x in (o, o + 1, o + 2)], np.int32)
    centre = 13
    assert idx[centre].tolist() == [0, o + 1, o + 1, o + 1]
    w, b, bn = S.layer_weights(f"lp/impulse/{form}/{c_in}-{c_out}", kernel, c_in, c_out, True, True)
    wf, bf = S.fold(w, b, bn)
    wq = M.q(wf, prec)
    assert (wq != wf).mean() > 0.9 and (bf < 0).any() and (bf > 0).any()
    osh = S.out_shape(shape, kernel, stride, padding)
    oidx = idx if subm else S.downsample(idx, B, shape, kernel, stride, padding)[0]
    up, down, up2 = (float(_q1(v, prec)) for v in TIES[prec])
    ulp = 2.0 ** -10 if prec == "fp16" else 2.0 ** -7
    assert (up, down, up2) == (1 + ulp, 1.0, 1 + 2 * ulp)
    values = [(1.0, True)] + [(v, True) for v in TIES[prec]] + [(-v, False) for v in TIES[prec]] + [(-1.0, False)]
    routes = ("x",) if c_in < 16 else ("x", "x16")
    for j, (value, relu) in enumerate(values):
        c = (j * 3) % c_in
        feats = np.zeros((27, c_in), np.float32)
        feats[centre, c] = value
        want, seen = _impulse_want(idx, oidx, osh, centre, c, value, wq, bf, form, relu, B, prec)
        assert seen == {"subm": 27, "k3s2p1": 8, "k311s211": 2}[form]
        if not relu:
            assert (want < 0).any()
        for route in routes:
            got = lp_layer(tensor(feats, idx, B, shape, capacity=27 + 5, n=27), w, b, bn, form, relu, prec, canvas=canvas, route=route)
            assert got["n"] == oidx.shape[0] and np.array_equal(got["indices"], oidx)
            d = np.argwhere(_bits(got["y"]) != _bits(want))
            assert not len(d), ((form, value, relu, route), len(d), [(tuple(i), float(got["y"][tuple(i)]), float(want[tuple(i)])) for i in d[:3]])
            assert np.array_equal(got["y16"], _host16(torch.from_numpy(want).to(T16[prec])))
            if canvas:
                dense = np.zeros((B, *osh, c_out), np.float32)
                dense[oidx[:, 0], oidx[:, 1], oidx[:, 2], oidx[:, 3]] = want
                dense = dense.transpose(0, 4, 1, 2, 3).reshape(B, c_out * osh[0], osh[1], osh[2])
                assert np.array_equal(_bits(got["bev"]), _bits(np.ascontiguousarray(dense)))


# ------------------------------------------------------------------------------------- single layers
PAIRS = ((5, 16), (8, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128))
COUNTS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300)
LAYER_FORMS = ("subm", "k3s2p1", "canvas")


def _reference(feats, idx, B, w, b, bn, form, relu, prec, residual):
    """(float64 rows of the rounded operands, the fp32 yardstick's, output indices, output shape) by the rulebook"""
    args = (feats, idx, S.GRID, w, b, bn, *FORMS[form][:3], FORMS[form][3], relu, prec, residual)
    truth, oidx, osh = L.layer_rows(S.Rulebook(B), *args)
    f32, _, _ = L.layer_rows(S.Rulebook(B, dtype=np.float32), *args)
    return truth, f32, oidx, osh


def _rows_of_canvas(bev, oidx, osh, c_out):
    d = bev.reshape(bev.shape[0], c_out, *osh)
    rows = d[oidx[:, 0], :, oidx[:, 1], oidx[:, 2], oidx[:, 3]]
    rest = d.copy()
    rest[oidx[:, 0], :, oidx[:, 1], oidx[:, 2], oidx[:, 3]] = 0
    assert not rest.any() and not np.signbit(rest).any(), "a cell that is no site is not +0"
    return rows


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_single_layers_under_the_fp32_kernels_bars(pair, prec):
    c_in, c_out = pair
    B = 2
    for ni, n in enumerate(COUNTS):
        v = PAIRS.index(pair) + ni
        # equal widths: the submanifold layer, its residual on every other count; the others walk through the three forms
        form = "subm" if c_in == c_out else LAYER_FORMS[v % 3]
        canvas, form = form == "canvas", "k311s211" if form == "canvas" else form
        residual, relu, bias, use_bn = form == "subm" and c_in == c_out and bool(ni & 1), bool((v >> 1) & 1), bool(v & 1), bool(v & 2) or not (v & 1)
        idx = sites(f"{c_in}", n, B)
        feats = S.synth.uniform(S.SEED, f"lp/layer/{c_in}/{n}/x", (n, c_in), -1.0 if not relu else 0.0, 2.0).astype(np.float32)
        w, b, bn = S.layer_weights(f"lp/layer/{c_in}-{c_out}/{form}", FORMS[form][0], c_in, c_out, bias, use_bn)
        truth, f32, oidx, osh = _reference(feats, idx, B, w, b, bn, form, relu, prec, residual)
        route = "x16" if c_in >= 16 and (ni & 2) else "x"
        got = lp_layer(tensor(feats, idx, B, S.GRID, capacity=n + 37, n=n), w, b, bn, form, relu, prec, residual, canvas, route,
                       mw=(0, 1, 3)[ni % 3])
        assert got["n"] == oidx.shape[0] and np.array_equal(got["indices"], oidx) and tuple(got["shape"]) == tuple(osh)
        rows = got["y"]
        assert np.array_equal(got["y16"], _host16(torch.from_numpy(rows).to(T16[prec])))
        if canvas:
            assert np.array_equal(_bits(_rows_of_canvas(got["bev"], oidx, osh, c_out)), _bits(rows))
        _hold(f"lp/{prec}/layer/{c_in}-{c_out}/{form}/n{n}/res{int(residual)}relu{int(relu)}", rows, f32, truth)


# ------------------------------------------------------------------------------------- the same bits
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c_in,c_out,form,residual,n", [(16, 16, "subm", True, 300), (32, 64, "k3s2p1", False, 257),
                                                        (128, 128, "subm", True, 65), (64, 128, "canvas", False, 300)])
def test_routes_grids_and_outputs_give_the_same_bits(c_in, c_out, form, residual, n, prec):
    canvas, form = form == "canvas", "k311s211" if form == "canvas" else form
    B = 2
    idx = sites(f"same/{c_in}", n, B)
    feats = S.synth.uniform(S.SEED, f"lp/same/{c_in}/x", (n, c_in), -1.0, 2.0).astype(np.float32)
    w, b, bn = S.layer_weights(f"lp/same/{c_in}-{c_out}", FORMS[form][0], c_in, c_out, True, True)

    def run(**kw):
        return lp_layer(tensor(feats, idx, B, S.GRID, capacity=n + 37, n=n), w, b, bn, form, True, prec, residual, canvas, **kw)

    ref = run()
    assert np.array_equal(ref["y16"], _host16(torch.from_numpy(ref["y"]).to(T16[prec])))          # y16 == q(y) exactly
    assert (ref["y"] > 0).any()
    for kw in (dict(route="x16"), dict(mw=1), dict(mw=3), dict(route="x16", mw=3), dict(outs=("y",)), dict(outs=("y16",)),
               dict(outs=("y16",), route="x16", mw=1)) + ((dict(outs=()),) if canvas else ()):
        got = run(**kw)
        for k in ("y", "y16", "bev"):
            if got[k] is not None:
                assert np.array_equal(_bits(got[k]), _bits(ref[k])), (kw, k)
        assert np.array_equal(got["indices"], ref["indices"])


# ------------------------------------------------------------------------------------- non-finite inputs
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c_in,c_out,form", [(5, 16, "subm"), (16, 16, "subm"), (32, 64, "k3s2p1")])
def test_nan_and_inf_rows_reach_what_the_model_says(c_in, c_out, form, prec):
    B, n = 2, 300
    idx = sites(f"nonfinite/{c_in}", n, B)
    feats = S.synth.uniform(S.SEED, f"lp/nonfinite/{c_in}/x", (n, c_in), 0.0, 2.0).astype(np.float32)
    feats[17], feats[211, 1] = np.nan, np.inf
    w, b, bn = S.layer_weights(f"lp/nonfinite/{c_in}-{c_out}", FORMS[form][0], c_in, c_out, True, True)
    residual = c_in == c_out
    truth, f32, oidx, _ = _reference(feats, idx, B, w, b, bn, form, True, prec, residual)
    assert not np.isfinite(truth).all() and np.isfinite(truth).all(1).sum() > 100
    for route in ("x",) if c_in < 16 else ("x", "x16"):
        got = lp_layer(tensor(feats, idx, B, S.GRID, capacity=n + 37, n=n), w, b, bn, form, True, prec, residual, route=route)
        g, t = S.finite_part(got["y"], truth)
        y, _ = S.finite_part(f32, truth)
        _hold(f"lp/{prec}/nonfinite/{c_in}-{c_out}/{form}/{route}", g, y, t)
        y16 = torch.from_numpy(got["y16"].view(np.int16)).view(T16[prec]).float().numpy()
        assert np.array_equal(~np.isfinite(y16), ~np.isfinite(truth))


# ------------------------------------------------------------------------------------- refusals
def _args(x, table, packed, out, dtype, c_in, c_out, feats=None, f16=None, y16=None):
    return hip.SpConvLpArgs(taps=27, c_in=c_in, c_out=c_out, relu=1, center_tap=13, in_capacity=x.capacity, x=hip.ptr(feats),
                            out_capacity=x.capacity, n_out=hip.ptr(x.n), table=hip.ptr(table), packed=hip.ptr(packed),
                            y=hip.ptr(out), status=hip.ptr(x.status), max_workgroups=0, dtype=dtype, x16=hip.ptr(f16), y16=hip.ptr(y16))


def test_bad_arguments_are_einval_and_nothing_is_launched():
    lib, B, n = hip.lib(), 2, 33
    idx = sites("refusal", n, B)
    packs = {}
    for c_in in (5, 16):
        w, b, bn = S.layer_weights(f"lp/refusal/{c_in}", (3, 3, 3), c_in, 16, True, True)
        packs[c_in] = (sparse.pack_layer(conv_module(w, b, (3, 3, 3), (1, 1, 1), (1, 1, 1), True), bn_module(bn), precision="fp16"), w, b, bn)
    x = tensor(np.ones((n, 16), np.float32), idx, B, S.GRID)
    x5 = tensor(np.ones((n, 5), np.float32), idx, B, S.GRID)
    table = sparse.subm_table(x)
    out = torch.full((n, 16), float(SENTINEL)).cuda()
    out16 = torch.full((n, 16), float(SENTINEL), dtype=torch.float16).cuda()
    f16, f16_5 = x.features.half(), x5.features.half()
    p16, p5 = packs[16][0], packs[5][0]
    bad = [(_args(x, table, p16, out, dtype, 16, 16, feats=x.features, y16=out16), b"dtype") for dtype in (hip.F32, hip.F16X3, 7, -1)]
    bad += [(_args(x, table, p16, out, hip.F16, 16, 16, feats=x.features, f16=f16, y16=out16), b"both x and x16"),
            (_args(x, table, p16, out, hip.F16, 16, 16, y16=out16), b"neither x nor x16"),
            (_args(x5, table, p5, out, hip.F16, 5, 16, f16=f16_5, y16=out16), b"x16 needs c_in"),
            (_args(x, table, p16, None, hip.F16, 16, 16, feats=x.features), b"no output")]
    for a, why in bad:
        assert lib.dal3_sp_conv_lp(a, hip.stream()) == hip.EINVAL and why in lib.dal3_last_error(), (why, lib.dal3_last_error())
    conv = conv_module(packs[16][1], packs[16][2], (3, 3, 3), (1, 1, 1), (1, 1, 1), True)
    Lr = hip.fold_layer_struct(conv, bn_module(packs[16][3]))
    buf = torch.full((p16.numel(),), 0x5A, dtype=torch.uint8, device="cuda")
    for dtype in (hip.F32, hip.F16X3, 7, -1):
        assert lib.dal3_sp_conv_lp_pack(Lr, 27, S.EPS, dtype, hip.ptr(buf), None, hip.stream()) == hip.EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((out16 == SENTINEL).all()) and bool((buf == 0x5A).all()) and int(x.status.item()) == 0
    assert lib.dal3_sp_conv_lp_pack_bytes(27, 16, 16) == p16.numel() == 256 + 128 + 27 * 1024
    assert lib.dal3_sp_conv_lp_pack_bytes(27, 5, 16) == p5.numel() == 256 + 128 + 27 * 1024
    assert lib.dal3_sp_conv_lp_pack_bytes(27, 128, 128) == 256 + 4 * 128 + 27 * 8 * 4 * 1024
    for taps, ci, co in ((0, 16, 16), (28, 16, 16), (27, 9, 16), (27, 16, 48), (27, 0, 16)):
        assert lib.dal3_sp_conv_lp_pack_bytes(taps, ci, co) == 0
    with pytest.raises(ValueError, match="not those of"):
        sparse.conv(x.features, table, x.n, p16, 16, 16, x.status)                 # a 16-bit blob given to the fp32 door
    with pytest.raises(ValueError, match="exactly one"):
        sparse.conv(x.features, table, x.n, p16, 16, 16, x.status, precision="fp16", features16=f16)
    with pytest.raises(ValueError, match="features16 must be"):
        sparse.conv(None, table, x.n, p16, 16, 16, x.status, precision="fp16", features16=x.features.bfloat16())


def test_a_weight_beyond_fp16_marks_the_pack_and_bf16_runs_it():
    B, n = 2, 33
    idx = sites("badw", n, B)
    w, b, _ = S.layer_weights("lp/badw", (3, 3, 3), 16, 16, True, False)
    w = w.copy()
    w[1, 1, 1, 3, 5] = 1.0e6
    conv = conv_module(w, b, (3, 3, 3), (1, 1, 1), (1, 1, 1), True)
    feats = S.synth.uniform(S.SEED, "lp/badw/x", (n, 16), 0.0, 2.0).astype(np.float32)
    for prec, refused in (("fp16", True), ("bf16", False)):
        status = torch.zeros(1, dtype=torch.int32).cuda()
        packed = sparse.pack_layer(conv, None, status, precision=prec)
        assert int(status.item()) == (hip.SP_BAD_WEIGHT if refused else 0)
        x = tensor(feats, idx, B, S.GRID)
        out = torch.full((n, 16), float(SENTINEL)).cuda()
        out16 = torch.full((n, 16), float(SENTINEL), dtype=T16[prec]).cuda()
        sparse.conv(x.features, sparse.subm_table(x), x.n, packed, 16, 16, x.status, out=out, precision=prec, out16=out16)
        if refused:
            assert int(x.status.item()) == hip.SP_BAD_WEIGHT and bool((out == SENTINEL).all()) and bool((out16 == SENTINEL).all())
        else:
            assert int(x.status.item()) == 0 and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 1.0e5
    # float32 packs the same weight as it is
    status = torch.zeros(1, dtype=torch.int32).cuda()
    sparse.pack_layer(conv, None, status)
    assert int(status.item()) == 0


# ------------------------------------------------------------------------------------- the whole backbone
_MODEL = {}


def model_case(c_in, prec):
    if (c_in, prec) not in _MODEL:
        feats, idx, B, shape = S.backbone_case(c_in)
        _MODEL[c_in, prec] = L.backbone(S.backbone_weights(c_in), feats, idx, shape, prec, B=B)
    return _MODEL[c_in, prec]


def hold_chain(row, got, model, truth):
    """the chain bar: the kernel's error against the unrounded float64 truth over the model's error against it"""
    e, m = L.errors(got, truth), L.errors(model, truth)
    ratio = {k: e[k] / m[k] for k in e}
    _LP_RECORD[row] = {"measured": e, "model": m, "ratio": ratio}
    for k, slack in (("rms", RMS_SLACK), ("max", MODEL_SLACK)):
        print(f"{row:34s} {k:4s} {e[k]:10.3e}  model {m[k]:10.3e}  ratio {ratio[k]:6.3f}  slack {slack:g}")
    assert ratio["rms"] <= RMS_SLACK and ratio["max"] <= MODEL_SLACK, (row, ratio)


def _run_backbone(m, feats, idx, B, shape, **kw):
    with torch.no_grad():
        return m(_dev(feats), _dev(idx), B, [shape[2], shape[1], shape[0] - 1], **kw)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c_in", (5, 6))
def test_backbone_against_the_model(c_in, prec):
    feats, idx, B, shape, truth, _ = backbone_truth(c_in)
    m = backbone_module(c_in)
    bev32, levels32 = _run_backbone(m, feats, idx, B, shape)
    m.sparse_precision = prec
    bev, levels = _run_backbone(m, feats, idx, B, shape)
    assert int(m.last_status.item()) == 0 and bev.dtype == torch.float32 and bev.shape == bev32.shape and not torch.equal(bev, bev32)
    model = model_case(c_in, prec)
    got = bev.cpu().numpy()
    inactive = np.abs(truth["bev"]).max(1) == 0
    cells = np.moveaxis(got, 1, -1)[inactive]
    assert not cells.any() and not np.signbit(cells).any()
    hold_chain(f"lp/{prec}/backbone/{c_in}/bev", got, model["bev"], truth["bev"])
    assert list(levels) == list(S.LEVELS)
    for k in S.LEVELS:
        x, x32 = levels[k], levels32[k]
        # the sites are the fp32 route's exactly; the rows are float32 with their 16-bit twin beside them
        assert (x.n is None and x32.n is None) or torch.equal(x.n, x32.n)
        n = x.capacity if x.n is None else int(x.n.item())
        assert n > 0 and torch.equal(x.indices[:n], x32.indices[:n]) and x.spatial_shape == x32.spatial_shape and x.capacity == x32.capacity
        assert x.features.dtype == torch.float32 and x.features16.dtype == T16[prec] and x32.features16 is None
        assert torch.equal(x.features16[:n], x.features[:n].to(T16[prec]))
        hold_chain(f"lp/{prec}/backbone/{c_in}/{k}", x.dense().cpu().numpy(), model[k], truth[k])
    # the bits depend on neither the grid nor the input's capacity
    for mw in (1, 3):
        bev2, levels2 = _run_backbone(m, feats, idx, B, shape, max_workgroups=mw)
        assert torch.equal(bev, bev2) and all(torch.equal(levels[k].dense(), levels2[k].dense()) for k in S.LEVELS)
    n = idx.shape[0]
    pad_f = np.concatenate([feats, np.full((29, c_in), np.nan, np.float32)])
    pad_i = np.concatenate([idx, np.full((29, 4), SENTINEL, np.int32)])
    bev3, _ = _run_backbone(m, pad_f, pad_i, B, shape, n_voxels=torch.tensor([n], dtype=torch.int64).cuda())
    assert torch.equal(bev, bev3)
    m.sparse_precision = "fp32"
    assert torch.equal(_run_backbone(m, feats, idx, B, shape)[0], bev32)


def test_backbone_enqueues_without_a_synchronisation_and_train_forward_ignores_the_knob():
    feats, idx, B, shape, _, _ = backbone_truth(5)
    m = backbone_module(5)
    m.sparse_precision = "fp16"
    df, di = _dev(feats), _dev(idx)
    n = torch.tensor([idx.shape[0]], dtype=torch.int64).cuda()
    voxel_shape = [shape[2], shape[1], shape[0] - 1]
    with torch.no_grad():
        want = m(df, di, B, voxel_shape)[0]                     # warms every pack
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            bev, _ = m(df, di, B, voxel_shape, n_voxels=n)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(bev, want)
    with pytest.raises(RuntimeError, match="eval-mode"):
        m.train()(df, di, B, voxel_shape)
    a, b = backbone_module(5).train(), backbone_module(5).train()
    b.sparse_precision = "bf16"
    with torch.no_grad():
        assert torch.equal(a.train_forward(df, di, B, voxel_shape)[0], b.train_forward(df, di, B, voxel_shape)[0])


# ------------------------------------------------------------------------------------- the detector door
def test_voxelnet_door():
    import test_gpu_rpn_lp as D
    import test_gpu_voxelnet as V
    pillars = importlib.import_module("3dal_pytorch_amd.pillars")
    m = V.detector.VoxelNet(**V.MODEL, test_cfg=V.TEST_CFG, **V.KW)
    m.load_state_dict(V.checkpoint(), strict=True)
    m = m.cuda().eval()
    pts, off = V.sweep()
    dpts = _dev(pts)
    want = m.detect(dpts, off, metadata=V.META)
    r = pillars.voxelize(dpts, off, V.VOXEL, V.RANGE, 5, 4000)
    voxels, coords, num, nv = r.finish()

    def stages():
        with torch.no_grad():
            bev, _ = m.backbone(m.reader(voxels, num), coords, 2, V.GRID)
            n = m.neck(bev)
            return bev, n, m.bbox_head(n)

    bev, n, preds = stages()
    m.sparse_precision = "fp16"
    assert m.backbone.sparse_precision == "fp16" and m.precision == m.neck.precision == "fp32"
    D._structure(m.detect(dpts, off, metadata=V.META), want)
    bev16, n16, preds16 = stages()
    assert not torch.equal(bev16, bev) and int(m.backbone.last_status.item()) == 0
    # the truth and the model chained over THIS detector from its own state dict
    sd = {k: v.cpu().numpy() for k, v in m.state_dict().items()}
    bsd = {k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}
    nsd = {k[len("neck."):]: v for k, v in sd.items() if k.startswith("neck.")}
    hsd = {k[len("bbox_head."):]: v for k, v in sd.items() if k.startswith("bbox_head.")}
    cfg = V.MODEL["neck"]
    with torch.no_grad():
        feats = m.reader(voxels, num).cpu().numpy()
    idx, shape = coords.cpu().numpy().astype(np.int32), (V.GRID[2] + 1, V.GRID[1], V.GRID[0])
    b64 = L.backbone(bsd, feats, idx, shape, "f64", B=2)["bev"]
    b16 = L.backbone(bsd, feats, idx, shape, "fp16", B=2)["bev"].astype(np.float32)
    assert b64.shape == tuple(bev.shape) and np.abs(b64).max() > 0
    n64 = M.neck(nsd, b64, "f64", cfg=cfg)
    h64 = R.head_cat(M.head(hsd, n64, "f64"))
    hold_chain("lp/fp16/voxelnet/bev", bev16.cpu().numpy(), b16, b64)
    m_n = M.neck(nsd, b16, "fp32", cfg=cfg)                  # the sparse middle alone on 16-bit operands
    hold_chain("lp/fp16/voxelnet/neck_alone", n16.cpu().numpy(), m_n, n64)
    hold_chain("lp/fp16/voxelnet/head_alone", D._cat(preds16), R.head_cat(M.head(hsd, m_n, "fp32")), h64)
    m.precision = "fp16"                                       # ... and combined with the dense stage's knob
    assert m.sparse_precision == "fp16"
    D._structure(m.detect(dpts, off, metadata=V.META), want)
    bev_b, n_b, preds_b = stages()
    assert torch.equal(bev_b, bev16) and not torch.equal(n_b, n16)
    m_n = M.neck(nsd, b16, "fp16", cfg=cfg)
    hold_chain("lp/fp16/voxelnet/neck_both", n_b.cpu().numpy(), m_n, n64)
    hold_chain("lp/fp16/voxelnet/head_both", D._cat(preds_b), R.head_cat(M.head(hsd, m_n, "fp16")), h64)
    m.precision = "fp32"
    m.sparse_precision = "fp32"
    bev_again, n_again, _ = stages()
    assert torch.equal(bev_again, bev) and torch.equal(n_again, n)
    got = m.detect(dpts, off, metadata=V.META)
    assert all(torch.equal(g[k], w[k]) for g, w in zip(got, want) for k in ("box3d_lidar", "scores", "label_preds"))


def test_pointpillars_refuses_the_knob():
    import test_gpu_detector as PP
    m = PP.detector.PointPillars(**PP.MODEL, test_cfg=PP.TEST_CFG, max_points=20, max_voxels=2000)
    with pytest.raises(ValueError, match="no sparse convolutions"):
        m.sparse_precision = "fp16"
    assert m.sparse_precision == "fp32"
