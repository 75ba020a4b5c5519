"""CPU-side checks of the sparse backbone's training pass (sparse.py's train_forward; dal3_sp_table_transposed and
dal3_sp_wgrad of include/dal3.h): sparse_train_ref's two differentiable float64 formulations against each other, the inverse
tables against the brute-force inverse, the planted faults against the bars, batch_norm_rows against nn.BatchNorm1d on the
live rows, the ABI's layout through a C compiler and every refusal made before a launch. No GPU compute here."""
import ctypes
import functools
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

import sparse_ref as S
import sparse_train_ref as T
from _common import ROOT

hip = importlib.import_module("3dal_pytorch_amd._hip")
sparse = importlib.import_module("3dal_pytorch_amd.sparse")
detector = importlib.import_module("3dal_pytorch_amd.detector")

ENTRIES = ("dal3_sp_table_transposed", "dal3_sp_wgrad_workspace_bytes", "dal3_sp_wgrad")
FORMS = {"subm": ((3, 3, 3), (1, 1, 1), (1, 1, 1), True), "k3s2p1": ((3, 3, 3), (2, 2, 2), (1, 1, 1), False),
         "k3s2p011": ((3, 3, 3), (2, 2, 2), (0, 1, 1), False), "k311s211": ((3, 1, 1), (2, 1, 1), (0, 0, 0), False)}


@pytest.fixture(autouse=True)
def _grad_on():
    """whatever a test before this file left switched"""
    with torch.enable_grad():
        yield


@functools.lru_cache(maxsize=None)
def case():
    feats, idx, B, shape = T.train_case(5)
    sd = S.backbone_weights(5)
    cot = T.cotangent("bev", (B, 128, 4, 5))
    rule = T.RuleT(B)
    return (feats, idx, B, shape, sd, cot, T.backbone_train(T.DenseT(B), sd, feats, idx, shape, cot),
            T.backbone_train(T.DenseT(B, torch.float32), sd, feats, idx, shape, cot), rule,
            T.backbone_train(rule, sd, feats, idx, shape, cot))


def _layer_case():
    """a 16 -> 16 submanifold layer with a bias and no BatchNorm behind it: where a bias gradient is not zero"""
    shape, B = (11, 13, 15), 2
    idx = S.batch([S.clustered("layer/16/0", shape, 2, 90, 1.6), S.clustered("layer/16/1", shape, 1, 60, 1.2)])
    feats = S.synth.uniform(S.SEED, "trlayer/x", (idx.shape[0], 16), 0.0, 2.0).astype(np.float32)
    w, b, _ = S.layer_weights("trlayer/16-16", (3, 3, 3), 16, 16, True, False)
    return (feats, idx, shape, w, b, (3, 3, 3), (1, 1, 1), (1, 1, 1), True, T.cotangent("trlayer", (B, 16, *shape))), B


def test_the_two_formulations_agree():
    feats, idx, B, shape, sd, cot, (out, grads, stats), _, rule, (out2, grads2, stats2) = case()
    sites = (idx.shape[0],) + tuple(rule.record[k]["indices"].shape[0] for k in ("conv2", "conv3", "conv4", "extra_conv"))
    assert sites == T.TRAIN_SITES
    assert out["bev"].shape == (4, 128, 4, 5)
    for k in ("bev",) + S.LEVELS:
        assert np.abs(out[k] - out2[k]).max() <= 1e-12 * np.abs(out[k]).max(), k
        for b in (0, 1):                                    # no sample saturates any level
            act = np.abs(out[k][b]).max(0) > 0
            assert act.any() and not act.all(), (k, b)
    assert int((np.abs(out["bev"]).max(1) > 0).sum()) >= 16
    assert set(grads) == set(grads2) == {k for k in sd if k.endswith(("weight", "bias"))}
    assert set(stats) == set(stats2) == {k for k in sd if k.endswith(("running_mean", "running_var"))}
    scale = max(np.abs(g).max() for g in grads.values())
    for k in grads:
        if T.zero_by_batchnorm(k):                          # a bias in front of a train-mode BatchNorm: rounding noise only
            assert max(np.abs(grads[k]).max(), np.abs(grads2[k]).max()) <= 1e-12 * scale, k
        else:
            assert np.abs(grads[k]).max() > 0 and np.abs(grads[k] - grads2[k]).max() <= 1e-12 * np.abs(grads[k]).max(), k
    for k in stats:
        assert np.abs(stats[k] - stats2[k]).max() <= 1e-12 * np.abs(stats[k]).max(), k
        assert np.abs(stats[k] - np.asarray(sd[k], np.float64)).max() > 0
    # single layers: the four forms, with the input gradient
    for form, (kernel, stride, padding, subm) in FORMS.items():
        f16 = S.synth.uniform(S.SEED, f"agree/{form}", (idx.shape[0], 16), 0.0, 2.0)
        w, b, _ = S.layer_weights(f"agree/{form}", kernel, 16, 32, True, False)
        osh = shape if subm else S.out_shape(shape, kernel, stride, padding)
        c = T.cotangent(f"agree/{form}", (B, 32, *osh))
        a = T.layer_train(T.DenseT(B), f16, idx, shape, w, b, kernel, stride, padding, subm, c)
        r = T.layer_train(T.RuleT(B), f16, idx, shape, w, b, kernel, stride, padding, subm, c)
        for k in ("y", "dx", "dW", "db"):
            assert np.abs(a[k]).max() > 0 and np.abs(a[k] - r[k]).max() <= 1e-12 * np.abs(a[k]).max(), (form, k)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_inverse_tables_are_the_brute_force_inverse(form):
    kernel, stride, padding, subm = FORMS[form]
    for shape in ((11, 13, 15), (6, 7, 9)):                 # the even depth: on (3,1,1)/(2,1,1) the last plane has no output site
        B = 2
        idx = S.batch([S.clustered(f"inv/{shape[0]}/0", shape, 2, 90, 1.6), S.clustered(f"inv/{shape[0]}/1", shape, 1, 60, 1.2)])
        if subm:
            t = S.table(idx, idx, B, shape, shape, kernel, stride, padding)
            assert np.array_equal(T.inverse_subm(t), T.inverse_brute(t, idx.shape[0]))
            continue
        oidx, osh = S.downsample(idx, B, shape, kernel, stride, padding)
        t = S.table(oidx, idx, B, shape, osh, kernel, stride, padding)
        inv = T.inverse_table(idx, oidx, B, shape, osh, kernel, stride, padding)
        assert np.array_equal(inv, T.inverse_brute(t, idx.shape[0]))
        assert (inv >= 0).any(1).all()                      # every tap is exercised
        orphan = (inv < 0).all(0)
        if form == "k311s211" and shape[0] % 2 == 0:
            assert orphan.any() and (idx[orphan, 1] == shape[0] - 1).all()
        elif form != "k3s2p011":
            assert not orphan.any()


def _worst(got, f32, truth):
    return {k: max(T.S.P.ratios(T.as_rows(g), T.as_rows(y), T.as_rows(t))[0][k] for g, y, t in zip(got, f32, truth)) for k in T.MEASURES}


def _quantities(res, layer):
    out, grads, stats = res
    keys = [k for k in sorted(grads) if not T.zero_by_batchnorm(k)]
    return [S.rows_of(out["bev"])] + [grads[k] for k in keys] + [stats[k] for k in sorted(stats)] + \
        [layer[k] for k in ("dx", "dW", "db")]


def test_planted_faults_are_caught_at_ten_times_the_bars():
    feats, idx, B, shape, sd, cot, truth, f32, _, _ = case()
    largs, LB = _layer_case()
    lt, lf = T.layer_train(T.DenseT(LB), *largs), T.layer_train(T.DenseT(LB, torch.float32), *largs)
    qt, qf = _quantities(truth, lt), _quantities(f32, lf)
    sane = _worst(_quantities(case()[9], T.layer_train(T.RuleT(LB), *largs)), qf, qt)
    assert all(sane[k] < 1e-3 for k in T.MEASURES)          # without a fault the float64 rulebook is far inside the yardstick
    smallest = np.inf
    for fault in T.FAULTS:
        wrong = _quantities(T.backbone_train(T.RuleT(B, fault=fault), sd, feats, idx, shape, cot),
                            T.layer_train(T.RuleT(LB, fault=fault), *largs))
        ratio = _worst(wrong, qf, qt)
        print(fault, ratio)
        for k in T.MEASURES:
            assert ratio[k] >= 10 * T.BARS[k], (fault, k, ratio[k])
            smallest = min(smallest, ratio[k])
    assert all(T.BARS[k] < smallest / 10 for k in T.MEASURES)


def test_batch_norm_rows_is_batchnorm1d_on_the_live_rows():
    torch.manual_seed(3)
    cap, n, C = 50, 37, 16
    x = torch.randn(cap, C, dtype=torch.float64)
    x[n:] = float("nan")                                    # the dead rows
    cot = torch.randn(n, C, dtype=torch.float64)
    for train in (True, False):
        ref, bn = nn.BatchNorm1d(C, eps=1e-3, momentum=0.01).double(), nn.BatchNorm1d(C, eps=1e-3, momentum=0.01).double()
        for m in (ref, bn):
            torch.manual_seed(4)
            m.weight.data.uniform_(0.5, 1.5), m.bias.data.uniform_(-1, 1), m.running_mean.uniform_(-1, 1), m.running_var.uniform_(0.5, 2)
            m.train(train)
        a = x[:n].clone().requires_grad_()
        want = ref(a)
        (want * cot).sum().backward()
        b = x.clone().requires_grad_()
        y = sparse.batch_norm_rows(bn, b, torch.tensor([n]))
        (y[:n] * cot).sum().backward()
        assert torch.allclose(y[:n], want, rtol=1e-10, atol=1e-12) and not y[n:].any() and not torch.signbit(y[n:]).any()
        assert torch.allclose(b.grad[:n], a.grad, rtol=1e-10, atol=1e-12) and not b.grad[n:].any()
        for k in ("weight", "bias"):
            assert torch.allclose(getattr(bn, k).grad, getattr(ref, k).grad, rtol=1e-10, atol=1e-12), k
        assert torch.allclose(bn.running_mean, ref.running_mean, rtol=1e-12) and torch.allclose(bn.running_var, ref.running_var, rtol=1e-12)
        assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == (1 if train else 0)
    # no count: every row; a count of 0 or 1: finite, and the running statistics stay
    bn = nn.BatchNorm1d(C, eps=1e-3, momentum=0.01).double().train()
    ref = nn.BatchNorm1d(C, eps=1e-3, momentum=0.01).double().train()
    assert torch.allclose(sparse.batch_norm_rows(bn, x[:n]), ref(x[:n]))
    before = (bn.running_mean.clone(), bn.running_var.clone())
    for k in (0, 1):
        y = sparse.batch_norm_rows(bn, x, torch.tensor([k]))
        assert torch.isfinite(y).all() and not y[k:].any()
        assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])
    assert int(bn.num_batches_tracked) == 3
    with pytest.raises(RuntimeError, match="BatchNorm1d"):
        sparse.batch_norm_rows(nn.BatchNorm1d(C, affine=False), x)


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dal3.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRIES:
        assert name + "(" in header and name in hip.SIGNATURES and hasattr(lib, name), name
    assert "DAL3_SP_WGRAD_SLICE = 1024" in header and hip.SP_WGRAD_SLICE == 1024


def test_the_workspace_is_one_partial_per_slice():
    lib = hip.lib()
    al = lambda b: (b + 255) & ~255
    size = lambda taps, ci, co, cap: al(4 * -(-cap // hip.SP_WGRAD_SLICE) * taps * ci * co) + al(4 * -(-cap // hip.SP_WGRAD_SLICE) * co)
    for args in ((27, 16, 16, 1), (27, 5, 16, 1024), (27, 64, 128, 1025), (3, 128, 128, 5000), (27, 16, 32, 0)):
        assert lib.dal3_sp_wgrad_workspace_bytes(*args) == size(*args), args
    for bad in ((0, 16, 16, 10), (28, 16, 16, 10), (27, 9, 16, 10), (27, 16, 48, 10), (27, 16, 16, -1)):
        assert lib.dal3_sp_wgrad_workspace_bytes(*bad) == 0


FAKE = 0x1000                                   # never dereferenced: every case fails before a launch
I3 = ctypes.c_int32 * 3


def _err(rc, word):
    assert rc == hip.EINVAL and word.encode() in hip.lib().dal3_last_error(), hip.lib().dal3_last_error()


def test_the_c_abi_refuses_bad_arguments_before_any_launch():
    lib = hip.lib()
    tr = lambda **kw: hip.SpTableTransposedArgs(**dict(dict(B=1, in_shape=I3(5, 5, 6), out_shape=I3(2, 5, 6), kernel=I3(3, 1, 1),
                                                            stride=I3(2, 1, 1), padding=I3(0, 0, 0), in_capacity=8, in_indices=FAKE,
                                                            out_capacity=8, out_key=FAKE, table=FAKE), **kw))
    _err(lib.dal3_sp_table_transposed(None, None), "null args")
    _err(lib.dal3_sp_table_transposed(tr(table=None), None), "null in_indices / table")
    _err(lib.dal3_sp_table_transposed(tr(in_indices=None), None), "null in_indices / table")
    _err(lib.dal3_sp_table_transposed(tr(out_key=None), None), "null out_key")
    _err(lib.dal3_sp_table_transposed(tr(out_shape=I3(3, 5, 6)), None), "out_shape[0]")
    _err(lib.dal3_sp_table_transposed(tr(kernel=I3(4, 1, 1)), None), "kernel 1 .. 3")
    _err(lib.dal3_sp_table_transposed(tr(B=0), None), "bad B")
    _err(lib.dal3_sp_table_transposed(tr(max_workgroups=-1), None), "max_workgroups")
    _err(lib.dal3_sp_table_transposed(tr(reserved=1), None), "reserved")
    _err(lib.dal3_sp_table_transposed(tr(in_capacity=-1), None), "capacity")
    wg = lambda **kw: hip.SpWgradArgs(**dict(dict(taps=27, c_in=16, c_out=32, in_capacity=8, x=FAKE, out_capacity=8, table=FAKE, dy=FAKE,
                                                  dw=FAKE, db=FAKE, workspace=FAKE, workspace_bytes=1 << 20), **kw))
    _err(lib.dal3_sp_wgrad(None, None), "null args")
    _err(lib.dal3_sp_wgrad(wg(c_in=24), None), "channels")
    _err(lib.dal3_sp_wgrad(wg(c_out=8), None), "channels")
    _err(lib.dal3_sp_wgrad(wg(taps=28), None), "taps")
    _err(lib.dal3_sp_wgrad(wg(max_workgroups=-1), None), "max_workgroups")
    _err(lib.dal3_sp_wgrad(wg(reserved=1), None), "reserved")
    _err(lib.dal3_sp_wgrad(wg(out_capacity=-1), None), "capacity")
    _err(lib.dal3_sp_wgrad(wg(dw=None), None), "null dw")
    _err(lib.dal3_sp_wgrad(wg(dy=None), None), "null table / dy / x")
    _err(lib.dal3_sp_wgrad(wg(table=None), None), "null table / dy / x")
    _err(lib.dal3_sp_wgrad(wg(x=None), None), "null table / dy / x")
    _err(lib.dal3_sp_wgrad(wg(workspace=None), None), "null workspace")
    _err(lib.dal3_sp_wgrad(wg(workspace=FAKE + 4), None), "8-byte aligned")
    assert lib.dal3_sp_wgrad(wg(workspace_bytes=16), None) == hip.EWORKSPACE


def test_python_refusals():
    f, i = torch.zeros(4, 16), torch.zeros(4, 4, dtype=torch.int32)
    conv = sparse.SubMConv3d(16, 16, 3, indice_key="k")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv.train_forward(SimpleNamespace(features=f))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sparse.wgrad(f, torch.zeros(27, 4, dtype=torch.int32), None, f, (3, 3, 3))
    for cls, c in ((sparse.SubMConv3d, 5), (sparse.SparseConv3d, 6)):
        with pytest.raises(RuntimeError, match="no data gradient"):
            cls(c, 16, 3).train_forward(SimpleNamespace(features=torch.zeros(4, c, requires_grad=True)))
    m = sparse.SpMiddleResNetFHD(num_input_features=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.train_forward(f[:, :5].contiguous(), i, 1, [45, 37, 40])
    with pytest.raises(RuntimeError, match="no data gradient"):
        m.conv_input[0].train_forward(SimpleNamespace(features=torch.zeros(4, 5, requires_grad=True)))
    with pytest.raises(RuntimeError, match="eval-mode"):    # forward in train mode stays refused
        m.train()(f, i, 1, [45, 37, 40])
    for name in ("SubMConv3d", "SparseConv3d", "SparseBasicBlock", "SpMiddleResNetFHD"):
        assert callable(getattr(getattr(sparse, name), "train_forward"))
    assert callable(detector.VoxelNet.first_stage_loss)
