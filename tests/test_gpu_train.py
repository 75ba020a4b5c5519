"""Training forward/backward of the shared-MLP stacks on the HIP training kernels against
torch autograd over the stock-torch composite of the same modules, evaluated in FLOAT64 (the composite is what the
train drivers ran before; tests/test_host_cpu.py ties it to the oracle). Tolerance: 1e-4 of each tensor's largest
entry, for outputs, running statistics and every parameter gradient. For scale: the same composite in fp32
through stock PyTorch-ROCm ops is 2e-4 .. 1e-3 away from the float64 gradients (a one-off script of round 2, since deleted); the HIP path
(exact-fp32 MFMA, float64 batch statistics) is ~1e-5 away."""
import copy
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _common import build_model, synth

train = importlib.import_module("3dal_pytorch_amd.train")
hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def _ref_ins_seg(m, pts, mul):
    """PointNetInstanceSeg.forward (static_model.py:271-295) with the Dropout draw replaced by `mul` (B,128,N)"""
    n = pts.size(2)
    o1 = F.relu(m.bn1(m.conv1(pts)))
    o2 = F.relu(m.bn2(m.conv2(o1)))
    o3 = F.relu(m.bn3(m.conv3(o2)))
    o4 = F.relu(m.bn4(m.conv4(o3)))
    o5 = F.relu(m.bn5(m.conv5(o4)))
    g = torch.max(o5, 2, keepdim=True)[0]
    x = torch.cat([o2, g.expand(-1, -1, n)], 1)
    x = F.relu(m.dbn1(m.dconv1(x)))
    x = F.relu(m.dbn2(m.dconv2(x)))
    x = F.relu(m.dbn3(m.dconv3(x)))
    x = F.relu(m.dbn4(m.dconv4(x)))
    x = m.dconv5(x * mul)
    return x.transpose(2, 1).contiguous()


def _close(got, want, scale_all=0.0):
    want = want.double()
    return float((got.double() - want).abs().max()) <= 1e-4 * float(want.abs().max()) + 1e-7 * scale_all


def test_ins_seg_training_step_matches_float64_autograd():
    """whole network, strict. fp32 and float64 forward passes can disagree on a discrete decision (a ReLU input or
    two pooled candidates within rounding of each other), which reroutes gradient and is not an arithmetic error;
    this configuration has no such case (the kernels are deterministic, so that is stable), the layer-level tests
    below cover the arithmetic at larger sizes on tie-free data, and the next test covers a larger network run."""
    B, N = 4, 256
    model = build_model("static_one", synth.state_dict("static_one", seed=21))
    ours = model.ins_seg.train()
    ref = copy.deepcopy(ours).double()
    pts = torch.from_numpy(synth.static_crops(B, N, seed=21)[0]).cuda().transpose(2, 1)
    mul = (torch.from_numpy(synth.uniform(21, "drop", (B, N, 128))).cuda() >= 0.5).float() * 2.0
    weight = torch.from_numpy(synth.normal(21, "lw", (B, N, 2)).astype(np.float32)).cuda()

    want = _ref_ins_seg(ref, pts.double(), mul.transpose(2, 1).double())
    (want * weight.double()).sum().backward()
    got = train.ins_seg_train_forward(ours, pts, drop_mask=mul.reshape(B * N, 128))
    (got * weight).sum().backward()

    assert _close(got.detach(), want.detach())
    gmax = max(float(q.grad.abs().max()) for q in ref.parameters())
    for (name, p), (_, q) in zip(ours.named_parameters(), ref.named_parameters()):
        # analytically-zero gradients (a conv bias in front of a train-mode BN; bn5.bias) are ~1e-13 in float64:
        # the absolute term covers them
        assert _close(p.grad, q.grad, gmax), name
        if ".bias" in name and "conv" in name and not name.startswith("dconv5"):
            assert float(p.grad.abs().max()) == 0.0 and float(q.grad.abs().max()) < 1e-9 * gmax
    for (name, b1), (_, b2) in zip(ours.named_buffers(), ref.named_buffers()):
        if name.endswith("num_batches_tracked"):
            assert int(b1) == int(b2)
        else:
            assert _close(b1, b2), name


@pytest.mark.parametrize("B,N", [(3, 100), (5, 77), (1, 1000), (2, 8192)])
def test_ins_seg_training_step_ragged_sizes_match_float64_autograd(B, N):
    """B*N not a multiple of 32 (300, 385, 1000 points; N not a multiple of 32 either: conv5 and the pooling run as
    two kernels), and 8192 points per crop (the pooled layer's sparse terms no longer fit the library's per-item LDS
    buckets: the stock-op path): outputs, running statistics and every gradient against float64 autograd, as in the test above. The
    yardstick for a gradient that a discrete decision rerouted is the stock fp32 composite's own distance."""
    model = build_model("static_one", synth.state_dict("static_one", seed=21))
    ours = model.ins_seg.train()
    ref32, ref64 = copy.deepcopy(ours), copy.deepcopy(ours).double()
    pts = torch.from_numpy(synth.static_crops(B, N, seed=21 + N)[0]).cuda().transpose(2, 1)
    mul = (torch.from_numpy(synth.uniform(21, "drop", (B, N, 128))).cuda() >= 0.5).float() * 2.0
    weight = torch.from_numpy(synth.normal(21, "lw", (B, N, 2)).astype(np.float32)).cuda()
    w64 = _ref_ins_seg(ref64, pts.double(), mul.transpose(2, 1).double())
    (w64 * weight.double()).sum().backward()
    w32 = _ref_ins_seg(ref32, pts, mul.transpose(2, 1))
    (w32 * weight).sum().backward()
    got = train.ins_seg_train_forward(ours, pts, drop_mask=mul.reshape(B * N, 128))
    (got * weight).sum().backward()
    assert got.shape == (B, N, 2) and _close(got.detach(), w64.detach())
    gmax = max(float(q.grad.abs().max()) for q in ref64.parameters())
    for (name, p), (_, q), (_, r) in zip(ours.named_parameters(), ref32.named_parameters(), ref64.named_parameters()):
        if _close(p.grad, r.grad, gmax):
            continue
        if float(r.grad.abs().max()) < 1e-6 * gmax:                    # analytically zero (B = 1: the pooled feature is
            assert float(p.grad.abs().max()) < 1e-5 * gmax, name      # one row, dbn1 removes it, conv3..5 get nothing)
            continue
        mine, stock = _rel(p.grad.double(), r.grad), _rel(q.grad.double(), r.grad)
        assert mine < 2e-2 and mine < 1.5 * stock + 1e-4, (name, mine, stock)
    for (name, b1), (_, b2) in zip(ours.named_buffers(), ref64.named_buffers()):
        if not name.endswith("num_batches_tracked"):
            assert _close(b1, b2), name
    # the random-Dropout path at a ragged size: runs, and the backward re-creates the forward's multiplier
    out = train.ins_seg_train_forward(ours, pts)
    out.sum().backward()
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(p.grad).all()) for p in ours.parameters())


def test_ins_seg_training_step_larger_batch_is_as_close_to_float64_as_stock_fp32():
    """B*N = 3072 points (several wgrad slices, odd tile counts). Here one discrete decision differs from the
    float64 run, so the yardstick is the stock PyTorch-ROCm fp32 composite's own distance from float64."""
    B, N = 3, 1024
    model = build_model("static_one", synth.state_dict("static_one", seed=21))
    ours = model.ins_seg.train()
    ref32, ref64 = copy.deepcopy(ours), copy.deepcopy(ours).double()
    pts = torch.from_numpy(synth.static_crops(B, N, seed=21)[0]).cuda().transpose(2, 1)
    mul = (torch.from_numpy(synth.uniform(21, "drop", (B, N, 128))).cuda() >= 0.5).float() * 2.0
    weight = torch.from_numpy(synth.normal(21, "lw", (B, N, 2)).astype(np.float32)).cuda()
    w64 = _ref_ins_seg(ref64, pts.double(), mul.transpose(2, 1).double())
    (w64 * weight.double()).sum().backward()
    w32 = _ref_ins_seg(ref32, pts, mul.transpose(2, 1))
    (w32 * weight).sum().backward()
    got = train.ins_seg_train_forward(ours, pts, drop_mask=mul.reshape(B * N, 128))
    (got * weight).sum().backward()
    assert _close(got.detach(), w64.detach())
    for (name, p), (_, q), (_, r) in zip(ours.named_parameters(), ref32.named_parameters(), ref64.named_parameters()):
        if float(r.grad.abs().max()) < 1e-6:
            continue                                                    # analytically zero, see above
        mine, stock = _rel(p.grad.double(), r.grad), _rel(q.grad.double(), r.grad)
        assert mine < 2e-2 and mine < 1.5 * stock + 1e-4, (name, mine, stock)


def _tie_free(z, gamma, beta, margin=1e-3):
    """nudge entries of z until no relu(bn(z)) input lies within `margin` of zero (float64 statistics)"""
    z = z.double().clone()
    for _ in range(20):
        mu, var = z.mean(0), z.var(0, unbiased=False)
        y = (z - mu) * torch.rsqrt(var + 1e-5) * gamma.double() + beta.double()
        near = y.abs() < margin
        if not bool(near.any()):
            return z.float()
        z[near] += 0.05 * torch.sign(gamma.double().expand_as(z)[near])
    raise AssertionError("could not make the data tie-free")


def test_linear_dgrad_wgrad_kernels_vs_float64():
    M, ci, co = 4128, 96, 160                                           # 129 point tiles, 3 wgrad slices, ragged tile blocks
    rnd = lambda tag, shape, std=1.0: torch.from_numpy(synth.normal(30, tag, shape, 0.0, std).astype(np.float32)).cuda()
    a, W, b = rnd("a", (M, ci)), rnd("W", (co, ci), 0.2), rnd("b", (co,))
    sc, sh = rnd("sc", (ci,)).abs() + 0.5, rnd("sh", (ci,), 0.3)
    act64 = torch.relu(a.double() * sc.double() + sh.double())
    z = train._linear(a, W, ci, ci, co, act=(sc, sh, True), bias=b)
    want = act64 @ W.double().t() + b.double()
    assert _close(z, want)
    seg = M // 3                                                        # per-segment bias (the decoder's per-crop term)
    gb = rnd("gb", (3, co))
    z2 = train._linear(a, W, ci, ci, co, act=(sc, sh, True), bias=gb, seg=seg)
    assert _close(z2, act64 @ W.double().t() + gb.double().repeat_interleave(seg, 0))
    dz = rnd("dz", (M, co))
    da = train._linear(dz, W, ci, co, ci, transpose=True)               # dgrad through the same weight
    assert _close(da, dz.double() @ W.double())
    acc = da.clone()
    train._linear(dz, W, ci, co, ci, transpose=True, out=acc, accumulate=True)
    assert _close(acc, 2 * (dz.double() @ W.double()))
    Wwide = rnd("Ww", (co, ci + 64), 0.2)                               # a column block of a wider matrix (dconv1)
    z3 = train._linear(a, Wwide, ci + 64, ci, co)
    assert _close(z3, a.double() @ Wwide[:, :ci].double().t())
    dW = train._wgrad(dz, a, co, ci, act=(sc, sh, True))
    assert _close(dW, dz.double().t() @ act64)
    assert _close(train._wgrad(dz, a, co, ci), dz.double().t() @ a.double())


def test_batchnorm_relu_backward_and_pooling_kernels_vs_float64_autograd():
    M, C, seg = 4128, 96, 1376
    rnd = lambda tag, shape, std=1.0: torch.from_numpy(synth.normal(31, tag, shape, 0.0, std).astype(np.float32)).cuda()
    gamma, beta = rnd("g", (C,)).abs() + 0.5, rnd("b", (C,), 0.3)
    z = _tie_free(rnd("z", (M, C)) * 3.0 + 1.0, gamma, beta)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    bn = train._BN(z, gamma, beta, rm, rv)
    z64 = z.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref_bn = torch.nn.BatchNorm1d(C).cuda().double().train()
    y64 = torch.relu(F.batch_norm(z64, ref_bn.running_mean, ref_bn.running_var, g64, b64, True, 0.1, 1e-5))
    assert _close(rm, ref_bn.running_mean) and _close(rv, ref_bn.running_var)
    # dense upstream gradient
    da = rnd("da", (M, C))
    (y64 * da.double()).sum().backward(retain_graph=True)
    dz, dgam, dbet = bn.backward(z, da=da)
    assert _close(dz, z64.grad) and _close(dgam, g64.grad) and _close(dbet, b64.grad)
    # the max over points and its sparse gradient
    g, arg = train._segmax(z, bn, seg)
    want_g, want_arg = y64.detach().reshape(3, seg, C).max(1)
    assert _close(g, want_g) and torch.equal(arg.long(), want_arg)
    z64.grad = g64.grad = b64.grad = None
    dg = rnd("dg", (3, C))
    (y64.reshape(3, seg, C).max(1)[0] * dg.double()).sum().backward()
    dz, dgam, dbet = bn.backward(z, dg=dg, arg=arg, seg=seg)
    assert _close(dz, z64.grad) and _close(dgam, g64.grad) and _close(dbet, b64.grad)
    assert _close(train._segsum(da, seg, 3), da.double().reshape(3, seg, C).sum(1))


def test_ins_seg_random_dropout_and_eval_after_training_step():
    """the default path draws its own Dropout mask; the running statistics it leaves behind are what the eval
    kernels then fold (PackedCache notices the in-place buffer updates)"""
    model = build_model("static_one", synth.state_dict("static_one", seed=23))
    pts_np, init_np, _ = synth.static_crops(4, 256, seed=23)
    pts, init = torch.from_numpy(pts_np).cuda().transpose(2, 1), torch.from_numpy(init_np).cuda()
    before = model.refine(pts, init).clone()
    model.train()
    n0 = int(model.ins_seg.bn1.num_batches_tracked)
    a = train.ins_seg_train_forward(model.ins_seg, pts)
    b = train.ins_seg_train_forward(model.ins_seg, pts)
    assert a.shape == (4, 256, 2) and not torch.equal(a, b)                      # different Dropout draws
    assert int(model.ins_seg.bn1.num_batches_tracked) == n0 + 2
    model.eval()
    after = model.refine(pts, init)
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)


def test_two_forwards_before_their_backwards_keep_their_own_dropout_masks():
    """the backward re-creates the Dropout multiplier from its key (seed, step). The key used to hold the module's
    LIVE device counter, so `loss(model(a)) + loss(model(b))` — two train-mode forwards, then the backwards — gave the
    first graph's backward the counter value of the SECOND forward: another mask than its forward used, wrong gradients,
    no error. The key now carries a snapshot. Two orders of the same two draws must give the same gradients, bit for bit:
    forward a, forward b, backward a, backward b  ==  forward a, backward a, forward b, backward b."""
    pa, _, _ = synth.static_crops(4, 256, seed=31)
    pb, _, _ = synth.static_crops(4, 256, seed=32)
    pa, pb = (torch.from_numpy(x).cuda().transpose(2, 1) for x in (pa, pb))
    wa = torch.from_numpy(synth.normal(31, "w", (4, 256, 2)).astype(np.float32)).cuda()

    def grads(interleaved):
        model = build_model("static_one", synth.state_dict("static_one", seed=23)).train()
        seg = model.ins_seg
        torch.manual_seed(77)                               # the two draws' seeds come from torch's CPU generator
        out = []
        if interleaved:
            for p in (pa, pb):
                seg.zero_grad()
                (train.ins_seg_train_forward(seg, p) * wa).sum().backward()
                out.append([q.grad.clone() for q in seg.parameters()])
        else:
            la = (train.ins_seg_train_forward(seg, pa) * wa).sum()
            lb = (train.ins_seg_train_forward(seg, pb) * wa).sum()
            for loss in (la, lb):
                seg.zero_grad()
                loss.backward()
                out.append([q.grad.clone() for q in seg.parameters()])
        return out
    one, two = grads(True), grads(False)
    for k in range(2):
        for g1, g2 in zip(one[k], two[k]):
            assert torch.equal(g1, g2)
    assert not all(torch.equal(a, b) for a, b in zip(one[0], one[1]))


@pytest.mark.parametrize("kind,attr,B,C,N", [("static_one", "box_est", 6, 3, 512), ("dynamic", "point_emb", 2, 4, 2560),
                                              ("dynamic", "box_emb", 32, 8, 101), ("dynamic", "box_emb", 5, 8, 101),
                                              ("static_one", "box_est", 3, 3, 90)])
def test_point_stack_training_step_matches_float64_autograd(kind, attr, B, C, N):
    """conv1..4 + max of the three point heads; box_emb's 101 boxes per item are not a multiple of 32; the last two
    cases have B*N not a multiple of 32 either (505 and 270 rows: the host pads the row buffers, the statistics and
    every gradient sum run over the real rows only)"""
    model = build_model(kind, synth.state_dict(kind, seed=22))
    ours = getattr(model, attr).train()
    ref = copy.deepcopy(ours).double()
    obj = torch.from_numpy(synth.normal(22, "stack" + attr, (B, N, C)).astype(np.float32)).cuda().transpose(2, 1)
    weight = torch.from_numpy(synth.normal(22, "lw", (B, 512)).astype(np.float32)).cuda()
    x = obj.double()
    for k in range(1, 5):
        x = F.relu(getattr(ref, f"bn{k}")(getattr(ref, f"conv{k}")(x)))
    want = torch.max(x, 2)[0]
    (want * weight.double()).sum().backward()
    got = train.point_stack_train_forward(ours, obj)
    (got * weight).sum().backward()
    assert _close(got.detach(), want.detach())
    gmax = max(float(getattr(ref, f"conv{k}").weight.grad.abs().max()) for k in range(1, 5))
    for k in range(1, 5):
        assert _close(getattr(ours, f"conv{k}").weight.grad, getattr(ref, f"conv{k}").weight.grad, gmax), k
        for part in ("weight", "bias"):
            assert _close(getattr(getattr(ours, f"bn{k}"), part).grad, getattr(getattr(ref, f"bn{k}"), part).grad, gmax)
        assert _close(getattr(ours, f"bn{k}").running_var, getattr(ref, f"bn{k}").running_var)
        assert _close(getattr(ours, f"bn{k}").running_mean, getattr(ref, f"bn{k}").running_mean)


def test_training_kernels_reject_bad_shapes():
    lib = hip.lib()
    a = torch.zeros((64, 32), device="cuda")
    w = torch.zeros((32, 32), device="cuda")
    z = torch.zeros((64, 32), device="cuda")
    assert lib.dal3_tr_linear(hip.ptr(a), 60, 32, 32, None, None, 0, hip.ptr(w), 32, 0, None, 0, 32, hip.ptr(z), 32, 0,
                              None, 0, hip.stream()) != 0
    assert "multiples of 32" in lib.dal3_last_error().decode()      # (the host pads row buffers: see the ragged tests)
    with pytest.raises(RuntimeError):
        train.point_stack_train_forward(build_model("static_one", synth.state_dict("static_one")).box_est.train(),
                                        torch.zeros((2, 3, 100)))                       # CPU tensors: no silent fallback


def _labels_for(B, N, seed, dev):
    rnd = lambda tag, shape, std=1.0: torch.from_numpy(synth.normal(seed, tag, shape, 0.0, std).astype(np.float32)).to(dev)
    return ((torch.from_numpy(synth.uniform(seed, "ml", (B, N))).to(dev) > 0.6).float(), rnd("cl", (B, 3)),
            (torch.from_numpy(synth.uniform(seed, "hc", (B,))).to(dev) * 12).long(), rnd("hr", (B,), 0.1),
            (torch.from_numpy(synth.uniform(seed, "sc", (B,))).to(dev) * 3).long(), rnd("sr", (B, 3), 0.3))


@pytest.mark.parametrize("kind,B", [("static_one", 4), ("static_two", 4), ("dynamic", 4), ("dynamic", 32),
                                    ("static_two", 3), ("dynamic", 3)])    # 3: FC tails / box_emb rows not in 32s
def test_whole_train_step_hip_backend_vs_torch_backend(kind, B):
    """model.train(); forward; the reference's criterion; backward; Adam step — as static_train.py:76-86 does —
    with the per-point stacks on the HIP training kernels vs the stock-torch composite. Dropout off (its draw is
    random); same NumPy stream for the object-point sampling. The two runs share every discrete decision here, so
    losses agree to 1e-4 and the parameters after the step stay within Adam's lr of each other."""
    losses = importlib.import_module("3dal_pytorch_amd.losses")
    out = {}                                                 # dynamic, B=32: the 101-box embedding runs on HIP too
    for backend in ("hip", "torch"):
        model = build_model(kind, synth.state_dict(kind, seed=24)).train()
        model.train_backend = backend
        model.sampler = "numpy"                              # the reference's draws, identical for both backends
        model.ins_seg.dropout.p = 0.0
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        if kind == "dynamic":
            p, bx, _, g = synth.dynamic_items(B, n_per_frame=256, seed=24)
            args = (torch.from_numpy(p).cuda().transpose(2, 1), torch.from_numpy(bx).cuda().transpose(2, 1),
                    torch.from_numpy(g).cuda())
            crit, n = losses.DynamicModelLoss(), p.shape[1]
        else:
            p, i, g = synth.static_crops(B, 1024, seed=24)
            args = (torch.from_numpy(p).cuda().transpose(2, 1), torch.from_numpy(i).cuda(), torch.from_numpy(g).cuda())
            crit = losses.FrustumPointNetLossTwoBoxEst() if kind == "static_two" else losses.FrustumPointNetLossOneBoxEst()
            n = 1024
        np.random.seed(77)
        o = model(*args)
        loss = crit(o, *_labels_for(B, n, 25, "cuda"))
        opt.zero_grad()
        loss["total_loss"].backward()
        grads = {k: v.grad.clone() for k, v in model.named_parameters()}
        opt.step()
        out[backend] = (float(loss["total_loss"].detach()), grads, {k: v.detach().clone() for k, v in model.named_parameters()},
                        o["mask"].clone())
    if not torch.equal(out["hip"][3], out["torch"][3]):
        # a logit pair within fp32 rounding of a tie flipped the segmentation of a point: the object points then
        # differ and the runs are no longer comparable term by term (dynamic B=32, and B=3 where the STOCK fp32 run is
        # the one that leaves the float64 mask: one point with a logit gap of 8e-5; found with a one-off script, since deleted)
        assert float((out["hip"][3] != out["torch"][3]).float().mean()) < (1e-4 if B >= 32 else 5e-4)
        assert abs(out["hip"][0] - out["torch"][0]) <= 2e-2 * abs(out["torch"][0])
        return
    assert abs(out["hip"][0] - out["torch"][0]) <= 1e-4 * abs(out["torch"][0])
    scale = max(float(g.norm()) for g in out["torch"][1].values())
    for k, gt in out["torch"][1].items():
        gh = out["hip"][1][k]                                # conv biases in front of a BN: exactly 0 vs autograd's noise
        # (B = 3: a BatchNorm over three items is ill-conditioned — gradients ~1e3, fp32 rounding of BOTH runs with them)
        assert float((gh - gt).norm()) <= 2e-2 * float(gt.norm()) + (1e-6 if B > 3 else 1e-5) * scale, k
    for k, pt in out["torch"][2].items():
        assert float((out["hip"][2][k] - pt).abs().max()) <= 2.5e-3, k        # Adam moves every weight by <= lr (+ decay)


def test_train_mode_with_the_device_sampler_needs_no_host_round_trip():
    """model.sampler == "device" (the default) also picks the object points of the TRAIN-mode forward on the GPU:
    same mask, every sampled point is a segmented point of its crop, gradients flow, and the step is deterministic"""
    losses = importlib.import_module("3dal_pytorch_amd.losses")
    B, N = 4, 1024
    p, i, g = synth.static_crops(B, N, seed=26)
    args = (torch.from_numpy(p).cuda().transpose(2, 1), torch.from_numpy(i).cuda(), torch.from_numpy(g).cuda())
    runs = []
    for _ in range(2):
        model = build_model("static_one", synth.state_dict("static_one", seed=26)).train()
        model.ins_seg.dropout.p = 0.0
        assert model.sampler == "device"
        o = model(*args)
        loss = losses.FrustumPointNetLossOneBoxEst()(o, *_labels_for(B, N, 27, "cuda"))["total_loss"]
        loss.backward()
        runs.append((float(loss.detach()), model.box_est.conv1.weight.grad.clone(), o["mask"].clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][1].abs().max()) > 0 and bool(torch.isfinite(runs[0][1]).all())
    # consecutive steps of ONE model draw different subsets (as np.random would): same logits, other box inputs
    again = model(*args)
    assert torch.equal(again["logits"], o["logits"]) and not torch.equal(again["center"], o["center"])
    ref = build_model("static_one", synth.state_dict("static_one", seed=26)).train()
    ref.sampler, ref.ins_seg.dropout.p = "numpy", 0.0
    np.random.seed(1)
    assert torch.equal(ref(*args)["mask"], runs[0][2])


# ------------------------------------------------------------------ round 2: fused pooling, Dropout kernel, FC tails
@pytest.mark.parametrize("c_in,c_out,seg,extra", [(64, 512, 4096, 0), (128, 128, 0, 0), (512, 256, 0, 0), (64, 64, 0, 0),
                                                  (192, 64, 0, 0), (256, 128, 0, 0), (64, 512, 0, 37), (512, 256, 0, 1001),
                                                  (128, 128, 0, 4095)])
def test_persistent_linear_kernels_match_float64_and_the_one_unit_kernels_bitwise(c_in, c_out, seg, extra):
    """the software-pipelined persistent kernels (tr_linear_pers_kernel: K = 64 and K = 128 as straight-line code, K >= 128
    generic, both tile shapes) at the step's size, 64 x 4096 rows: against float64, and against the one-unit-per-wave
    kernels, which an accumulating call into a zeroed buffer still takes (0 + x is exact) — the same FMA chain per
    element, so the same bits; `extra`: unit counts that are no multiple of the wave count"""
    M = 64 * 4096 + 64 * extra                                          # extra: waves with one unit more than others
    gen = torch.Generator(device="cuda").manual_seed(c_in * 7 + c_out)
    a = torch.randn((M, c_in), device="cuda", generator=gen)
    W = torch.randn((c_out, c_in), device="cuda", generator=gen) / c_in ** 0.5
    sc = torch.rand(c_in, device="cuda", generator=gen) + 0.5
    sh = torch.randn(c_in, device="cuda", generator=gen) * 0.3
    n_seg = M // seg if seg else 1
    b = torch.randn((n_seg, c_out) if seg else (c_out,), device="cuda", generator=gen)
    kw = dict(act=(sc, sh, True), bias=b)
    if seg:
        kw["seg"] = seg
    z = train._linear(a, W, c_in, c_in, c_out, **kw)
    ref = torch.zeros_like(z)
    train._linear(a, W, c_in, c_in, c_out, out=ref, accumulate=True, **kw)
    assert torch.equal(z, ref)
    rows = torch.arange(0, M, 997, device="cuda")                       # a float64 check on a sample of the rows
    act64 = torch.relu(a[rows].double() * sc.double() + sh.double())
    bias64 = b.double()[rows // seg] if seg else b.double()
    assert _close(z[rows], act64 @ W.double().t() + bias64)
    dz = torch.randn((M, c_out), device="cuda", generator=gen)          # dgrad: the transposed weight, no bias
    da = train._linear(dz, W, c_in, c_out, c_in, transpose=True)
    ref = torch.zeros_like(da)
    train._linear(dz, W, c_in, c_out, c_in, transpose=True, out=ref, accumulate=True)
    assert torch.equal(da, ref)
    assert _close(da[rows], dz[rows].double() @ W.double())


@pytest.mark.parametrize("B,N,c_in,c_out", [(4, 256, 128, 1024), (3, 96, 64, 128), (2, 4096, 128, 1024),
                                            (16, 4096, 128, 1024), (32, 2048, 64, 256),
                                            # the kernel with resident activations (c_in 128, >= 1024 groups of 64 points):
                                            # two and four groups per wave, waves that cross a segment, few channels
                                            (20, 3840, 128, 1024), (400, 192, 128, 256), (64, 4096, 128, 1024),
                                            (18, 4096, 128, 128),
                                            # the generic-K persistent kernel (too few groups for the resident one, 2,048
                                            # units): K = 128, and K = 256 with the K loop's middle rounds
                                            (8, 2048, 128, 1024), (64, 512, 256, 512)])
def test_fused_linear_pool_equals_linear_then_segmax_bitwise(B, N, c_in, c_out):
    """dal3_tr_linear_pool (conv -> BN -> ReLU -> max over each crop's points without writing the layer's output) must
    give the bits of dal3_tr_linear + dal3_tr_segmax: same g, same arg-max (first maximum), ties included"""
    M = B * N
    gen = torch.Generator(device="cuda").manual_seed(B * 1000 + N)
    a = torch.randn((M, c_in), device="cuda", generator=gen)
    a[: 2 * N: 2] = a[1: 2 * N: 2]                                   # exact ties between neighbouring points
    W = torch.randn((c_out, c_in), device="cuda", generator=gen) / c_in ** 0.5
    b = torch.randn(c_out, device="cuda", generator=gen)
    sc_in = torch.rand(c_in, device="cuda", generator=gen) + 0.5
    sh_in = torch.randn(c_in, device="cuda", generator=gen) * 0.3

    class BN:                                                        # just the affine the kernels read
        scale = torch.rand(c_out, device="cuda", generator=gen) - 0.3    # some negative scales too
        shift = torch.randn(c_out, device="cuda", generator=gen) * 0.2
    BN.M = M
    act = (sc_in, sh_in, True)
    z = train._linear(a, W, c_in, c_in, c_out, act=act, bias=b)
    g0, arg0 = train._segmax(z, BN, N)
    g1, arg1 = train._linear_pool(a, act, W, b, BN, N)
    assert torch.equal(g0, g1)
    assert torch.equal(arg0, arg1)
    assert int((arg0 % 2 == 0).sum()) > 0                            # (ties resolved towards the first point)
    y = torch.relu(z * BN.scale + BN.shift).view(B, N, c_out)
    assert torch.allclose(y.max(1).values, g1, rtol=0, atol=1e-6)


def test_dropout_kernel_statistics_key_and_backward():
    M, C, p = 4096, 128, 0.5
    x = torch.randn((M, C), device="cuda")
    sc, sh = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    key = (1234567, step, p)
    y1 = train._act_dropout(x, (sc, sh, True), key)
    y2 = train._act_dropout(x, (sc, sh, True), key)
    assert torch.equal(y1, y2)                                       # the multiplier is a function of the key
    a = torch.relu(x * sc + sh)
    kept = (y1 != 0) | (a == 0)
    assert torch.allclose(y1[kept], a[kept] * 2.0, rtol=1e-6, atol=1e-6)      # (fma in the kernel, mul + add in torch)
    frac = float(((y1 != 0) & (a != 0)).sum()) / float((a != 0).sum())
    assert abs(frac - 0.5) < 0.01                                    # Bernoulli(1 - p) over 260k draws
    cols = ((y1 != 0) & (a != 0)).float().mean(0) / (a != 0).float().mean(0)
    assert float(cols.min()) > 0.4 and float(cols.max()) < 0.6       # no channel pattern
    # the backward pass re-creates the same multiplier from the key: d/dx of (y * w).sum() through the dropout
    w = torch.randn((M, C), device="cuda")
    back = train._act_dropout(w, None, key)
    mult = torch.where(kept & (a != 0), torch.full_like(a, 2.0), torch.zeros_like(a))
    sure = a > 1e-5                                                  # (an activation within rounding of 0 may be gated differently)
    assert torch.equal(back[sure], (w * mult)[sure])
    step.add_(1)                                                     # a new step: a new draw
    y3 = train._act_dropout(x, (sc, sh, True), key)
    assert not torch.equal(y3, y1)
    agree = float(((y3 != 0) == (y1 != 0))[a != 0].float().mean())
    assert 0.45 < agree < 0.55                                       # independent of the previous one
    # a caller-supplied multiplier (the parity tests' path) is applied as is
    forced = (torch.rand((M, C), device="cuda") > 0.3).float() * 1.25
    assert torch.allclose(train._act_dropout(x, (sc, sh, True), forced), a * forced, rtol=1e-6, atol=1e-6)
    # p = 0 keeps everything
    assert torch.allclose(train._act_dropout(x, (sc, sh, True), (5, None, 0.0)), a, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("kind,head_name,c_in,B", [("static_one", "box_est", 512, 64), ("dynamic", "point_emb", 512, 64),
                                                   ("dynamic", "box_emb", 512, 64), ("dynamic", "box_est", 384, 64),
                                                   ("static_one", "box_est", 512, 40), ("dynamic", "box_est", 384, 7),
                                                   ("static_one", "box_est", 512, 5), ("dynamic", "point_emb", 512, 256),
                                                   ("static_one", "box_est", 512, 300), ("dynamic", "box_est", 384, 289)])
def test_fc_tail_on_hip_kernels_matches_float64_autograd(kind, head_name, c_in, B):
    """the per-item Linear -> BatchNorm1d -> ReLU tails (rows = items) on the training kernels: output, input
    gradient, every parameter gradient and the running statistics against float64 autograd of `_PointHead.tail`.
    Up to dal3_tr_fc_max_rows() = 256 items: the rows-are-items kernels (csrc/dal3_train_fc.hip); more: the per-point kernels (B = 300, 289: no multiple of 32 — padded rows, statistics over the real ones)"""
    model = build_model(kind, synth.state_dict(kind, seed=27)).train()
    head = getattr(model, head_name)
    ref = copy.deepcopy(head).double()
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((B, c_in), device="cuda", generator=gen).abs()           # pooled features are >= 0
    x.requires_grad_(True)
    xd = x.detach().double().requires_grad_(True)
    want = ref.tail(xd)
    w = torch.randn(want.shape, device="cuda", generator=gen)
    (want * w.double()).sum().backward()
    assert train.fc_tail_supported(x)
    got = train.fc_tail_train_forward(head, x)
    (got * w).sum().backward()
    assert got.shape == want.shape and _close(got.detach(), want.detach())
    assert _close(x.grad, xd.grad)
    names = [n for n, _ in head.named_parameters() if n.startswith("fc")]
    gmax = max(float(dict(ref.named_parameters())[n].grad.abs().max()) for n in names)
    for n in names:
        p, q = dict(head.named_parameters())[n], dict(ref.named_parameters())[n]
        assert p.grad is not None and _close(p.grad, q.grad, gmax), n
    for (n, b1), (_, b2) in zip(head.named_buffers(), ref.named_buffers()):
        if n.startswith("fcbn") and not n.endswith("num_batches_tracked"):
            assert _close(b1, b2), n
        if n.startswith("fcbn") and n.endswith("num_batches_tracked"):
            assert int(b1) == int(b2)
    assert not train.fc_tail_supported(x.cpu())


@pytest.mark.parametrize("B,N,int_labels", [(4, 1024, False), (3, 1000, True), (64, 4096, False)])
def test_fused_mask_loss_matches_float64_log_softmax_nll(B, N, int_labels):
    """losses._mask_loss on CUDA tensors is dal3_tr_seg_ce: the value and the gradient against the reference's
    F.nll_loss(F.log_softmax(...)) in float64, float and int64 labels, a point count that is no multiple of the
    kernel's block, logits up to +-60 (no overflow), and bitwise repeatability"""
    losses = importlib.import_module("3dal_pytorch_amd.losses")
    gen = torch.Generator(device="cuda").manual_seed(B * N)
    logits = (torch.randn((B, N, 2), device="cuda", generator=gen) * 4.0)
    logits[0, :8] = torch.tensor([[60.0, -60.0], [-60.0, 60.0], [0.0, 0.0], [1e-3, -1e-3]] * 2, device="cuda")
    lab = (torch.rand((B, N), device="cuda", generator=gen) > 0.6)
    labels = lab.long() if int_labels else lab.float()
    x = logits.clone().requires_grad_(True)
    got = losses._mask_loss(x, labels)
    (got * 3.0).backward()
    x64 = logits.double().requires_grad_(True)
    want = F.nll_loss(F.log_softmax(x64.view(-1, 2), dim=1), lab.view(-1).long())
    (want * 3.0).backward()
    assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want))
    assert float((x.grad.double() - x64.grad).abs().max()) <= 1e-6 * float(x64.grad.abs().max())
    y = logits.clone().requires_grad_(True)
    again = losses._mask_loss(y, labels)
    (again * 3.0).backward()
    assert float(again) == float(got) and torch.equal(y.grad, x.grad)


@pytest.mark.parametrize("M,C", [(4128, 96), (300, 64), (64 * 4096, 128)])
def test_fused_statistics_entries_equal_the_two_step_ones_bitwise(M, C):
    """dal3_tr_bn_stats = dal3_tr_colred(mode 0) + dal3_tr_bn_finalize and dal3_tr_bnbwd_sums = dal3_tr_colred(mode 1) +
    dal3_tr_bnbwd_coef: the second stage of the reduction carries the epilogue, the numbers are the same bits"""
    lib = hip.lib()
    gen = torch.Generator(device="cuda").manual_seed(M + C)
    z = torch.randn((M, C), device="cuda", generator=gen) * 2.0 + 0.5
    da = torch.randn((M, C), device="cuda", generator=gen)
    gamma = torch.rand(C, device="cuda", generator=gen) + 0.5
    beta = torch.randn(C, device="cuda", generator=gen) * 0.3
    rm1, rv1 = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    rm2, rv2 = rm1.clone(), rv1.clone()
    bn = train._BN(z, gamma, beta, rm1, rv1)                                   # fused
    sums = train._colred(z, 0)
    st = torch.empty((4, C), device="cuda")
    hip.check(lib.dal3_tr_bn_finalize(hip.ptr(sums), C, M, hip.ptr(gamma), hip.ptr(beta), hip.ptr(rm2), hip.ptr(rv2), 0.1,
                                      1e-5, hip.ptr(st[0]), hip.ptr(st[1]), hip.ptr(st[2]), hip.ptr(st[3]), hip.stream()))
    for a, b in ((bn.mu, st[0]), (bn.rstd, st[1]), (bn.scale, st[2]), (bn.shift, st[3]), (rm1, rm2), (rv1, rv2)):
        assert torch.equal(a, b)
    dz, dgam, dbet = bn.backward(z, da=da)                                      # fused sums + coefficients
    sums1 = train._colred(z, 1, da=da, bn=(bn.scale, bn.shift, bn.mu, bn.rstd))
    co = torch.empty((5, C), device="cuda")
    hip.check(lib.dal3_tr_bnbwd_coef(hip.ptr(sums1), C, M, hip.ptr(bn.gamma), hip.ptr(bn.rstd), hip.ptr(co[0]), hip.ptr(co[1]),
                                     hip.ptr(co[2]), hip.ptr(co[3]), hip.ptr(co[4]), hip.stream()))
    assert torch.equal(dgam, co[0]) and torch.equal(dbet, co[1])


@pytest.mark.parametrize("tag", ["one", "two", "dyn"])
def test_criteria_on_the_gpu_match_the_stock_float64_formulation(tag):
    """The three loss modules on CUDA tensors (mask term: dal3_tr_seg_ce, box terms: dal3_tr_box_loss, one launch per
    estimate) against the same modules on CPU float64 tensors (stock torch ops, pinned to the reference's criteria by
    tests/test_host_dropin_train.py): every entry of the loss dict and the gradient of the total w.r.t. every output that
    takes part, two values of w_box, a batch that needs more than one pass of the kernel's 256 threads."""
    losses = importlib.import_module("3dal_pytorch_amd.losses")
    crit = {"one": losses.FrustumPointNetLossOneBoxEst, "two": losses.FrustumPointNetLossTwoBoxEst,
            "dyn": losses.DynamicModelLoss}[tag]()
    for B, w_box in ((8, 1.0), (300, 0.3)):
        out_np, labels_np = synth.loss_case(50 + B, batch=B, n_pts=64, two_stage=(tag == "two"))
        labels_np = list(labels_np)
        labels_np[1] = labels_np[1] + np.float32(3.0) * (np.arange(B)[:, None] % 2).astype(np.float32)   # some centres beyond delta
        grad_keys = [k for k, v in out_np.items() if v.dtype == np.float32 and not k.endswith("label_two")]
        res = {}
        for dev, dt in (("cuda", torch.float32), ("cpu", torch.float64)):
            o = {k: (torch.from_numpy(v).to(dev).to(dt) if v.dtype == np.float32 else torch.from_numpy(v).to(dev))
                 for k, v in out_np.items()}
            for k in grad_keys:
                o[k].requires_grad_(True)
            lab = [torch.from_numpy(a).to(dev).to(dt) if a.dtype == np.float32 else torch.from_numpy(a).to(dev) for a in labels_np]
            ls = crit(o, *lab, w_box=w_box)
            ls["total_loss"].backward()
            res[dev] = ({k: float(v.detach()) for k, v in ls.items()},
                        {k: o[k].grad.detach().cpu().double() for k in grad_keys if o[k].grad is not None})
        assert set(res["cuda"][0]) == set(res["cpu"][0]) and set(res["cuda"][1]) == set(res["cpu"][1])
        for k, v in res["cpu"][0].items():
            assert abs(res["cuda"][0][k] - v) <= 2e-6 * max(abs(v), 1e-3), (k, res["cuda"][0][k], v)
        for k, g in res["cpu"][1].items():
            assert float((res["cuda"][1][k] - g).abs().max()) <= 2e-6 * max(float(g.abs().max()), 1e-6), k


def test_an_out_of_range_class_label_poisons_losses_and_gradients():
    """F.nll_loss of the stock criterion raises on a label outside its classes; dal3_tr_box_loss answers with NaN
    in every loss term AND in that item's rows of all five gradients (a step taken without looking at the loss then
    poisons the parameters instead of training on a rejected batch); the other items' rows stay finite"""
    losses = importlib.import_module("3dal_pytorch_amd.losses")
    B = 6
    out_np, labels_np = synth.loss_case(61, batch=B, n_pts=64, two_stage=False)
    o = {k: torch.from_numpy(v).cuda().requires_grad_(v.dtype == np.float32) for k, v in out_np.items()}
    lab = [torch.from_numpy(a).cuda() for a in labels_np]
    lab[2] = lab[2].clone()
    lab[2][3] = -1                                           # heading class label of item 3: an ignore value
    ls = losses.FrustumPointNetLossOneBoxEst()(o, *lab)
    assert all(bool(torch.isnan(ls[k])) for k in ("total_loss", "center_loss", "heading_class_loss", "size_class_loss"))
    ls["total_loss"].backward()
    for k in ("center", "heading_scores", "heading_residuals_normalized", "size_scores", "size_residuals_normalized"):
        g = o[k].grad.reshape(B, -1)
        assert bool(torch.isnan(g[3]).all()), k


@pytest.mark.parametrize("B,C,K,N", [(4, 1024, 128, 4096), (3, 512, 256, 512), (5, 512, 128, 101), (2, 1024, 128, 5120)])
def test_pooled_layer_sparse_terms_match_stock_index_put_and_gather(B, C, K, N):
    """dal3_tr_pool_sparse against index_put_(accumulate=True) / gather-multiply-sum in float64, with many channels
    sharing a pooled point (the kernel adds them in channel order: bitwise repeatable) — short lists (sorted) and
    lists of hundreds of channels (placed by rank) in one call"""
    gen = torch.Generator(device="cuda").manual_seed(B * C + N)
    arg = torch.randint(0, max(N // 8, 1), (B, C), device="cuda", generator=gen, dtype=torch.int32)     # heavy sharing
    arg[:, ::7] = torch.randint(0, N, (B, (C + 6) // 7), device="cuda", generator=gen, dtype=torch.int32)
    arg[0] = 0                                             # a zero-padded item: every channel pooled at its first point
    if B > 1:
        arg[1] = torch.randint(0, 3, (C,), device="cuda", generator=gen, dtype=torch.int32) * (N // 3)   # three long lists
    kd = torch.randn((B, C), device="cuda", generator=gen)
    W = torch.randn((C, K), device="cuda", generator=gen)
    a = torch.randn((B * N, K), device="cuda", generator=gen)
    da0 = torch.randn((B * N, K), device="cuda", generator=gen)
    rows = (arg.long() + torch.arange(B, device="cuda")[:, None] * N).reshape(-1)
    want_da = da0.double().index_put((rows,), (kd.double()[:, :, None] * W.double()[None]).reshape(-1, K), accumulate=True)
    want_dw = (kd.double()[:, :, None] * a.double()[rows].reshape(B, C, K)).sum(0)
    outs = []
    for _ in range(2):
        da, dws = da0.clone(), torch.empty((C, K), device="cuda")
        hip.check(hip.lib().dal3_tr_pool_sparse(hip.ptr(arg), hip.ptr(kd), hip.ptr(W), K, hip.ptr(a), K, B, C, K, N, hip.ptr(da), K,
                                                hip.ptr(dws), hip.stream()))
        outs.append((da, dws))
    assert _close(outs[0][0], want_da) and _close(outs[0][1], want_dw)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert hip.lib().dal3_tr_pool_sparse(hip.ptr(arg), hip.ptr(kd), hip.ptr(W), K, hip.ptr(a), K, B, C, K, 9000, hip.ptr(da), K,
                                         hip.ptr(dws), hip.stream()) != 0          # 2 N + C + 1 > 16384: refused


@pytest.mark.parametrize("B,C", [(64, 1024), (5, 96), (1, 32)])
def test_pooled_layer_coefficients_match_the_float64_formulas(B, C):
    """dal3_tr_pool_coef (the conv5 shortcut's per-channel algebra in one launch) against the stock float64 expressions it
    replaced in train.py's _pooled_layer_backward"""
    gen = torch.Generator(device="cuda").manual_seed(B * 31 + C)
    dg = torch.randn((B, C), device="cuda", generator=gen)
    g = torch.relu(torch.randn((B, C), device="cuda", generator=gen))        # about half of the gates closed
    zarg = torch.randn((B, C), device="cuda", generator=gen) * 2 + 0.5
    mu = torch.randn(C, device="cuda", generator=gen)
    rstd = torch.rand(C, device="cuda", generator=gen) + 0.5
    gamma = torch.randn(C, device="cuda", generator=gen)
    M = B * 4096
    coef = torch.empty((4, C), dtype=torch.float64, device="cuda")
    kd = torch.empty((B, C), device="cuda")
    hip.check(hip.lib().dal3_tr_pool_coef(hip.ptr(dg), hip.ptr(g), hip.ptr(zarg), hip.ptr(mu), hip.ptr(rstd), hip.ptr(gamma), B, C,
                                          M, hip.ptr(coef), hip.ptr(kd), hip.stream()))
    D = (dg * (g > 0)).double()
    xhat = (zarg.double() - mu.double()) * rstd.double()
    dbeta, dgamma = D.sum(0), (D * xhat).sum(0)
    k1 = gamma.double() * rstd.double()
    k2, k3 = dbeta / M, dgamma / M
    want = torch.stack([dbeta, dgamma, -k1 * k2 + k1 * k3 * rstd.double() * mu.double(), -k1 * k3 * rstd.double()])
    assert float((coef - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert torch.equal(kd, (k1 * D).float())
    assert hip.lib().dal3_tr_pool_coef(hip.ptr(dg), hip.ptr(g), hip.ptr(zarg), hip.ptr(mu), hip.ptr(rstd), hip.ptr(gamma), 0, C, M,
                                       hip.ptr(coef), hip.ptr(kd), hip.stream()) != 0


@pytest.mark.parametrize("C,K,M", [(1024, 128, 64 * 4096), (96, 64, 1000), (512, 256, 32768)])
def test_pooled_layer_float64_algebra_kernels_match_the_stock_expressions(C, K, M):
    """dal3_tr_pool_moments / _gv / _dw against the float64 torch expressions they replaced (train.py
    _moments_through, _pooled_layer_backward): the same quantities to ~1e-12 in float64, to fp32 rounding where the
    output is fp32"""
    gen = torch.Generator(device="cuda").manual_seed(C + K)
    W = torch.randn((C, K), device="cuda", generator=gen) / K ** 0.5
    b = torch.randn(C, device="cuda", generator=gen)
    x = torch.randn((4096, K), device="cuda", generator=gen).double() * 0.7 + 0.3
    m1 = x.sum(0) * (M / 4096)
    xc = x - x.mean(0)
    Sc = ((xc.t() @ xc) * (M / 4096)).float().contiguous()
    lib = hip.lib()
    sums = torch.empty(2 * C, dtype=torch.float64, device="cuda")
    hip.check(lib.dal3_tr_pool_moments(hip.ptr(W), K, hip.ptr(b), hip.ptr(m1), hip.ptr(Sc), M, C, K, hip.ptr(sums), hip.stream()))
    W64 = W.double()
    mu = W64 @ (m1 / M) + b.double()
    var = ((W64 @ (Sc.double() / M)) * W64).sum(1).clamp_(min=0.0)
    want = torch.cat([mu * M, (var + mu * mu) * M])
    assert float((sums - want).abs().max()) <= 1e-11 * float(want.abs().max())
    coef = torch.randn((4, C), device="cuda", generator=gen).double()
    A, Bc = coef[2], coef[3]
    G = torch.empty((K, K), device="cuda")
    v = torch.empty(K, device="cuda")
    need = lib.dal3_tr_pool_gv_workspace_bytes(K)
    gws = torch.empty(need, dtype=torch.uint8, device="cuda")
    hip.check(lib.dal3_tr_pool_gv(hip.ptr(coef), hip.ptr(W), K, hip.ptr(b), C, K, hip.ptr(G), hip.ptr(v), hip.ptr(gws), need,
                                  hip.stream()))
    assert torch.equal(G, (W64.t() @ (Bc[:, None] * W64)).float()) or _close(G, W64.t() @ (Bc[:, None] * W64))
    assert _close(v, (A + Bc * b.double()) @ W64)
    dWs = torch.randn((C, K), device="cuda", generator=gen)
    for centred in (1, 0):
        S = Sc if centred else (Sc.double() + m1[:, None] * m1[None] / M).float().contiguous()
        S64 = S.double() + (m1[:, None] * m1[None] / M if centred else 0.0)
        dW = torch.empty((C, K), device="cuda")
        hip.check(lib.dal3_tr_pool_dw(hip.ptr(coef), hip.ptr(W), K, hip.ptr(b), hip.ptr(S), hip.ptr(m1), M, centred, hip.ptr(dWs),
                                      C, K, hip.ptr(dW), hip.stream()))
        want = A[:, None] * m1[None] + Bc[:, None] * (W64 @ S64 + b.double()[:, None] * m1[None]) + dWs.double()
        assert _close(dW, want)
    assert lib.dal3_tr_pool_gv(hip.ptr(coef), hip.ptr(W), K, hip.ptr(b), C, 96, hip.ptr(G), hip.ptr(v), hip.ptr(gws), need,
                               hip.stream()) != 0
    assert lib.dal3_tr_pool_gv(hip.ptr(coef), hip.ptr(W), K, hip.ptr(b), C, K, hip.ptr(G), hip.ptr(v), hip.ptr(gws), 16,
                               hip.stream()) != 0


@pytest.mark.parametrize("B,N,C", [(8, 4096, 512), (3, 256, 64), (2, 128, 128)])
def test_bn_backward_with_segment_sums_equals_the_two_pass_route(B, N, C):
    """dal3_tr_bnbwd_apply_segsum: the same dz bits as dal3_tr_bnbwd_apply, and per-crop column sums equal to
    dal3_tr_segsum's over that dz up to the order of the float64 additions"""
    M = B * N
    gen = torch.Generator(device="cuda").manual_seed(B * N + C)
    z = torch.randn((M, C), device="cuda", generator=gen)
    da = torch.randn((M, C), device="cuda", generator=gen)
    gamma, beta = torch.rand(C, device="cuda", generator=gen) + 0.5, torch.randn(C, device="cuda", generator=gen) * 0.1
    bn = train._BN(z, gamma, beta, None, None)
    dz0, dgam0, dbet0 = bn.backward(z, da=da)
    dz1, dgam1, dbet1, sums = bn.backward(z, da=da, sum_seg=N)
    assert sums is not None and sums.shape == (B, C)
    assert torch.equal(dz0, dz1) and torch.equal(dgam0, dgam1) and torch.equal(dbet0, dbet1)
    ref = train._segsum(dz0, N, B)
    want = dz0.double().view(B, N, C).sum(1)
    scale = float(dz0.abs().sum(0).max())                                 # (the sums cancel: compare on the scale of what is added)
    assert float((sums.double() - want).abs().max()) <= 1e-6 * scale
    assert float((sums - ref).abs().max()) <= 1e-6 * scale
    assert bn.backward(z[: M - 32], da=da[: M - 32], sum_seg=N)[3] is None    # ragged: left to the separate pass


@pytest.mark.parametrize("kind", ["static_one", "dynamic"])
def test_a_training_step_leaves_no_buffers_behind_without_the_garbage_collector(kind):
    """a step's activations must be released by its own backward. Two ways they were not: the point stack kept its OUTPUT
    as a plain ctx attribute (a reference cycle g -> grad_fn -> ctx -> g that only Python's cyclic collector breaks:
    4-9 GB of dead steps at DynamicModel's batch, 13 GB peak), and the ctx attributes outlived backward for as long as
    the caller held the loss. With the collector off and the previous step's loss still referenced, the allocation after
    every step must be the same."""
    import gc
    losses = importlib.import_module("3dal_pytorch_amd.losses")
    B = 8
    model = build_model(kind, synth.state_dict(kind, seed=24)).train()
    model.train_backend, model.sampler = "hip", "device"
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    if kind == "dynamic":
        p, bx, _, g = synth.dynamic_items(B, n_per_frame=256, seed=24)
        args = (torch.from_numpy(p).cuda().transpose(2, 1), torch.from_numpy(bx).cuda().transpose(2, 1), torch.from_numpy(g).cuda())
        crit, n = losses.DynamicModelLoss(), p.shape[1]
    else:
        p, i, g = synth.static_crops(B, 1024, seed=24)
        args = (torch.from_numpy(p).cuda().transpose(2, 1), torch.from_numpy(i).cuda(), torch.from_numpy(g).cuda())
        crit, n = losses.FrustumPointNetLossOneBoxEst(), 1024
    labels = _labels_for(B, n, 25, "cuda")
    gc.collect()
    gc.disable()
    try:
        seen, loss = [], None
        for _ in range(6):
            o = model(*args)
            loss = crit(o, *labels)["total_loss"]            # (the previous step's loss dies here, after this forward)
            opt.zero_grad()
            loss.backward()
            opt.step()
            del o
            torch.cuda.synchronize()
            seen.append(torch.cuda.memory_allocated())
        assert max(seen[2:]) - min(seen[2:]) <= 1 << 20, seen    # (steps 0-1: Adam's state and the scratch buffer appear)
        with pytest.raises(RuntimeError, match="a second time"):
            loss.backward()
    finally:
        gc.enable()



@pytest.mark.parametrize("B,some_missing", [(64, False), (5, True), (300, False)])
def test_parse_output_to_tensors_in_one_launch_equals_the_slices(B, some_missing):
    """static_model._parse in train mode (dal3_parse_box_pred / _backward, tools/static_model.py:64-92): the seven tensors
    bit for bit what slicing and scaling box_pred gives, contiguous; the gradient of box_pred bit for bit autograd's, also
    when some of the seven take no part in the loss (NULL gradients)"""
    sm = importlib.import_module("3dal_pytorch_amd.static_model")
    gen = torch.Generator(device="cuda").manual_seed(B)
    bp = torch.randn((B, 39), device="cuda", generator=gen)
    x = bp.clone().requires_grad_(True)
    y = bp.clone().requires_grad_(True)
    got = sm._parse(x)
    mean = sm._mean_size(bp.device)
    srn = y[:, 30:39].reshape(B, 3, 3)
    want = (y[:, 0:3], y[:, 3:15], y[:, 15:27], y[:, 15:27] * (np.pi / sm.NUM_HEADING_BIN), y[:, 27:30], srn, srn * mean[None])
    w = [torch.randn(t.shape, device="cuda", generator=gen) for t in want]
    use = [0, 3, 6] if some_missing else range(7)
    for i in range(7):
        assert got[i].is_contiguous() and torch.equal(got[i].detach(), want[i].detach()), i
    sum((got[i] * w[i]).sum() for i in use).backward()
    sum((want[i] * w[i]).sum() for i in use).backward()
    assert torch.equal(x.grad, y.grad)
