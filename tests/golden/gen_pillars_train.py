#!/usr/bin/env python3
"""Generate tests/golden/pillars_train.npz from the REAL reference (jacky121298/3DAL_PyTorch): one training step of its own
`PillarFeatureNet` (det3d/models/readers/pillar_encoder.py, PFNLayer in train mode) on GOLDEN_ROWS pillars of the ragged
batch of tests/golden/pillars.npz, for the one- and the two-layer net with C = 5, momentum 0.01 and eps 1e-3.

Run only where the reference checkout exists (DAL3_REFERENCE, default /root/reference):
    python tests/golden/gen_pillars_train.py

The reference is imported as tests/golden/gen_pillars.py imports it (the same stub modules). Recorded, as data only, in
.float() and in .double(): the outputs, the gradients of linear.weight, norm.weight and norm.bias per layer under the
seeded cotangent pillars_train_ref.cotangent("golden", P), and running_mean / running_var after the step; and the rows
used. Asserted here: pillars_train_ref's truth (the project's composite() in .double() under autograd) and its NumPy
definition equal the reference's .double() run to 1e-11. The archive has fixed timestamps: a rerun reproduces it byte
for byte."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gen_pillars as G  # noqa: E402
import pillars_ref as R  # noqa: E402
import pillars_train_ref as T  # noqa: E402


def reference_step(mod, vox, num, co, cot, dtype):
    mod = copy.deepcopy(mod).to(dtype).train()
    out = mod(torch.from_numpy(vox).to(dtype), torch.from_numpy(num), torch.from_numpy(co)).reshape(vox.shape[0], -1)
    out.backward(torch.from_numpy(cot).to(dtype))
    L = mod.pfn_layers
    return {"out": out.detach().numpy(), "dW": [l.linear.weight.grad.numpy() for l in L],
            "dgamma": [l.norm.weight.grad.numpy() for l in L], "dbeta": [l.norm.bias.grad.numpy() for l in L],
            "running_mean": [l.norm.running_mean.numpy() for l in L], "running_var": [l.norm.running_var.numpy() for l in L]}


def main():
    torch.set_num_threads(1)
    _, pil, _ = G.import_reference()
    P = R.PILLAR
    vox, num, co, cot, rows = T.golden_inputs()
    out = {"rows": rows.astype(np.int32)}
    for n_layers in (1, 2):
        sd = R.reader_weights(n_layers, P["C"])
        mod = pil.PillarFeatureNet(num_input_features=P["C"], num_filters=(64,) * n_layers, voxel_size=P["voxel_size"],
                                   pc_range=P["pc_range"], norm_cfg=dict(type="BN1d", eps=T.EPS, momentum=T.MOMENTUM))
        mod.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
        f32 = T.flat(reference_step(mod, vox, num, co, cot, torch.float32))
        f64 = T.flat(reference_step(mod, vox, num, co, cot, torch.float64))
        mine = T.flat(T.composite_run(T.module(n_layers, P["C"]), vox, num, co, cot, torch.float64))
        manual = T.flat(T.manual(sd, vox, num, co, cot))
        for row, want in f64.items():
            for got in (mine[row], manual[row]):
                assert np.allclose(got, want, rtol=1e-11, atol=1e-11 * np.abs(want).max()), (n_layers, row, np.abs(got - want).max())
            out[f"l{n_layers}/{row}/f32"], out[f"l{n_layers}/{row}/f64"] = f32[row].astype(np.float32), want
        gate, gap = T.margins(sd, vox, num, co)
        print(f"{n_layers} layer(s): {rows.size} pillars, margins gate {gate:.2e} gap {gap:.2e}, fp32 own error of out "
              f"{R.judge(f32['out'], f64['out'])}")
    path = os.path.join(HERE, "pillars_train.npz")
    G.save(path, {k.replace("/", "."): v for k, v in out.items()})
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
