#!/usr/bin/env python3
"""Generate tests/golden/rpn.npz from the REAL reference (jacky121298/3DAL_PyTorch): its own `RPN`
(det3d/models/necks/rpn.py) and `CenterHead` (det3d/models/bbox_heads/center_head.py) in the production configuration
(configs/waymo/pp/waymo_centerpoint_pp_two_pfn_stride1_3x.py), on the seeded canvases and weights of tests/rpn_ref.py.

Run only where the reference checkout exists (DAL3_REFERENCE, as tests/golden/gen_pillars.py reads it):
    python tests/golden/gen_rpn.py

The two files are loaded by path behind stub modules for what their import chain needs and this machine lacks:
torchvision, the registries, the loggers, the losses, and det3d.models.utils with `Sequential` (children named by
position, `add` appends) and `build_norm_layer` (BN -> nn.BatchNorm2d with the cfg's eps and momentum) restated.

What is recorded, per canvas: the head's five maps of the fp32 modules (head(neck(x)), 11 channels) and of the same
modules' .double() copies (the truth), whole; of the neck's 384-channel output every fourth channel (all three upsampled
maps are among them) in fp32 and as the truth, and the CRC-32 of the WHOLE fp32 output's bytes, so that a bit-for-bit
comparison of all of it costs four bytes. The truth is stored as the fp32 output plus a float32 difference (the
difference is ~1e-7 of the value, so its own rounding is ~1e-14 of it). The reference's key list with shapes for the
whole `PointPillars` model (reader, neck, bbox_head) is stored as strings. The restatement of tests/rpn_ref.py is
asserted here against the .double() outputs. Fixed timestamps: a rerun reproduces the archive byte for byte.
"""
import logging
import os
import sys
import zlib

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gen_pillars as G  # noqa: E402
import rpn_ref as R  # noqa: E402

CHANNEL_STEP = 4


def import_reference():
    _, pil, _ = G.import_reference()

    class Registry:
        @staticmethod
        def register_module(cls):
            return cls

    class Sequential(nn.Module):
        def __init__(self, *mods):
            super().__init__()
            for m in mods:
                self.add(m)

        def add(self, module, name=None):
            self.add_module(str(len(self._modules)) if name is None else name, module)

        def __getitem__(self, i):
            return list(self._modules.values())[i]

        def forward(self, x):
            for m in self._modules.values():
                x = m(x)
            return x

    def build_norm_layer(cfg, num_features, postfix=""):
        assert cfg["type"] == "BN"
        return "bn" + str(postfix), nn.BatchNorm2d(num_features, eps=cfg.get("eps", 1e-5), momentum=cfg.get("momentum", 0.1))

    def kaiming_init(m, **kw):
        nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)

    utils = sys.modules["det3d.models.utils"]
    utils.__dict__.update(Sequential=Sequential, build_norm_layer=build_norm_layer, Empty=nn.Identity, GroupNorm=nn.GroupNorm,
                          change_default_args=None)
    for name in ["torchvision", "det3d.torchie", "det3d.models.necks", "det3d.models.bbox_heads", "det3d.models.losses",
                 "det3d.core.utils"]:
        G._stub(name)
    G._stub("torchvision.models", resnet=None)
    G._stub("det3d.torchie.cnn", constant_init=None, kaiming_init=kaiming_init, xavier_init=None)
    G._stub("det3d.torchie.trainer", load_checkpoint=None)
    G._stub("det3d.models.builder")
    sys.modules["det3d.models"].builder = sys.modules["det3d.models.builder"]
    sys.modules["det3d.models.registry"].__dict__.update(NECKS=Registry, HEADS=Registry)
    sys.modules["det3d.core"].box_torch_ops = None
    G._stub("det3d.models.losses.centernet_loss", FastFocalLoss=nn.Identity, RegLoss=nn.Identity)
    G._stub("det3d.core.utils.circle_nms_jit", circle_nms=None)
    rpn = G._load_file("det3d.models.necks.rpn", "det3d/models/necks/rpn.py")
    head = G._load_file("det3d.models.bbox_heads.center_head", "det3d/models/bbox_heads/center_head.py")
    return pil, rpn, head


def load(mod, sd):
    mod.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    return mod.eval()


def main():
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    pil, rpn, head = import_reference()
    neck = load(rpn.RPN(**R.NECK, logger=logging.getLogger("RPN")), R.neck_weights())
    bbox = load(head.CenterHead(**R.HEAD), R.head_weights())
    reader = pil.PillarFeatureNet(num_input_features=5, num_filters=(64, 64), with_distance=False, voxel_size=(0.32, 0.32, 6.0),
                                  pc_range=(-74.88, -74.88, -2, 74.88, 74.88, 4.0))
    assert neck.blocks[0][2].eps == 1e-3 and bbox.shared_conv[1].eps == 1e-5 and bbox.tasks[0].hm[1].eps == 1e-5
    out = {}
    keys, shapes = [], []
    for prefix, mod in (("reader.", reader), ("neck.", neck), ("bbox_head.", bbox)):
        for k, v in mod.state_dict().items():
            keys.append(prefix + k)
            shapes.append(list(v.shape) + [0] * (4 - v.dim()))
    out["keys"] = np.asarray(keys)
    out["key_shapes"] = np.asarray(shapes, np.int64)
    out["key_ndim"] = np.asarray([sum(1 for d in s if d) for s in shapes], np.int64)
    neck64, bbox64 = None, None
    for tag, shape in R.CANVASES.items():
        x = R.canvas(tag, shape)
        out[f"{tag}_in_sum"] = np.asarray(float(x.astype(np.float64).sum()))
        out[f"{tag}_occupied"] = np.asarray(float((x != 0).any(1).mean()))
        n32 = neck(torch.from_numpy(x))
        h32 = bbox(n32)
        if neck64 is None:
            import copy
            neck64, bbox64 = copy.deepcopy(neck).double(), copy.deepcopy(bbox).double()
        n64 = neck64(torch.from_numpy(x).double())
        h64 = bbox64(n64)
        n32, n64 = n32.numpy(), n64.numpy()
        h32c, h64c = R.head_cat([{k: v.numpy() for k, v in d.items()} for d in h32]), R.head_cat([{k: v.numpy() for k, v in d.items()} for d in h64])
        assert list(h32[0]) == list(R.HEAD_ORDER)
        mine_n = R.neck_f64(R.neck_weights(), x)
        mine_h = R.head_cat(R.head_f64(R.head_weights(), mine_n))
        for name, mine, want in (("neck", mine_n, n64), ("head", mine_h, h64c)):
            err = np.abs(mine - want).max() / np.abs(want).max()
            assert err < 1e-12, (tag, name, err)
        print(f"{tag} {shape}: occupied {float(out[f'{tag}_occupied']):.2f}, neck rms {np.sqrt((n64 ** 2).mean()):.3f} "
              f"fp32 own error {R.judge(n32, n64)}; head rms {np.sqrt((h64c ** 2).mean()):.3f} own error {R.judge(h32c, h64c)}")
        out[f"{tag}_neck_crc"] = np.asarray(zlib.crc32(np.ascontiguousarray(n32).tobytes()), np.int64)
        sub32, sub64 = n32[:, ::CHANNEL_STEP], n64[:, ::CHANNEL_STEP]
        out[f"{tag}_neck_f32"], out[f"{tag}_neck_diff"] = sub32, (sub64 - sub32.astype(np.float64)).astype(np.float32)
        out[f"{tag}_head_f32"], out[f"{tag}_head_diff"] = h32c, (h64c - h32c.astype(np.float64)).astype(np.float32)
        for name, f32, f64 in (("neck", sub32, sub64), ("head", h32c, h64c)):
            back = f32.astype(np.float64) + out[f"{tag}_{name}_diff"].astype(np.float64)
            assert np.abs(back - f64).max() <= 1e-13 * np.abs(f64).max()
    path = os.path.join(HERE, "rpn.npz")
    G.save(path, out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
