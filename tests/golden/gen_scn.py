#!/usr/bin/env python3
"""Generate tests/golden/scn_keys.json from the REAL reference (jacky121298/3DAL_PyTorch): the state_dict keys and shapes
of its own `SpMiddleResNetFHD` (det3d/models/backbones/scn.py), for num_input_features 5 and 6.

Run only where the reference checkout exists (DAL3_REFERENCE, as tests/golden/gen_pillars.py reads it):
    python tests/golden/gen_scn.py

scn.py is loaded by path behind stub modules for what its import chain needs and this machine lacks: the registry,
det3d.models.utils.build_norm_layer (BN1d -> nn.BatchNorm1d with the cfg's eps and momentum), and `spconv`, which is
CUDA-only. The stub's SubMConv3d / SparseConv3d only DECLARE parameters of spconv 1.x's shapes (spconv/conv.py:
weight (*kernel_size, in_channels, out_channels), bias (out_channels)); SparseSequential names its children by position,
as spconv's does. Nothing is computed: the fixture holds names and shapes only."""
import importlib.util
import json
import os
import sys
import types

import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DAL3_REFERENCE", "/root/reference")


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    mod.__path__ = []
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    return mod


def import_reference():
    def triple(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3

    class _Conv(nn.Module):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                     indice_key=None, **kwargs):
            super().__init__()
            self.weight = nn.Parameter(torch.zeros(*triple(kernel_size), in_channels, out_channels))
            if bias:
                self.bias = nn.Parameter(torch.zeros(out_channels))
            else:
                self.register_parameter("bias", None)

    class SubMConv3d(_Conv):
        pass

    class SparseConv3d(_Conv):
        pass

    class SparseSequential(nn.Module):
        def __init__(self, *mods):
            super().__init__()
            for i, m in enumerate(mods):
                self.add_module(str(i), m)

    class Registry:
        @staticmethod
        def register_module(cls):
            return cls

    def build_norm_layer(cfg, num_features, postfix=""):
        cfg = dict(cfg)
        assert cfg.pop("type") == "BN1d"
        return "bn" + str(postfix), nn.BatchNorm1d(num_features, eps=cfg.get("eps", 1e-5), momentum=cfg.get("momentum", 0.1))

    _stub("spconv", SparseModule=nn.Module, SparseSequential=SparseSequential, SubMConv3d=SubMConv3d, SparseConv3d=SparseConv3d,
          SparseConvTensor=object)
    _stub("det3d")
    _stub("det3d.models")
    _stub("det3d.models.backbones")
    _stub("det3d.models.registry", BACKBONES=Registry)
    _stub("det3d.models.utils", build_norm_layer=build_norm_layer)
    spec = importlib.util.spec_from_file_location("det3d.models.backbones.scn", os.path.join(REF, "det3d/models/backbones/scn.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["det3d.models.backbones.scn"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    scn = import_reference()
    out = {}
    for c in (5, 6):
        m = scn.SpMiddleResNetFHD(num_input_features=c, ds_factor=8)
        out[str(c)] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "scn_keys.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print({c: len(v) for c, v in out.items()})


if __name__ == "__main__":
    main()
