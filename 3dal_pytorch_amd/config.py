"""The reference's configuration door for the detection run: `Config.fromfile` for its Python config files (det3d/torchie/
utils/config.py, written here from scratch: `addict` is not required), `build_detector` for a config's `model` dict
(det3d/models/builder.py through detector.PointPillars / detector.VoxelNet / two_stage.TwoStageDetector) and
`load_checkpoint` (det3d/torchie/trainer/checkpoint.py:42-172) for files only.

The config files import `det3d.utils.config_tool.get_downsample_factor`; the loader provides that one function under that
module path while the file runs and leaves `sys.modules` and `sys.path` as it found them.
"""
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch


class ConfigDict(dict):
    """a dict whose items are attributes as well; dicts inside (also inside lists and tuples) become ConfigDicts. A missing
    key raises KeyError as an item and AttributeError as an attribute."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        for k, v in dict(*args, **kwargs).items():
            self[k] = v

    @classmethod
    def _wrap(cls, v):
        if isinstance(v, dict) and not isinstance(v, ConfigDict):
            return cls(v)
        if isinstance(v, (list, tuple)) and type(v) in (list, tuple):
            return type(v)(cls._wrap(x) for x in v)
        return v

    def __setitem__(self, name, value):
        super().__setitem__(name, self._wrap(value))

    def __setattr__(self, name, value):
        self[name] = value

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError("'{}' object has no attribute '{}'".format(self.__class__.__name__, name)) from None

    def __delattr__(self, name):
        try:
            del self[name]
        except KeyError:
            raise AttributeError(name) from None

    def update(self, *args, **kwargs):
        for k, v in dict(*args, **kwargs).items():
            self[k] = v

    def setdefault(self, key, default=None):
        if key not in self:
            self[key] = default
        return self[key]

    def to_dict(self):
        def plain(v):
            if isinstance(v, dict):
                return {k: plain(x) for k, x in v.items()}
            if type(v) in (list, tuple):
                return type(v)(plain(x) for x in v)
            return v
        return plain(self)


def get_downsample_factor(model_config):
    """det3d/utils/config_tool.py:39-53: the neck's down strides multiplied, over its last up stride, times the backbone's
    ds_factor; a two-stage model's numbers are its first stage's"""
    if "neck" not in model_config:
        model_config = model_config["first_stage_cfg"]
    neck_cfg = model_config["neck"]
    downsample_factor = np.prod(neck_cfg.get("ds_layer_strides", [1]))
    if len(neck_cfg.get("us_layer_strides", [])) > 0:
        downsample_factor /= neck_cfg.get("us_layer_strides", [])[-1]
    downsample_factor *= model_config["backbone"]["ds_factor"]
    downsample_factor = int(downsample_factor)
    assert downsample_factor > 0
    return downsample_factor


_SHIM = ("det3d", "det3d.utils", "det3d.utils.config_tool")


class Config:
    """det3d.torchie.Config: attribute and item access to a config file's names"""

    @staticmethod
    def fromfile(filename):
        filename = os.path.abspath(os.path.expanduser(filename))
        if not os.path.isfile(filename):
            raise FileNotFoundError('file "{}" does not exist'.format(filename))
        if not filename.endswith(".py"):
            raise IOError("Only py type is supported here!")
        module_name = os.path.basename(filename)[:-3]
        if "." in module_name:
            raise ValueError("Dots are not allowed in config file path.")
        with open(filename, "r") as f:
            text = f.read()
        # the one import the configs make of the reference, for the duration of the run only
        saved_modules = {name: sys.modules.get(name) for name in _SHIM}
        saved_path = list(sys.path)
        try:
            parent = None
            for name in _SHIM:
                mod = types.ModuleType(name)
                mod.__path__ = []
                sys.modules[name] = mod
                if parent is not None:
                    setattr(parent, name.rsplit(".", 1)[1], mod)
                parent = mod
            parent.get_downsample_factor = get_downsample_factor
            sys.path.insert(0, os.path.dirname(filename))
            namespace = {"__file__": filename, "__name__": module_name}
            exec(compile(text, filename, "exec"), namespace)
        finally:
            sys.path[:] = saved_path
            for name, mod in saved_modules.items():
                if mod is None:
                    sys.modules.pop(name, None)
                else:
                    sys.modules[name] = mod
        cfg_dict = {name: value for name, value in namespace.items() if not name.startswith("__")}
        return Config(cfg_dict, filename=filename, text=text)

    def __init__(self, cfg_dict=None, filename=None, text=None):
        if cfg_dict is None:
            cfg_dict = dict()
        elif not isinstance(cfg_dict, dict):
            raise TypeError("cfg_dict must be a dict, but got {}".format(type(cfg_dict)))
        if text is None and filename:
            with open(filename, "r") as f:
                text = f.read()
        object.__setattr__(self, "_cfg_dict", ConfigDict(cfg_dict))
        object.__setattr__(self, "_filename", filename)
        object.__setattr__(self, "_text", text or "")

    @property
    def filename(self):
        return self._filename

    @property
    def text(self):
        return self._text

    def __repr__(self):
        return "Config (path: {}): {}".format(self.filename, self._cfg_dict.__repr__())

    def __len__(self):
        return len(self._cfg_dict)

    def __getattr__(self, name):
        return getattr(self._cfg_dict, name)

    def __getitem__(self, name):
        return self._cfg_dict[name]

    def __setattr__(self, name, value):
        self._cfg_dict[name] = value

    def __setitem__(self, name, value):
        self._cfg_dict[name] = value

    def __iter__(self):
        return iter(self._cfg_dict)

    def __contains__(self, name):
        return name in self._cfg_dict


# ------------------------------------------------------------------------------------------- the checkpoint door
def load_state_dict(module, state_dict, strict=False, logger=None):
    """checkpoint.py:42-93: copy what fits, collect unexpected keys, missing keys (BatchNorm's num_batches_tracked is not
    missed) and size mismatches, and report them in the reference's wording: raised with strict, printed otherwise"""
    unexpected_keys, shape_mismatch_pairs = [], []
    own_state = module.state_dict()
    for name, param in state_dict.items():
        if name not in own_state:
            unexpected_keys.append(name)
            continue
        if isinstance(param, torch.nn.Parameter):
            param = param.data
        if param.size() != own_state[name].size():
            shape_mismatch_pairs.append([name, own_state[name].size(), param.size()])
            continue
        own_state[name].copy_(param)
    all_missing_keys = set(own_state.keys()) - set(state_dict.keys())
    missing_keys = [key for key in all_missing_keys if "num_batches_tracked" not in key]
    err_msg = []
    if unexpected_keys:
        err_msg.append("unexpected key in source state_dict: {}\n".format(", ".join(unexpected_keys)))
    if missing_keys:
        err_msg.append("missing keys in source state_dict: {}\n".format(", ".join(missing_keys)))
    if shape_mismatch_pairs:
        # the reference draws this table with terminaltables; the rows are the same, the frame is plain
        rows = [["key", "expected shape", "loaded shape"]] + [[str(c) for c in row] for row in shape_mismatch_pairs]
        widths = [max(len(r[c]) for r in rows) for c in range(3)]
        table = "\n".join("| " + " | ".join(r[c].ljust(widths[c]) for c in range(3)) + " |" for r in rows)
        err_msg.append("these keys have mismatched shape:\n" + table)
    if len(err_msg) > 0:
        err_msg.insert(0, "The model and loaded state dict do not match exactly\n")
        err_msg = "\n".join(err_msg)
        if strict:
            raise RuntimeError(err_msg)
        elif logger is not None:
            logger.warning(err_msg)
        else:
            print(err_msg)


def load_checkpoint(model, filename, map_location="cpu", strict=False, logger=None):
    """checkpoint.py:122-173 for files (no URL scheme is served: this project never downloads): a bare state dict (an
    OrderedDict) or {"state_dict": ...}; `module.` is stripped when the first key has it. -> the loaded checkpoint"""
    if "://" in filename:
        raise IOError("{}: only checkpoint files are loaded here (no model zoo, no URL)".format(filename))
    if not os.path.isfile(filename):
        raise IOError("{} is not a checkpoint file".format(filename))
    checkpoint = torch.load(filename, map_location=map_location)
    if isinstance(checkpoint, OrderedDict):
        state_dict = checkpoint
    elif isinstance(checkpoint, dict) and "state_dict" in checkpoint:
        state_dict = checkpoint["state_dict"]
    else:
        raise RuntimeError("No state_dict found in checkpoint file {}".format(filename))
    if list(state_dict.keys())[0].startswith("module."):
        state_dict = {k[7:]: v for k, v in state_dict.items()}
    load_state_dict(model.module if hasattr(model, "module") else model, state_dict, strict, logger)
    return checkpoint


# ------------------------------------------------------------------------------------------- the model builder
def _plain(v):
    return v.to_dict() if isinstance(v, ConfigDict) else v


def _init_weights(model, pretrained):
    """single_stage.py:33-40"""
    if pretrained is None:
        return
    try:
        load_checkpoint(model, pretrained, strict=False)
        print("init weight from {}".format(pretrained))
    except Exception:
        print("no pretrained model at {}".format(pretrained))


def _voxel_kwargs(voxel_generator):
    """the config's voxel_generator dict (or WaymoDataset.voxel_generator) -> what the detectors' constructors call it"""
    if voxel_generator is None:
        return {}
    num = voxel_generator["max_voxel_num"]
    num = [num, num] if isinstance(num, int) else list(num)
    return dict(max_points=int(voxel_generator["max_points_in_voxel"]), max_voxels=int(num[1]),      # [1]: the val capacity
                voxel_size=list(voxel_generator["voxel_size"]), pc_range=list(voxel_generator["range"]))


def _one_stage_args(cfg, voxel):
    """-> (type, constructor arguments, pretrained path) of a PointPillars / VoxelNet dict"""
    args = dict(_plain(cfg))
    kind = args.pop("type")
    pretrained = args.pop("pretrained", None)       # tried here after the build: the classes' own door is strict
    for part in ("reader", "backbone", "neck", "bbox_head"):
        if isinstance(args.get(part), dict):
            args[part] = dict(args[part])
            # logging.getLogger("RPN") / ("CenterHead") in the configs: the reference's modules log their construction
            # through it; nothing here does, and a Logger is no part of a model
            args[part].pop("logger", None)
    if kind == "PointPillars":
        # the pillar reader carries voxel_size and pc_range itself; the generator's must be the same grid
        reader = args.get("reader", {})
        for mine, theirs in (("voxel_size", "voxel_size"), ("pc_range", "pc_range")):
            if voxel and mine in reader and [float(v) for v in reader[mine]] != [float(v) for v in voxel[theirs]]:
                raise ValueError(f"the reader's {mine} {list(reader[mine])} is not the voxel generator's {voxel[theirs]}")
        voxel = {k: v for k, v in voxel.items() if k in ("max_points", "max_voxels")}
    elif kind != "VoxelNet":
        raise KeyError(f"detector type {kind!r} is not built here (known: PointPillars, VoxelNet, TwoStageDetector)")
    return kind, dict(args, **voxel), pretrained


def build_detector(cfg, train_cfg=None, test_cfg=None, voxel_generator=None):
    """det3d.models.build_detector for `cfg.model`. voxel_generator: the config's dict of that name (range, voxel_size,
    max_points_in_voxel, max_voxel_num), handed to the constructors as max_points, max_voxels (the val capacity), voxel_size
    and pc_range: what `detect` voxelises with. A `pretrained` path is tried as single_stage.py:33-40 tries it: a missing
    file prints "no pretrained model at ..." and the build goes on. A keyword that a class does not know is refused by that
    class, by name (TypeError)."""
    from . import detector, two_stage
    voxel = _voxel_kwargs(voxel_generator)
    train_cfg, test_cfg = _plain(train_cfg), _plain(test_cfg)
    kind = cfg["type"]
    if kind == "TwoStageDetector":
        args = dict(_plain(cfg))
        args.pop("type")
        pretrained = args.pop("pretrained", None)
        first_kind, first_args, first_pretrained = _one_stage_args(args.pop("first_stage_cfg"), voxel)
        first = {"PointPillars": detector.PointPillars, "VoxelNet": detector.VoxelNet}[first_kind](
            **first_args, train_cfg=train_cfg, test_cfg=test_cfg)
        _init_weights(first, first_pretrained)
        model = two_stage.TwoStageDetector(first, **args, train_cfg=train_cfg, test_cfg=test_cfg)
        _init_weights(model, pretrained)
        return model
    kind, args, pretrained = _one_stage_args(cfg, voxel)
    model = {"PointPillars": detector.PointPillars, "VoxelNet": detector.VoxelNet}[kind](**args, train_cfg=train_cfg, test_cfg=test_cfg)
    _init_weights(model, pretrained)
    return model
