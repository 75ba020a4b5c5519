"""The whole C boundary at once: every ctypes.Structure, every SIGNATURES entry and every integer constant of
3dal_pytorch_amd/_hip.py against include/dal3.h as a C compiler lays it out (tests/abi_check.py: one compile, one run), and
the checker itself against planted faults. A new struct, entry or constant is covered without a test of its own. No GPU."""
import ctypes
import importlib
import os

import pytest

import abi_check as A
from _common import ROOT

hip = importlib.import_module("3dal_pytorch_amd._hip")

# dal3_optim_hyper has no Structure: solver.py addresses its 8-byte fields as slots OPTIM_<FIELD> of one int64 / float64 block
SLOT_STRUCTS = ("dal3_optim_hyper",)
# header constants with no int of their name in _hip.py, and why
UNMIRRORED = {
    "DAL3_VERSION": "read from the header where it is needed (__graft_entry__.header_version)",
    **{k: "the library's own upper bounds; the binding never sizes anything by them"
       for k in ("DAL3_MAX_ITEMS", "DAL3_MAX_POINTS_PER_ITEM", "DAL3_MAX_TILES")},
    **{"DAL3_BM_" + k: "metrics.py builds f64_fields / i32_fields from the field order, bit by bit"
       for k in ("CENTER", "HEADING_SCORES", "HEADING_RESIDUALS", "SIZE_SCORES", "SIZE_RESIDUALS", "CENTER_LABEL",
                 "HEADING_RESIDUAL_LABEL", "SIZE_RESIDUAL_LABEL", "HEADING_CLASS_LABEL", "SIZE_CLASS_LABEL")},
    **{"DAL3_ROI_CLS_SCORE_" + k: "held by the dict ROI_CLS_SCORE under the configuration's spelling (checked below)"
       for k in ("ROI_IOU", "CLS")},
}
# sizes that the header's comments, DESIGN.md or earlier tests state as numbers: a change of one is a change of the ABI
SIZES = {"dal3_score_acc": 72, "dal3_box_metric_acc": 48, "dal3_box_metric_args": 280, "dal3_optim_chunk": 24,
         "dal3_optim_hyper": 80, "dal3_center_targets_args": 792, "dal3_center_loss_args": 400, "dal3_gt_paste_args": 88,
         "dal3_augment_points_args": 184, "dal3_augment_boxes_args": 136}


@pytest.fixture(scope="module")
def abi(tmp_path_factory):
    return A.measure(os.path.join(ROOT, "include", "dal3.h"), tmp_path_factory.mktemp("abi"))


@pytest.fixture(scope="module")
def mirrors():
    return A.mirrors_of(hip)


def test_every_struct_has_the_headers_layout(abi, mirrors):
    assert A.check_structs(mirrors, abi, SLOT_STRUCTS) == []
    slots = {f: getattr(hip, "OPTIM_" + f.upper(), None) for _, f, _ in abi.structs["dal3_optim_hyper"]}
    assert A.check_slots("dal3_optim_hyper", slots, hip.OPTIM_SLOTS, abi) == []
    assert A.check_slots("dal3_optim_hyper", dict(slots, lr=2, beta1=1), 11, abi) == [
        ("dal3_optim_hyper", "11 slots, header sizeof 80"), ("dal3_optim_hyper.lr", "slot 2, header (offset, size) (8, 8)"),
        ("dal3_optim_hyper.beta1", "slot 1, header (offset, size) (16, 8)")]
    n_fields = sum(len(f) for f in abi.structs.values())
    print(f"checked {len(abi.structs)} structs, {n_fields} fields")
    assert len(abi.structs) >= 41 and len(mirrors) >= 40


def test_pinned_sizes(abi, mirrors):
    by_name = {c: t for t, c in mirrors.items()}
    for cname, n in SIZES.items():
        assert abi.sizes[cname] == n, cname
        assert cname in SLOT_STRUCTS or ctypes.sizeof(by_name[cname]) == n, cname


def test_every_signature_has_the_prototypes_classes(abi, mirrors):
    assert A.check_signatures(hip.SIGNATURES, abi, mirrors) == []
    n_params = sum(len(p) for _, p in abi.prototypes.values())
    print(f"checked {len(abi.prototypes)} prototypes, {n_params} parameters")
    assert len(abi.prototypes) >= 164


def test_every_constant_is_mirrored_or_listed(abi):
    assert A.check_constants(vars(hip), abi, UNMIRRORED) == []
    assert hip.ROI_CLS_SCORE == {k: abi.constants["DAL3_ROI_CLS_SCORE_" + k.upper()] for k in ("roi_iou", "cls")}
    print(f"checked {len(abi.constants) - len(UNMIRRORED)} constants against _hip.py, {len(UNMIRRORED)} listed")
    assert len(abi.constants) - len(UNMIRRORED) >= 72


# ---- the checker on planted faults: Python objects made here, each reported by name and nothing else reported
def _plant(cls, change):
    fields = list(cls._fields_)
    change(fields, [f[0] for f in fields].index)
    return type(cls.__name__ + "Plant", (ctypes.Structure,), {"_fields_": fields})


def _where(findings):
    return {w for w, _ in findings}


def test_planted_swap_of_equal_width_neighbours(abi, mirrors):
    def swap(fields, at):
        i = at("yaw_col")
        assert fields[i + 1] == ("boxes_f64", ctypes.c_int32)
        fields[i], fields[i + 1] = fields[i + 1], fields[i]
    got = A.check_struct("dal3_nms_args", _plant(hip.NmsArgs, swap), abi, mirrors)
    assert _where(got) == {"dal3_nms_args.yaw_col", "dal3_nms_args.boxes_f64"}


@pytest.mark.parametrize("pad", ["explicit", "alignment"])
def test_planted_narrow_field_with_later_offsets_intact(abi, mirrors, pad):
    """in_capacity as int32: with a pad field of its own, and with the pad that the next pointer's alignment gives"""
    def narrow(fields, at):
        i = at("in_capacity")
        fields[i] = ("in_capacity", ctypes.c_int32)
        if pad == "explicit":
            fields.insert(i + 1, ("pad", ctypes.c_int32))
    t = _plant(hip.SpConvArgs, narrow)
    assert ctypes.sizeof(t) == ctypes.sizeof(hip.SpConvArgs) and t.x.offset == hip.SpConvArgs.x.offset
    got = A.check_struct("dal3_sp_conv_args", t, abi, mirrors)
    assert _where(got) == {"dal3_sp_conv_args.in_capacity"} | ({"dal3_sp_conv_args.pad"} if pad == "explicit" else set())
    assert any(w.endswith("in_capacity") and "(24, 4)" in what for w, what in got)


def test_planted_dropped_trailing_field(abi, mirrors):
    got = A.check_struct("dal3_nms_args", _plant(hip.NmsArgs, lambda fields, at: fields.pop()), abi, mirrors)
    assert _where(got) == {"dal3_nms_args", "dal3_nms_args.workspace_bytes"}


def test_planted_float_for_int_of_equal_width(abi, mirrors):
    def retype(fields, at):
        fields[at("mirror")] = ("mirror", ctypes.c_float)
    got = A.check_struct("dal3_nms_args", _plant(hip.NmsArgs, retype), abi, mirrors)
    assert _where(got) == {"dal3_nms_args.mirror"}


def test_planted_struct_without_a_name_and_header_struct_without_a_mirror(abi, mirrors):
    module = type(hip)("fake")
    module.Nameless = type("Nameless", (ctypes.Structure,), {"__module__": "fake", "_fields_": [("x", ctypes.c_int)]})
    assert _where(A.check_structs({**mirrors, **A.mirrors_of(module)}, abi, SLOT_STRUCTS)) == {"Nameless"}
    less = {t: c for t, c in mirrors.items() if t is not hip.Map}
    assert "dal3_map" in _where(A.check_structs(less, abi, SLOT_STRUCTS))
    twice = {**mirrors, _plant(hip.Map, lambda fields, at: None): "dal3_map"}
    assert _where(A.check_structs(twice, abi, SLOT_STRUCTS)) == {"dal3_map"}


def _signatures(name, change):
    res, args = hip.SIGNATURES[name]
    args = list(args)
    change(args)
    return dict(hip.SIGNATURES, **{name: (res, args)})


def test_planted_signature_faults(abi, mirrors):
    name = "dal3_tr_linear_bn_stats"
    params = [p for _, p in abi.prototypes[name][1]]
    assert len(params) == 29 and hip.SIGNATURES[name][1][4] is hip.vp and hip.SIGNATURES[name][1][1] is ctypes.c_int64

    got = A.check_signatures(_signatures(name, lambda a: a.pop(4)), abi, mirrors)
    assert got == [(name, "28 arguments, header 29")]
    got = A.check_signatures(_signatures(name, lambda a: a.__setitem__(1, ctypes.c_int)), abi, mirrors)
    assert _where(got) == {f"{name}.{params[1]}"} and abi.prototypes[name][1][1][0] == "int64_t"

    name = "dal3_pillar_pack"
    i = hip.SIGNATURES[name][1].index(ctypes.c_double)
    assert abi.prototypes[name][1][i][0] == "double"
    got = A.check_signatures(_signatures(name, lambda a: a.__setitem__(i, ctypes.c_float)), abi, mirrors)
    assert _where(got) == {f"{name}.{abi.prototypes[name][1][i][1]}"}

    table = dict(hip.SIGNATURES, dal3_version=(ctypes.c_size_t, []))
    del table["dal3_nms"]
    assert _where(A.check_signatures(table, abi, mirrors)) == {"dal3_version return", "dal3_nms"}


def test_planted_constant_faults(abi):
    off_by_one = dict(vars(hip), NMS_MAX_PRE=hip.NMS_MAX_PRE + 1)
    assert A.check_constants(off_by_one, abi, UNMIRRORED) == [("DAL3_NMS_MAX_PRE", "65537, header 65536")]
    unlisted = {k: v for k, v in UNMIRRORED.items() if k != "DAL3_MAX_TILES"}
    assert _where(A.check_constants(vars(hip), abi, unlisted)) == {"DAL3_MAX_TILES"}
    assert _where(A.check_constants(vars(hip), abi, dict(UNMIRRORED, DAL3_OK="", DAL3_GONE=""))) == {"DAL3_OK", "DAL3_GONE"}


def test_a_declaration_outside_the_two_shapes_is_refused():
    for decl in ("int (*fn)", "float *x", "int", "", "double a, *b"):
        with pytest.raises(ValueError, match="does not fit the parse"):
            A.declarators(decl)
