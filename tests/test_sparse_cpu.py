"""CPU-side checks of the sparse 3-D middle (3dal_pytorch_amd/sparse.py, detector.VoxelNet; dal3_sp_* of include/dal3.h):
sparse_ref's two float64 formulations against each other, the planted faults against the measures, the fold's
restatement, the reference's key set (tests/golden/scn_keys.json, written by tests/golden/gen_scn.py), the ABI's layout
through a C compiler, and every refusal the host makes before a launch. No GPU compute here."""
import ctypes
import functools
import importlib
import json
import os

import numpy as np
import pytest
import torch

import rpn_ref as R
import sparse_ref as S
from _common import ROOT

hip = importlib.import_module("3dal_pytorch_amd._hip")
sparse = importlib.import_module("3dal_pytorch_amd.sparse")
detector = importlib.import_module("3dal_pytorch_amd.detector")
rpn = importlib.import_module("3dal_pytorch_amd.rpn")

ENTRIES = ("dal3_sp_sort_workspace_bytes", "dal3_sp_sort", "dal3_sp_downsample_workspace_bytes", "dal3_sp_downsample",
           "dal3_sp_table", "dal3_sp_conv_pack_floats", "dal3_sp_conv_pack", "dal3_sp_conv")
NECK = dict(layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[128, 256], us_layer_strides=[1, 2],
            us_num_filters=[256, 256], num_input_features=256)
MODEL = dict(reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5),
             backbone=dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8), neck=dict(type="RPN", **NECK),
             bbox_head=dict(type="CenterHead", **dict(R.HEAD, in_channels=512)))


@functools.lru_cache(maxsize=None)
def case():
    feats, idx, B, shape = S.backbone_case(5)
    sd = S.backbone_weights(5)
    rb, dn = S.Rulebook(B), S.Dense(B)
    return feats, idx, B, shape, sd, rb, S.backbone(rb, sd, feats, idx, shape), dn, S.backbone(dn, sd, feats, idx, shape)


def test_the_two_formulations_agree():
    *_, gathered, _, dense = case()
    assert gathered["bev"].shape == (3, 256, 5, 6)
    for k in ("bev",) + S.LEVELS:
        assert np.abs(gathered[k] - dense[k]).max() <= 1e-12 * np.abs(dense[k]).max(), k
        act = np.abs(dense[k][:1]).max(1) > 0
        assert act.any() and not act.all(), k               # clustered input: no level is saturated


def _table_from_mask(mask_out, mask_in, kernel, stride, padding):
    """the neighbour table read off the dense masks: row ids of the active cells in key order, looked up by array indexing"""
    rid = np.full(mask_in.shape, -1, np.int64)
    rid[mask_in] = np.arange(int(mask_in.sum()))
    o = np.argwhere(mask_out)                               # key order
    t = np.full((int(np.prod(kernel)), o.shape[0]), -1, np.int32)
    tap = 0
    for kz in range(kernel[0]):
        for ky in range(kernel[1]):
            for kx in range(kernel[2]):
                c = o[:, 1:] * np.asarray(stride) - np.asarray(padding) + np.asarray([kz, ky, kx])
                ok = np.all((c >= 0) & (c < np.asarray(mask_in.shape[1:])), 1)
                t[tap, ok] = rid[o[ok, 0], c[ok, 0], c[ok, 1], c[ok, 2]]
                tap += 1
    return o.astype(np.int32), t


def test_the_integers_of_the_two_formulations_agree_exactly():
    _, idx, B, shape, _, rb, _, dn, _ = case()
    assert set(rb.record) == set(dn.record) == {"res0", "conv2", "res1", "conv3", "res2", "conv4", "res3", "extra_conv"}
    prev = None
    for (name, _, kernel, stride, padding), res in zip(S.STEMS[1:], ("res1", "res2", "res3", None)):
        mask_in = dn.record["res0"] if prev is None else dn.record[prev]
        o, t = _table_from_mask(dn.record[name], mask_in, kernel, stride, padding)
        r = rb.record[name]
        assert r["indices"].shape[0] == o.shape[0] and np.array_equal(r["indices"], o), name        # counts and sites, in key order
        if prev is not None:                                # level 0 keeps the caller's order: its rows are not key-ordered
            assert np.array_equal(r["table"], t), name
        if res is not None:
            _, t27 = _table_from_mask(dn.record[name], dn.record[name], (3, 3, 3), (1, 1, 1), (1, 1, 1))
            assert np.array_equal(rb.record[res]["table"], t27), res
        prev = name
    # level 0, in the caller's (scrambled) order: through the rows' ranks by key
    rank = np.argsort(np.argsort(S.keys_of(idx, B, shape), kind="stable"), kind="stable")
    _, t27 = _table_from_mask(dn.record["res0"], dn.record["res0"], (3, 3, 3), (1, 1, 1), (1, 1, 1))
    inv = np.argsort(rank)
    want = np.where(t27[:, rank] >= 0, inv[np.maximum(t27[:, rank], 0)], -1)
    assert np.array_equal(rb.record["res0"]["table"], want)
    _, tdown = _table_from_mask(dn.record["conv2"], dn.record["res0"], (3, 3, 3), (2, 2, 2), (1, 1, 1))
    assert np.array_equal(rb.record["conv2"]["table"], np.where(tdown >= 0, inv[np.maximum(tdown, 0)], -1))
    # the sort the kernels search
    key, pos = S.sort_sites(idx, B, shape, capacity=idx.shape[0] + 5)
    assert np.all(np.diff(key) >= 0) and np.array_equal(key[:idx.shape[0]], np.sort(S.keys_of(idx, B, shape)))
    assert (key[idx.shape[0]:] == B * int(np.prod(shape))).all() and np.array_equal(idx[pos[:idx.shape[0]]], S.unkey(key[:idx.shape[0]], shape))


def _both_tables(idx, B, shape, kernel, stride, padding, what):
    """the dict walk and its vectorised twin, on the strided window and on the 27-tap table of its output -> count of hits"""
    idx = np.asarray(idx, np.int32)
    o, osh = S.downsample(idx, B, shape, kernel, stride, padding)
    hits = 0
    for args in ((idx, idx, B, shape, shape, (3, 3, 3), (1, 1, 1), (1, 1, 1)), (o, idx, B, shape, osh, kernel, stride, padding),
                 (o, o, B, osh, osh, (3, 3, 3), (1, 1, 1), (1, 1, 1))):
        slow, fast = S.table(*args), S.table_sorted(*args)
        assert slow.dtype == fast.dtype == np.int32 and slow.shape == fast.shape and np.array_equal(slow, fast), what
        hits += int((slow >= 0).sum())
    return hits


def test_the_vectorised_table_is_the_dict_walk():
    import sparse_book_cases as K
    import sparse_train_ref as T
    from test_gpu_sparse import BOOK_CASES
    k3s2 = ((3, 3, 3), (2, 2, 2), (1, 1, 1))
    for name, (idx, B, shape) in BOOK_CASES.items():
        for _, _, kernel, stride, padding in S.STEMS[1:len(K.levels(shape))]:      # every level the bookkeeping test walks
            assert _both_tables(idx, B, shape, kernel, stride, padding, name) > 0
            idx, shape = S.downsample(idx, B, shape, kernel, stride, padding)
    idx, B, shape = BOOK_CASES["n65"]
    bad = idx.copy()
    bad[10, 3], bad[50, 0], bad[7, 1] = shape[2], B, -1                     # past the grid, past the batch, negative
    _both_tables(bad, B, shape, *k3s2, "bad coordinate")
    t = S.table_sorted(bad, bad, B, shape, shape, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    assert (t[:, [7, 10, 50]] == -1).all() and not np.isin(t, [7, 10, 50]).any()       # a bad row has no tap and is nobody's neighbour
    dup = idx.copy()
    dup[20], dup[41] = dup[3], dup[3]
    _both_tables(dup, B, shape, *k3s2, "duplicate")
    t = S.table_sorted(dup, dup, B, shape, shape, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    assert (t[13, [3, 20, 41]] == 41).all()                                 # the last row of a key answers, as in the dict
    idx, B, shape = K.window_sites()
    for kernel, stride, padding in K.window_cases():
        assert _both_tables(idx, B, shape, kernel, stride, padding, (kernel, stride, padding)) > 0
        # and the transposed table that scales (sparse_train_ref.inverse_table) is the forward one read backwards
        o, osh = S.downsample(idx, B, shape, kernel, stride, padding)
        fwd = S.table_sorted(o, idx, B, shape, osh, kernel, stride, padding)
        assert np.array_equal(T.inverse_table(idx, o, B, shape, osh, kernel, stride, padding), T.inverse_brute(fwd, idx.shape[0]))


def test_check_grid_is_sp_grid_ok():
    """sparse._check_grid and the library's sp_grid_ok on the largest grid and on the first one refused. The library compares
    cells with floor((2^31 - 1) / B); the product B * cells < 2^31 - 1 that _check_grid used to take admits one more cell count
    for every B >= 2 (2^31 - 1 is prime), which the library then refused. _check_grid now divides as the library does."""
    import sparse_book_cases as K
    lib = hip.lib()
    sort = lambda B, shape: hip.SpSortArgs(B=B, shape=I3(*shape), capacity=0, status=FAKE)       # capacity 0: nothing is launched
    B, shape = K.WIDTH_GRIDS["largest"]
    sparse._check_grid(B, shape)
    assert lib.dal3_sp_sort(sort(B, shape), None) == hip.OK
    B, shape = K.FIRST_REFUSED
    assert B * int(np.prod(shape, dtype=np.int64)) == 2 ** 31 - 2 and not K.admissible(B, shape)
    _err(lib.dal3_sp_sort(sort(B, shape), None), "2^31 - 1")
    with pytest.raises(ValueError, match="31-bit"):
        sparse._check_grid(B, shape)
    for B, shape in ((1, (2, 32767, 32768)), (1, (1, 46341, 46340)), (65535, (1, 1, 32768)), (65535, (1, 1, 32769)), (65536, (1, 1, 1)),
                     (1, (1, 1, 65537)), (1, (65536, 1, 1)), (3, (5, 7, 9)), *K.WIDTH_GRIDS.values()):
        rc = lib.dal3_sp_sort(sort(B, shape), None)
        assert rc in (hip.OK, hip.EINVAL)
        if rc == hip.OK:
            sparse._check_grid(B, shape)
        else:
            with pytest.raises(ValueError):
                sparse._check_grid(B, shape)
        assert K.admissible(B, shape) == (rc == hip.OK), (B, shape)


def test_planted_faults_are_caught_at_ten_times_the_bars():
    feats, idx, B, shape, sd, _, _, _, truth = case()
    f32 = S.backbone(S.Dense(B, torch.float32), sd, feats, idx, shape)
    yard = S.judge(f32["bev"], truth["bev"])
    assert all(0 < yard[k] < 1e-4 for k in S.MEASURES)
    worst = np.inf
    for fault in S.FAULTS:
        wrong = S.backbone(S.Dense(B, fault=fault), sd, feats, idx, shape)
        ratio, _, _ = S.ratios(wrong["bev"], f32["bev"], truth["bev"])
        for k in S.MEASURES:
            assert ratio[k] >= 10 * S.BARS[k], (fault, k, ratio[k])
            worst = min(worst, ratio[k])
    assert all(S.BARS[k] < worst / 10 for k in S.MEASURES)     # every bar is under a tenth of the smallest planted-fault ratio


def test_fold_is_the_dense_stages_arithmetic():
    w, b, bn = S.layer_weights("fold", (3, 3, 3), 16, 32, True, True)
    wf, bf = S.fold(w, b, bn)
    rw, rb_ = R.fold(np.ascontiguousarray(w.transpose(4, 3, 0, 1, 2)), b, bn, S.EPS)     # the same operations on (c_out, ...)
    assert np.array_equal(wf.transpose(4, 3, 0, 1, 2).view(np.uint32), rw.view(np.uint32)) and np.array_equal(bf.view(np.uint32), rb_.view(np.uint32))
    g, beta, mean, var = (np.asarray(v, np.float64) for v in bn)
    assert np.array_equal(bf, ((np.asarray(b, np.float64) - mean) * (g / np.sqrt(var + 1e-3)) + beta).astype(np.float32))
    w0, b0 = S.fold(w, None, None)
    assert np.array_equal(w0, w) and not b0.any()


def test_state_dict_keys_are_the_references():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "scn_keys.json")))
    for c in (5, 6):
        m = sparse.SpMiddleResNetFHD(num_input_features=c, ds_factor=8)
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == g[str(c)]
        assert {k: tuple(np.shape(v)) for k, v in S.backbone_weights(c).items()} == {k: tuple(s) for k, s in g[str(c)]}
    keys = dict(g["5"])
    assert keys["conv_input.0.weight"] == [3, 3, 3, 5, 16] and keys["extra_conv.0.weight"] == [3, 1, 1, 128, 128]
    assert keys["conv4.0.weight"] == [3, 3, 3, 64, 128] and "conv_input.0.bias" not in keys and keys["conv2.3.conv1.bias"] == [32]
    model = detector.VoxelNet(**MODEL)
    sd = model.state_dict()
    assert {k.split(".")[0] for k in sd} == {"backbone", "neck", "bbox_head"}           # the voxel-mean reader has no parameters
    assert {k[len("backbone."):] for k in sd if k.startswith("backbone.")} == set(keys)
    assert {k[len("neck."):] for k in sd if k.startswith("neck.")} == set(rpn.RPN(**NECK).state_dict())
    assert sd["neck.blocks.0.1.weight"].shape == (128, 256, 3, 3) and sd["bbox_head.shared_conv.0.weight"].shape == (64, 512, 3, 3)


def test_the_voxelnet_neck_and_head_build_and_run():
    neck, head = rpn.RPN(**NECK).eval(), rpn.CenterHead(**dict(R.HEAD, in_channels=512)).eval()
    assert neck.hip_serves() and head.hip_serves()
    with torch.no_grad():
        y = neck.train().composite(torch.zeros(1, 256, 6, 8))
        assert y.shape == (1, 512, 6, 8)
        out = head.train().composite(y)
    assert out[0]["hm"].shape == (1, 3, 6, 8)


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dal3.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRIES:
        assert name + "(" in header and name in hip.SIGNATURES and hasattr(lib, name), name
    assert "DAL3_SP_OVERFLOW = 256, DAL3_SP_BAD_COORD = 512, DAL3_SP_DUPLICATE = 1024, DAL3_SP_BAD_WEIGHT = 2048" in header
    assert (hip.SP_OVERFLOW, hip.SP_BAD_COORD, hip.SP_DUPLICATE, hip.SP_BAD_WEIGHT) == (256, 512, 1024, 2048)
    assert "dal3_spconv.hip" in open(os.path.join(ROOT, "3dal_pytorch_amd", "csrc", "Makefile")).read()


def test_sizes_are_the_carve_and_the_pack_layout():
    lib = hip.lib()
    al = lambda b: (b + 255) & ~255
    sort = lambda n: 4 * al(4 * n) + al(4 * 256 * ((n + 4095) // 4096))
    assert lib.dal3_sp_sort_workspace_bytes(1000) == sort(1000)
    assert lib.dal3_sp_downsample_workspace_bytes(1000, 8) == sort(8000) + al(4 * ((8000 + 255) // 256)) + al(8)
    assert lib.dal3_sp_sort_workspace_bytes(-1) == 0 and lib.dal3_sp_downsample_workspace_bytes(10, 0) == 0
    # a flag section, the folded bias of every 32-row tile, [tap][4 k-steps][out tile][lane] float4 fragments
    assert lib.dal3_sp_conv_pack_floats(27, 5, 16) == 64 + 32 + 27 * 1 * 1 * 256
    assert lib.dal3_sp_conv_pack_floats(27, 64, 128) == 64 + 128 + 27 * 8 * 4 * 256
    assert lib.dal3_sp_conv_pack_floats(3, 128, 128) == 64 + 128 + 3 * 16 * 4 * 256
    for bad in ((0, 16, 16), (28, 16, 16), (27, 9, 16), (27, 16, 48), (27, 256, 16)):
        assert lib.dal3_sp_conv_pack_floats(*bad) == 0


FAKE = 0x1000                                   # never dereferenced: every case fails before a launch
I3 = ctypes.c_int32 * 3


def _err(rc, word):
    assert rc == hip.EINVAL and word.encode() in hip.lib().dal3_last_error(), hip.lib().dal3_last_error()


def test_the_c_abi_refuses_bad_arguments_before_any_launch():
    lib = hip.lib()
    sort = lambda **kw: hip.SpSortArgs(**dict(dict(B=2, shape=I3(41, 1504, 1504), capacity=10, indices=FAKE, sorted_key=FAKE,
                                                   sorted_pos=FAKE, status=FAKE, workspace=FAKE, workspace_bytes=1 << 20), **kw))
    _err(lib.dal3_sp_sort(None, None), "null args")
    _err(lib.dal3_sp_sort(sort(B=24), None), "2^31 - 1")                         # 24 x 41 x 1504 x 1504 needs 32 bits
    assert 23 * 41 * 1504 * 1504 < 2 ** 31 - 1 <= 24 * 41 * 1504 * 1504
    _err(lib.dal3_sp_sort(sort(shape=I3(41, 0, 1504)), None), "every axis")
    _err(lib.dal3_sp_sort(sort(status=None), None), "null status")
    _err(lib.dal3_sp_sort(sort(max_workgroups=-1), None), "max_workgroups")
    assert lib.dal3_sp_sort(sort(workspace_bytes=16), None) == hip.EWORKSPACE
    down = lambda **kw: hip.SpDownsampleArgs(**dict(dict(B=1, in_shape=I3(41, 37, 45), out_shape=I3(21, 19, 23), kernel=I3(3, 3, 3),
                                                         stride=I3(2, 2, 2), padding=I3(1, 1, 1), in_capacity=10, in_indices=FAKE,
                                                         out_capacity=80, out_indices=FAKE, out_key=FAKE, n_out=FAKE, status=FAKE,
                                                         workspace=FAKE, workspace_bytes=1 << 20), **kw))
    _err(lib.dal3_sp_downsample(down(out_shape=I3(20, 19, 23)), None), "out_shape[0]")
    _err(lib.dal3_sp_downsample(down(kernel=I3(4, 3, 3)), None), "kernel 1 .. 3")
    _err(lib.dal3_sp_downsample(down(n_out=None), None), "n_out")
    table = lambda **kw: hip.SpTableArgs(**dict(dict(B=1, in_shape=I3(5, 5, 6), out_shape=I3(2, 5, 6), kernel=I3(3, 1, 1), stride=I3(2, 1, 1),
                                                     padding=I3(0, 0, 0), out_capacity=8, out_indices=FAKE, in_capacity=8, in_key=FAKE,
                                                     table=FAKE), **kw))
    _err(lib.dal3_sp_table(table(table=None), None), "null out_indices / table")
    _err(lib.dal3_sp_table(table(out_shape=I3(3, 5, 6)), None), "out_shape[0]")
    conv = lambda **kw: hip.SpConvArgs(**dict(dict(taps=27, c_in=16, c_out=32, relu=1, center_tap=13, in_capacity=8, x=FAKE, out_capacity=8,
                                                   table=FAKE, packed=FAKE, y=FAKE, status=FAKE), **kw))
    _err(lib.dal3_sp_conv(conv(c_in=24), None), "channels")
    _err(lib.dal3_sp_conv(conv(relu=2), None), "relu")
    _err(lib.dal3_sp_conv(conv(center_tap=27), None), "center_tap")
    _err(lib.dal3_sp_conv(conv(packed=FAKE + 4), None), "16-byte")
    _err(lib.dal3_sp_conv(conv(y=None), None), "no output")
    _err(lib.dal3_sp_conv(conv(x=FAKE + 4), None), "16-byte aligned")
    _err(lib.dal3_sp_conv(conv(y=None, canvas=FAKE, canvas_B=1, canvas_shape=I3(2, 5, 6)), None), "out_indices")
    layer = hip.Layer(FAKE, None, FAKE, None, None, None, 16, 32)
    _err(lib.dal3_sp_conv_pack(layer, 27, 1e-3, FAKE, None, None), "all four")
    _err(lib.dal3_sp_conv_pack(hip.Layer(FAKE, None, None, None, None, None, 16, 24), 27, 1e-3, FAKE, None, None), "channels")


def test_python_refusals():
    with pytest.raises(ValueError, match="31-bit"):
        sparse._check_grid(24, (41, 1504, 1504))
    sparse._check_grid(4, (41, 1504, 1504))                 # the production grid at B = 4 fits
    f, i = torch.zeros(4, 5), torch.zeros(4, 4, dtype=torch.int32)
    with pytest.raises(TypeError, match="tensor"):
        sparse.SparseConvTensor(np.zeros((4, 5), np.float32), i, (41, 37, 45), 1)
    with pytest.raises(ValueError, match="float32"):
        sparse.SparseConvTensor(f.double(), i, (41, 37, 45), 1)
    with pytest.raises(ValueError, match="int32"):
        sparse.SparseConvTensor(f, i.long(), (41, 37, 45), 1)
    with pytest.raises(ValueError, match="int32"):
        sparse.SparseConvTensor(f, i[:, :3], (41, 37, 45), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sparse.SparseConvTensor(f, i, (41, 37, 45), 1)
    m = sparse.SpMiddleResNetFHD(num_input_features=5)
    with pytest.raises(RuntimeError, match="eval-mode"):
        m.train()(f, i, 1, [45, 37, 40])
    with pytest.raises(RuntimeError, match="eval-mode"):
        sparse.SparseBasicBlock(16, 16).train()(None)
    with pytest.raises(NotImplementedError):
        sparse.SparseBasicBlock(16, 32)
    assert sparse.out_shape((41, 1504, 1504), (3, 3, 3), (2, 2, 2), (1, 1, 1)) == (21, 752, 752)
    assert sparse.out_shape((11, 376, 376), (3, 3, 3), (2, 2, 2), (0, 1, 1)) == (5, 188, 188)
    assert sparse.out_shape((5, 188, 188), (3, 1, 1), (2, 1, 1), (0, 0, 0)) == (2, 188, 188)
    assert sparse.candidates((3, 3, 3), (2, 2, 2)) == 8 and sparse.candidates((3, 1, 1), (2, 1, 1)) == 2
    assert sparse.safe_capacity(100, 1, (41, 37, 45), (3, 3, 3), (2, 2, 2), (1, 1, 1)) == 800
    assert sparse.safe_capacity(100000, 1, (5, 5, 6), (3, 1, 1), (2, 1, 1), (0, 0, 0)) == 60


def test_the_detector_builds_and_refuses_what_is_not_built():
    model = detector.VoxelNet(**MODEL)
    assert isinstance(model.backbone, sparse.SpMiddleResNetFHD) and type(model.reader).__name__ == "VoxelFeatureExtractorV3"
    assert (model.max_points, model.max_voxels) == (5, 150000)
    with pytest.raises(NotImplementedError, match="loss is not built"):
        model({}, return_loss=True)
    with pytest.raises(NotImplementedError, match="second stage"):
        model.forward_two_stage({})
    with pytest.raises(RuntimeError, match="voxel_size and pc_range"):
        model.eval().detect(torch.zeros(4, 5), [0, 4])
    with pytest.raises(KeyError, match=r"SpMiddleResNetFHD.*|known: \['PointPillarsScatter', 'SpMiddleResNetFHD'\]"):
        detector._build(dict(type="SpMiddleFHD"), detector.BACKBONES, "backbone")
    with pytest.raises(KeyError, match="VoxelFeatureExtractorV3"):
        detector._build(dict(type="VoxelFeatureExtractor"), detector.READERS, "reader")
    assert set(detector.BACKBONES) == {"PointPillarsScatter", "SpMiddleResNetFHD"}
