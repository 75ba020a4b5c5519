"""The byte counts of the PointNet heads' packed blobs, pinned: what dal3_pack_weights returns with packed_dev == NULL
for every head kind x dtype (each is its layout walk of csrc/dal3_api.hip run on a null base, plus the ring's tail where
the blob has one). The numbers were recorded from the library in front of the commit that merged the walks' measure and
view helpers, so a walk that drifts from the layout the kernels read fails here. No GPU."""
import ctypes as C
import importlib

hip = importlib.import_module("3dal_pytorch_amd._hip")

BYTES = {                                                       # [head kind] -> fp32, bf16, fp16, f16x3
    hip.HEAD_INS_SEG: (5983232, 2895616, 2895616, 3615488),
    hip.HEAD_STATIC_BOX_EST: (3166720, 1982720, 1982720, 2375936),
    hip.HEAD_POINT_EMB: (3092480, 1941248, 1941248, 2301696),
    hip.HEAD_BOX_EMB: (677888, 530432, 530432, 694272),
    hip.HEAD_DYNAMIC_BOX_EST: (283392, 283392, 283392, 283392),
}


def test_packed_sizes_are_the_recorded_ones():
    lib = hip.lib()
    for kind, row in BYTES.items():
        for dtype, want in zip((hip.F32, hip.BF16, hip.F16, hip.F16X3), row):
            need = C.c_size_t(0)
            assert lib.dal3_pack_weights(kind, None, 0, dtype, None, C.byref(need), None) == hip.OK, (kind, dtype)
            assert need.value == want, (kind, dtype, need.value, want)
