"""The seven run-kernel workspace sizes, pinned. Each dal3_*_workspace_bytes is its carve (dal3_block.h's Carver) run on a
null base; the numbers below are what the closed formulas returned before the carves replaced them, recorded from that
library over the grid (VOXELIZE: from the library before its sort's buffers became dal3_block.h's carve), so a carve
that drifts from the layout the kernels were written against fails here. No GPU."""
import importlib

hip = importlib.import_module("3dal_pytorch_amd._hip")

N = (0, 1, 63, 64, 65, 4095, 4096, 4097, 65536, 1000003)       # K, E, T
SEQS = (0, 1, 7)
CAPACITIES = (1, 500, 65536)
MAPS = ((1, 1, 1), (2, 32, 32), (4, 468, 468))                  # (B, H, W)

GROUP = (0, 1792, 1792, 1792, 2560, 50176, 50176, 51968, 802816, 12251648)      # per E, whatever T
CLASSIFY = (0, 512, 512, 512, 512, 512, 512, 512, 512, 8192)
TRACK = {                                                       # [S][K] -> per capacity
    0: ((0, 0, 0),
        (768, 768, 768),
        (768, 768, 768),
        (768, 768, 768),
        (1536, 1536, 1536),
        (49152, 49152, 49152),
        (49152, 49152, 49152),
        (49920, 49920, 49920),
        (786432, 786432, 786432),
        (12000768, 12000768, 12000768)),
    1: ((512, 48384, 6291712),
        (1280, 49152, 6292480),
        (1280, 49152, 6292480),
        (1280, 49152, 6292480),
        (2048, 49920, 6293248),
        (49664, 97536, 6340864),
        (49664, 97536, 6340864),
        (50432, 98304, 6341632),
        (786944, 834816, 7078144),
        (12001280, 12049152, 18292480)),
    7: ((1024, 336384, 44040448),
        (1792, 337152, 44041216),
        (1792, 337152, 44041216),
        (1792, 337152, 44041216),
        (2560, 337920, 44041984),
        (50176, 385536, 44089600),
        (50176, 385536, 44089600),
        (50944, 386304, 44090368),
        (787456, 1122816, 44826880),
        (12001792, 12337152, 56041216)),
}
MATCH = (0, 768, 1024, 1024, 1792, 65536, 65536, 66304, 1048576, 16000768)
NMS = {                                                         # [boxes_f64] -> per K
    0: (0, 1536, 4608, 4608, 6144, 294912, 294912, 296448, 4718592, 72001536),
    1: (0, 1536, 5888, 5888, 7424, 376832, 376832, 378368, 6029312, 92001536),
}
DECODE = (256, 256, 3584)
VOXELIZE = {                                                    # [B] -> per N
    1: (512, 3328, 3328, 3328, 4864, 100096, 100096, 102656, 1590784, 24268800),
    2: (512, 3328, 3328, 3328, 4864, 100096, 100096, 102656, 1590784, 24268800),
    300: (2816, 5632, 5632, 5632, 7168, 102400, 102400, 104960, 1593088, 24271104),
}


def test_workspace_sizes_are_the_recorded_ones():
    lib = hip.lib()
    for i, n in enumerate(N):
        for T in N:
            assert lib.dal3_group_workspace_bytes(n, T) == GROUP[i], (n, T)
        assert lib.dal3_motion_classify_workspace_bytes(n) == CLASSIFY[i], n
        assert lib.dal3_track_match_workspace_bytes(n) == MATCH[i], n
        for f64 in (0, 1):
            assert lib.dal3_nms_workspace_bytes(n, f64) == NMS[f64][i], (n, f64)
        for S in SEQS:
            for c, cap in enumerate(CAPACITIES):
                assert lib.dal3_track_workspace_bytes(S, n, cap) == TRACK[S][i][c], (S, n, cap)
        for B in VOXELIZE:
            assert lib.dal3_voxelize_workspace_bytes(B, n) == VOXELIZE[B][i], (B, n)
    for i, (B, H, W) in enumerate(MAPS):
        assert lib.dal3_center_decode_workspace_bytes(B, H, W) == DECODE[i], (B, H, W)


def test_invalid_arguments_still_size_to_zero():
    lib = hip.lib()
    big = (1 << 24) + 1                                     # DAL3_MAX_ITEMS + 1
    assert lib.dal3_group_workspace_bytes(-1, 4) == 0 and lib.dal3_group_workspace_bytes(4, -1) == 0
    assert lib.dal3_group_workspace_bytes(big, 4) == 0 and lib.dal3_group_workspace_bytes(4, big) == 0
    assert lib.dal3_motion_classify_workspace_bytes(-1) == 0 and lib.dal3_motion_classify_workspace_bytes(big) == 0
    assert lib.dal3_track_workspace_bytes(-1, 4, 500) == 0 and lib.dal3_track_workspace_bytes(1, -1, 500) == 0
    assert lib.dal3_track_workspace_bytes(1, 4, 0) == 0
    assert lib.dal3_track_workspace_bytes(1, 4, hip.TRACK_MAX_CAPACITY + 1) == 0
    assert lib.dal3_track_match_workspace_bytes(-1) == 0
    assert lib.dal3_nms_workspace_bytes(-1, 0) == 0 and lib.dal3_nms_workspace_bytes(8, 2) == 0
    assert lib.dal3_nms_workspace_bytes(big, 0) == 0
    assert lib.dal3_center_decode_workspace_bytes(-1, 4, 4) == 0 and lib.dal3_center_decode_workspace_bytes(1, big, 1) == 0
