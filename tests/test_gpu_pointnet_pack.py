"""The PointNet heads' packed blobs, pinned byte for byte: every case of tests/pointnet_pack_cases.py (five head kinds,
ins_seg with 3 and 4 input channels, four dtypes, one planted case per guard flag) is packed by dal3_pack_weights and
compared with tests/golden/pointnet_blobs.npz (tests/golden/gen_pointnet_blobs.py): the byte count, the CRC-32 of every
4096-byte page and the SHA-256 of the whole blob. A layout, bound-coefficient or flag edit that end-to-end parity would
let through fails here, at the first differing page."""
import hashlib

import numpy as np
import pytest

from _common import golden
import pointnet_pack_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want():
    return golden("pointnet_blobs")


def test_golden_covers_exactly_the_cases(want):
    assert sorted({k.rsplit("/", 1)[0] for k in want}) == sorted(P.CASES)


@pytest.mark.parametrize("case", P.CASES)
def test_blob_is_the_recorded_one(case, want):
    blob = P.pack(case)
    assert blob.size == int(want[f"{case}/size"]), (case, "byte count", blob.size, int(want[f"{case}/size"]))
    crc = P.page_crcs(blob)
    diff = np.nonzero(crc != want[f"{case}/crc"])[0]
    assert diff.size == 0, f"{case}: {diff.size} of {crc.size} pages differ, the first at byte offset {int(diff[0]) * P.PAGE}"
    sha = np.frombuffer(hashlib.sha256(blob.tobytes()).digest(), np.uint8)
    assert np.array_equal(sha, want[f"{case}/sha"]), (case, "SHA-256 differs although every page's CRC-32 agrees")
