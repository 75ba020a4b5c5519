#!/usr/bin/env python3
"""Generate tests/golden/pointnet_blobs.npz: what dal3_pack_weights writes for every case of tests/pointnet_pack_cases.py,
recorded from the library that is built in the tree. Run once on the MI355X:
    python tests/golden/gen_pointnet_blobs.py [output.npz]

The golden pins the packers BEFORE a change to them, so it is generated with the library of the commit in front of that
change (the committed file: d58bfbf, the parent of the commit that merged the PointNet packers).

Per case: `size` (the blob's byte count), `crc` (zlib.crc32 of every 4096-byte page) and `sha` (SHA-256 of the whole
blob). dal3_pack_weights zero-fills the blob before it packs, so the bytes are deterministic; every case is packed twice
here and the two blobs must be equal. A planted case whose page checksums equal its clean twin's is refused, and so is a
plant that did not set its flag word (or a twin in which that word is set): a plant that never reached its guard would
otherwise look pinned. The f16x3 plant must hold fp16 NaNs where its twin holds none. Fixed timestamps: a rerun
reproduces the archive byte for byte."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gen_pillars as G  # noqa: E402
import pointnet_pack_cases as P  # noqa: E402


def f16_nans(blob):
    h = blob.view(np.uint16)
    return int(((h & 0x7C00) == 0x7C00).sum() - ((h & 0x7FFF) == 0x7C00).sum())


def main():
    out, blobs = {}, {}
    for case in P.CASES:
        blob = P.pack(case)
        assert np.array_equal(blob, P.pack(case)), (case, "two packs of one case differ")
        out[f"{case}/size"] = np.int64(blob.size)
        out[f"{case}/crc"] = P.page_crcs(blob)
        out[f"{case}/sha"] = np.frombuffer(hashlib.sha256(blob.tobytes()).digest(), np.uint8)
        clean = P.twin(case)
        if clean is None:
            blobs[case] = blob
            continue
        plant = case.split("/")[2]
        assert blob.size == blobs[clean].size
        assert not np.array_equal(out[f"{case}/crc"], out[f"{clean}/crc"]), (case, "page checksums equal the clean twin's")
        if plant in P.FLAG_FROM_END:
            assert P.flag_word(plant, blobs[clean]) == 0, (case, "the flag is set in the clean twin")
            assert P.flag_word(plant, blob) != 0, (case, "the plant did not reach its flag")
        else:                                               # fp32 sections and fp16 streams: a NaN half-word pattern at
            n0, n1 = f16_nans(blobs[clean]), f16_nans(blob)  # an odd half of an fp32 value counts in both blobs alike
            assert n1 > n0, (case, "no NaN was packed", n0, n1)
        print(f"{case}: {blob.size} bytes, flag/NaN check passed")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "pointnet_blobs.npz")
    G.save(path, out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(P.CASES)} cases, {len(out)} arrays")


if __name__ == "__main__":
    main()
