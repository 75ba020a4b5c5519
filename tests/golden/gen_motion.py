#!/usr/bin/env python3
"""Generate motion.npz from the REAL reference (jacky121298/3DAL_PyTorch): tools/trackGT.py's main() on the seeded train
and val work dirs of tests/motion_ref.write_work_dirs, then tools/motionState.py's main() (scikit-learn's
SVC(kernel='linear')) on the same dirs. Stored: recorded results only — the features and labels, the kept ids, the GT
static flags, the id lists of every output pickle, the fitted model, its decisions and predictions, the printed score.
The inputs are rebuilt from the seeds.

Checked here, so that a float64 last bit cannot flip a recorded flag: no GT object has its end-to-end distance or its
largest speed within 1e-6 of 1; at most 1 % of the val rows have |decision| <= 2e-3.

Run where the reference, scikit-learn and tqdm exist (DAL3_REFERENCE, default /root/reference):
    python tests/golden/gen_motion.py
"""
import contextlib
import io
import os
import pickle
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import motion_ref  # noqa: E402

REF = os.environ.get("DAL3_REFERENCE", "/root/reference")


def run_main(module, argv):
    old = sys.argv
    sys.argv = argv
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            module.main()
    finally:
        sys.argv = old
    return buf.getvalue()


def load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def main():
    sys.path.insert(0, os.path.join(REF, "tools"))
    import motionState
    import trackGT
    from sklearn.svm import SVC
    rec = {}
    with tempfile.TemporaryDirectory() as tmp:
        train, val, _, _ = motion_ref.write_work_dirs(tmp)
        for name, wd in (("train", train), ("val", val)):
            run_main(trackGT, ["trackGT.py", "--infos", os.path.join(wd, "infos.pkl"), "--result", os.path.join(wd, "trackGT.pkl")])
            gt = load(os.path.join(wd, "trackGT.pkl"))
            dist = np.array([np.linalg.norm(np.array(o["box"])[0, :3] - np.array(o["box"])[-1, :3]) for o in gt.values()])
            vmax = np.array([np.max(o["vel"]) for o in gt.values()], np.float64)
            assert np.abs(dist - 1).min() > 1e-6 and np.abs(vmax - 1).min() > 1e-6, "a GT object on the static rule's edge"
            rec[f"gt_{name}_names"] = np.array(list(gt.keys()))
            rec[f"gt_{name}_static"] = np.array([o["static"] for o in gt.values()], np.int64)
            rec[f"gt_{name}_dist"], rec[f"gt_{name}_max_vel"] = dist, vmax
            rec[f"gt_{name}_first_box"] = np.array([o["box"][0] for o in gt.values()])
            rec[f"gt_{name}_len"] = np.array([len(o["box"]) for o in gt.values()], np.int64)
        out = run_main(motionState, ["motionState.py", "--track_train", train, "--track_val", val])
        rec["n_train"] = np.array(int(re.search(r"Number of train: (\d+)", out).group(1)))
        rec["n_val"] = np.array(int(re.search(r"Number of val: (\d+)", out).group(1)))
        rec["score_text"] = np.array(re.search(r"Score on test set: (\S+)", out).group(1))
        rec["printed"] = np.array(out)
        for kind in ("trackStatic", "trackDynamic"):
            parts = [load(os.path.join(train, f"{kind}_{i}.pkl")) for i in range(motion_ref.SPLIT)]
            rec[f"train_{kind}_ids"] = np.array([k for p in parts for k in p.keys()])
            rec[f"train_{kind}_counts"] = np.array([len(p) for p in parts], np.int64)
            rec[f"val_{kind}_ids"] = np.array(list(load(os.path.join(val, f"{kind}.pkl")).keys()))
        # the features and the model: motionState's own trackFeature on the same files, and the same SVC call
        tr = {}
        for i in range(motion_ref.SPLIT):
            tr = dict(list(tr.items()) + list(load(os.path.join(train, f"track_{i}.pkl")).items()))
        trainX, trainY, static, dynamic = motionState.trackFeature(tr, load(os.path.join(train, "trackGT.pkl")), training=True)
        valX, valY, kept = motionState.trackFeature(load(os.path.join(val, "track.pkl")), load(os.path.join(val, "trackGT.pkl")))
    assert list(static.keys()) == list(rec["train_trackStatic_ids"]) and list(dynamic.keys()) == list(rec["train_trackDynamic_ids"])
    clf = SVC(kernel="linear").fit(trainX, trainY)
    y_pred = clf.predict(valX)
    assert str(clf.score(valX, valY)) == str(rec["score_text"])
    ids = list(kept.keys())
    assert [i for i, p in zip(ids, y_pred) if p == 1] == list(rec["val_trackStatic_ids"])
    dec = clf.decision_function(valX)
    assert (np.abs(dec) <= 2e-3).mean() <= 0.01, "too many val rows inside the solver's own tolerance"
    assert list(clf.classes_) == [0, 1]
    rec.update(trainX=trainX, trainY=trainY, valX=valX, valY=valY, val_keep_ids=np.array(ids),
               train_keep_ids=np.array([k for k in tr if k in static or k in dynamic]),
               coef=clf.coef_[0], intercept=clf.intercept_, decision=dec, y_pred=y_pred.astype(np.int64))
    for k, v in rec.items():
        print(k, v.shape, v.dtype)
    print("train", trainX.shape, "static", int(trainY.sum()), "val", valX.shape, "score", rec["score_text"],
          "in band", int((np.abs(dec) <= 2e-3).sum()), "model", clf.coef_, clf.intercept_)
    np.savez_compressed(os.path.join(HERE, "motion.npz"), **rec)


if __name__ == "__main__":
    main()
