"""Generates tests/golden/object_stage_golden.npz: the reference's object stage (SLAM/multiprocess/quadrics.py, driven as
SLAM/multiprocess/mapper.py:155-163 drives it) over the scripted sequences of tests/object_scenes.py (ALL: the scenes and the wide one), recorded as data only.

The reference module imports on a CPU with two stub modules (cv2; plyfile with PlyData / PlyElement) and MPLBACKEND=Agg.  Its one
non-reproducible input is random.randint in detections_filter: the module's `random` attribute is replaced by a shim that serves the key
rule of tests/object_oracle.py (and answers generate_random_color's calls).  The shim is told which input detection each accepted one is
by a first, dry pass of the filter (get_2dim_quarics numbers the detections in det["node_id"]).

Recorded after every frame, under "<sequence>/<frame>/<name>": every object's category, id, axes, R, centre, the observation count and
the observations (bbox and K @ Rt) of each; every detection's fate and row (the row its det["node_id"] names in the map as it stood
before remove_outlier, followed through remove_outlier's pops: -1 when that object went); the two depth numbers; has_new_object.

    python tests/golden/make_object_stage_golden.py [reference root]       (tests/test_object_oracle.py calls record() for its live run)
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import object_oracle as O  # noqa: E402
import object_scenes as S  # noqa: E402

OUT = os.path.join(HERE, "object_stage_golden.npz")


class _KeyRuleRandom:
    """random.randint for the reference: inside detections_filter the 60 calls of an accepted detection are (u, v) of samples 0..29."""

    def __init__(self):
        self.plan = None

    def arm(self, seed, frame_id, accepted):
        self.plan, self.calls = (seed, frame_id, list(accepted)), 0

    def disarm(self):
        self.plan = None

    def randint(self, a, b):
        if self.plan is None or self.calls >= 2 * O.N_SAMPLES * len(self.plan[2]):
            return a
        seed, frame_id, accepted = self.plan
        d, s, which = accepted[self.calls // (2 * O.N_SAMPLES)], self.calls % (2 * O.N_SAMPLES) // 2, self.calls % 2
        self.calls += 1
        return a + O.object_key(seed, 8 + which, frame_id, d * 32 + s) % (b - a + 1)


def load_reference(root):
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    if "plyfile" not in sys.modules:
        ply = types.ModuleType("plyfile")
        ply.PlyData = ply.PlyElement = object
        sys.modules["plyfile"] = ply
    spec = importlib.util.spec_from_file_location("dqo_reference_quadrics", os.path.join(root, "SLAM", "multiprocess", "quadrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(root):
    """{key: array} of every sequence (the overflow sequence too: the reference has no capacities)."""
    import torch
    Q = load_reference(root)
    shim = _KeyRuleRandom()
    Q.random = shim
    out = {}
    for name, make in S.ALL.items():
        seq = make()
        Q.factory_id = 0
        Map_global = None
        if seq["preset"]:  # rows as an earlier Object_Optimize_only would have left them (quadrics.py:2293-2295)
            Map_global = []
            for r in seq["preset"]:
                obj = Q.Object(int(r["cat"]), [float(x) for x in r["bbox"]], None, 0.9, [1.0, 0.1], S.K.astype(np.float64),
                               r["Rt"].astype(np.float64), 0, False)
                obj.ellipsoid_ = Q.Ellipsoid(r["axes"].astype(np.float64), r["R"].astype(np.float64), r["center"].astype(np.float64))
                Map_global.append(obj)
        for fi, f in enumerate(seq["frames"]):
            d = f["dets"]
            info = dict(detections=[dict(ellipse=[float(x) for x in d["ellipse"][i]], category_id=int(d["cat"][i]),
                                         bbox=[float(x) for x in d["bbox"][i]], detection_score=float(d["score"][i]), color=[0, 0, 0])
                                    for i in range(len(d["cat"]))])
            dets = Q.get_2dim_quarics(info)
            K, Rt = f["K"].astype(np.float64), f["Rt"].astype(np.float64)
            depth = torch.from_numpy(f["depth"])
            # mapper.py:155-163
            shim.disarm()
            dry, _ = Q.detections_filter(dets, depth, S.W, S.H)
            accepted = [x["node_id"] for x in dry]
            shim.arm(seq["seed"], f["frame_id"], accepted)
            cur, cur_depth = Q.detections_filter(dets, depth, S.W, S.H)
            shim.disarm()
            first_id = Q.factory_id
            if Map_global is None:
                Map_global = Q.ObjectsInitialization(cur, cur_depth, Rt, K)
                has_new, before, n_before = True, list(Map_global), 0
            else:
                n_before = len(Map_global)
                proj = Q.Occlusions_Check(Map_global, K, Rt, S.W, S.H, f["frame_id"])
                has_new, _ = Q.MatchObject(Map_global, cur, cur_depth, proj, f["frame_id"], torch.zeros(S.H, S.W, 3), K, Rt)
                before = list(Map_global)
                Map_global = Q.remove_outlier(Map_global, K, Rt, False)
            M = len(dets)
            fate, row, dd = np.full(M, O.FATE_DROPPED, np.int32), np.full(M, -1, np.int32), np.zeros((M, 2))
            for k, det in enumerate(cur):
                i = accepted[k]
                dd[i] = cur_depth[k]
                if not det["is_validate"]:
                    fate[i] = O.FATE_INVALID
                elif det["obj"] is None:
                    fate[i] = O.FATE_UNMATCHED
                else:
                    fresh = det["obj"].id_ >= first_id
                    fate[i] = O.FATE_MATCHED if not fresh else (O.FATE_NEW if det["node_id"] >= n_before else O.FATE_REPLACED)
                    row[i] = next((j for j, o in enumerate(Map_global) if o is before[det["node_id"]]), -1)
            key = f"{name}/{fi}/"
            out[key + "fate"], out[key + "row"], out[key + "depth"] = fate, row, dd
            out[key + "has_new_object"] = np.array(int(bool(has_new)), np.int32)
            out[key + "cat"] = np.array([o.category_id_ for o in Map_global], np.int32)
            out[key + "uid"] = np.array([o.id_ for o in Map_global], np.int32)
            out[key + "axes"] = np.array([o.ellipsoid_.axes_ for o in Map_global], np.float64).reshape(-1, 3)
            out[key + "R"] = np.array([o.ellipsoid_.R_ for o in Map_global], np.float64).reshape(-1, 9)
            out[key + "center"] = np.array([o.ellipsoid_.center_ for o in Map_global], np.float64).reshape(-1, 3)
            out[key + "nviews"] = np.array([len(o.bboxes_) for o in Map_global], np.int32)
            out[key + "view_bbox"] = np.array([b for o in Map_global for b in o.bboxes_], np.float64).reshape(-1, 4)
            out[key + "view_P34"] = np.array([K @ r for o in Map_global for r in o.Rts_], np.float64).reshape(-1, 12)
    return out


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DQO_REFERENCE_ROOT", "")
    if not os.path.isdir(root):
        sys.exit("the reference tree is needed to regenerate the golden: pass its root")
    data = record(root)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {len(data)} arrays, {os.path.getsize(OUT)} bytes")
