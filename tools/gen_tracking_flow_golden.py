"""Generate ``tests/golden/tracking_flow.npz`` from the reference's own ``FlowShiftTracker`` (through ``oracle.ref_harness``, where the reference tree is available).

OpenCV is not installed, so a stub ``cv2`` module is registered before the reference's tracker is imported: ``calcOpticalFlowPyrLK`` calls this project's
``sleap_nn_amd.tracking.flow.pyr_lk`` (a STAND-IN, not an OpenCV pin: the optical flow of every golden number here is the stand-in's), the two
``TERM_CRITERIA_*`` constants have OpenCV's values, and ``cvtColor`` / ``resize`` raise.  The sleap-io stand-ins come from ``tools/gen_tracking_golden.py``.
Everything else -- candidates, shifted instances, features, scores, reductions, matching, queues, the pre-cull -- is the reference's own code, unmodified.  A golden
made with the real library can replace the file without touching code.

The frames and poses are regenerated from seeds by ``tests/_flow.py``: the file holds results and parameters only.  Recorded per case and frame: ids, tracking
scores, ``get_scores``' matrix and the shifted keypoints of every candidate (in the order the reference builds them).  A case is REFUSED when its ids change with
every shifted point moved by up to 0.02 px (the tolerance the kernels are held to against ``pyr_lk``), or with the scores perturbed by ``1 +- 1e-9``.  The ``close``
case is asserted to give DIFFERENT ids with ``use_flow=False``: without it the golden could not tell a flow tracker from the plain one.  The note also records the
largest error ``pyr_lk`` shows against known translations on the seeded textures (``measure_stand_in``), the basis of the CPU test's bar.

    python tools/gen_tracking_flow_golden.py
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden", "tracking_flow.npz")

OF = {"of_window_size": 21, "of_max_levels": 3}
CASES = {
    "fixed_hungarian": {"kw": {}, "seq": "plain"},
    "fixed_greedy": {"kw": {"track_matching_method": "greedy", "scoring_reduction": "max"}, "seq": "plain"},
    "local_queues": {"kw": {"candidates_method": "local_queues", "max_tracks": 4}, "seq": "plain"},
    "lost_points": {"kw": {"window_size": 3}, "seq": "lost"},
    "min_points": {"kw": {"min_match_points": 2, "min_new_track_points": 1}, "seq": "sparse"},
    "precull": {"kw": {"tracking_target_instance_count": 3, "tracking_pre_cull_to_target": 1, "tracking_pre_cull_iou_threshold": 0}, "seq": "surplus"},
    "close_euclid": {"kw": {"features": "centroids", "scoring_method": "euclidean_dist", "track_matching_method": "greedy", "window_size": 2, "of_window_size": 15}, "seq": "close"},
}
TRANSLATIONS = [(0.4, -0.3), (3.3, 2.1), (-7.6, 5.2), (14.0, -9.5), (1.0, 0.0), (-0.7, 11.2)]


def measure_stand_in():
    """The largest error of ``pyr_lk`` (defaults) against known translations: 96 x 128 textures of seeds 1 .., 40 interior points each (28 px from the border)."""
    from sleap_nn_amd.tracking.flow import pyr_lk
    from tests import _flow as TF

    worst = 0.0
    for seed, sh in enumerate(TRANSLATIONS, start=1):
        a, b = TF.texture(seed, 96, 128), TF.texture(seed, 96, 128, sh)
        pts = TF.interior_points(seed + 50, 40, 96, 128, 28)
        got, status = pyr_lk(a, b, pts)
        assert status.all()
        worst = max(worst, float(np.linalg.norm(got - pts - np.float32(sh), axis=1).max()))
    return worst


def install(noise):
    """The stub ``cv2`` and the reference's ``Tracker``.  ``noise["g"]``: None, or a Generator whose draws (up to 0.02 px per point) are added to the flow."""
    from sleap_nn_amd.tracking.flow import pyr_lk

    cv2 = types.ModuleType("cv2")
    cv2.TERM_CRITERIA_COUNT, cv2.TERM_CRITERIA_EPS = 1, 2

    def calc(ref_img, new_img, pts, next_pts, winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01)):
        assert next_pts is None and winSize[0] == winSize[1] and criteria[0] == 3
        shifted, status = pyr_lk(ref_img, new_img, pts, win=int(winSize[0]), max_level=int(maxLevel), max_iter=int(criteria[1]), eps=float(criteria[2]))
        if noise["g"] is not None:
            ang, r = noise["g"].uniform(0, 2 * np.pi, len(shifted)), noise["g"].uniform(0, 0.02, len(shifted))
            shifted = shifted + np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1).astype(np.float32)
        return shifted, status.reshape(-1, 1), np.zeros((len(shifted), 1), np.float32)

    def refuse(*_a, **_k):
        raise NotImplementedError("the cv2 stub has no colour conversion or resize")

    cv2.calcOpticalFlowPyrLK, cv2.cvtColor, cv2.resize = calc, refuse, refuse
    sys.modules["cv2"] = cv2
    import gen_tracking_golden as G

    return G, G.install()


def run_reference(Tracker, kw, frames, objs_per_frame, perturb=None):
    seen = {}
    base = Tracker.from_config(**kw)

    class Spy(type(base)):  # (FlowShiftTracker with use_flow, the plain Tracker without)
        def get_scores(self, cur, cand):
            s = type(base).get_scores(self, cur, cand)
            seen["scores"] = np.array(s, dtype=np.float64)
            moved = [x for t in self.candidate.current_tracks for x in cand[t] if x.shifted_keypoints is not None]
            seen["shifted"] = [np.asarray(x.shifted_keypoints, dtype=np.float64) for x in moved]
            seen["lost"] = sum(int((np.isnan(x.shifted_keypoints).any(axis=1) & ~np.isnan(x.src_predicted_instance.numpy()).any(axis=1)).sum()) for x in moved)  # nodes the flow lost
            return perturb(s) if perturb is not None else s

    tr = Spy.from_config(**kw) if not kw.get("use_flow") else None
    if tr is None:  # from_config names FlowShiftTracker itself: build the spy from the instance's fields
        import attrs

        tr = Spy(**{getattr(f, "alias", f.name): getattr(base, f.name) for f in attrs.fields(type(base)) if f.init})
    out = []
    for t, objs in enumerate(objs_per_frame):
        seen.clear()
        for o in objs:
            o.track, o.tracking_score = None, None
        tr.track(list(objs), frame_idx=t, image=frames[t])
        ids = np.array([-1 if o.track is None else int(o.track.name.split("_")[1]) for o in objs], dtype=np.int64)
        tsc = np.array([np.nan if o.track is None or o.tracking_score is None else float(o.tracking_score) for o in objs], dtype=np.float64)
        out.append((ids, tsc, seen.get("scores"), seen.get("shifted"), seen.get("lost", 0)))
    return out


def same_ids(a, b):
    return all(np.array_equal(x[0], y[0]) for x, y in zip(a, b))


def main():
    from tests import _flow as TF

    noise = {"g": None}
    G, Tracker = install(noise)
    worst = measure_stand_in()
    print(f"pyr_lk against known translations: largest error {worst:.4f} px")
    arrs, seeds, lost = {}, {}, {}
    for name, case in CASES.items():
        kw = dict(OF, use_flow=True, **case["kw"])
        for seed in range(500, 600):
            frames, seq = TF.flow_sequence(seed, case["seq"])
            if min(len(p) for p, _s in seq) == 0:
                continue
            make = lambda: [[G.PredictedInstance(p, s) for p, s in zip(pts, sc)] for pts, sc in seq]
            noise["g"] = None
            base = run_reference(Tracker, kw, frames, make())
            ok = all(same_ids(base, run_reference(Tracker, kw, frames, make(), perturb=f)) for f in (lambda s: s * (1 + 1e-9), lambda s: s * (1 - 1e-9)))
            for k in range(3):
                noise["g"] = np.random.default_rng(1000 + k)
                ok = ok and same_ids(base, run_reference(Tracker, kw, frames, make()))
            noise["g"] = None
            n_lost = sum(r[4] for r in base)
            n_ids = len({int(i) for r in base for i in r[0] if i >= 0})
            if case["seq"] == "lost":
                ok = ok and n_lost > 0
            if case["seq"] == "sparse":  # instances at or below the floors must occur
                ok = ok and any((~np.isnan(p).any(axis=1)).sum() <= 2 for pts, _s in seq for p in pts)
            if case["seq"] == "surplus":
                ok = ok and max(len(p) for p, _s in seq) > 3
            if case["seq"] == "close":
                plain = run_reference(Tracker, {k: v for k, v in kw.items() if not k.startswith("of_") and k != "use_flow"}, frames, make())
                assert not same_ids(base, plain), "the close case must tell the flow tracker from the plain one"
                assert n_ids == 2, "the flow tracker must keep the two identities"
            if not ok:
                continue
            seeds[name] = seed
            lost[name] = n_lost
            for t, (ids, tsc, sc, sh, _n) in enumerate(base):
                arrs[f"{name}/ids/{t}"], arrs[f"{name}/tracking_scores/{t}"] = ids, tsc
                if sc is not None:
                    arrs[f"{name}/scores/{t}"] = sc
                if sh:
                    arrs[f"{name}/shifted/{t}"] = np.stack(sh)
            print(f"{name}: sequence {case['seq']} seed {seed}, {sum(len(p) for p, _s in seq)} instances, {n_ids} ids, {n_lost} nodes lost by the flow")
            break
        else:
            raise AssertionError(f"no seed gave a stable {name} case")
    arrs["params"] = np.array(json.dumps({"cases": CASES, "of": OF, "seeds": seeds, "lost_nodes": lost, "stand_in_max_error_px": worst, "translations": TRANSLATIONS,
                                          "note": "the optical flow is the stand-in sleap_nn_amd.tracking.flow.pyr_lk handed to the reference as cv2.calcOpticalFlowPyrLK, "
                                                  "not OpenCV's; sleap-io objects are the stand-ins of tools/gen_tracking_golden.py; frames and poses come from "
                                                  "tests/_flow.py by seed"}))
    np.savez_compressed(GOLD, **arrs)
    print(f"wrote {GOLD} ({os.path.getsize(GOLD) / 1024:.0f} KiB, {len(arrs)} arrays)")


if __name__ == "__main__":
    main()
