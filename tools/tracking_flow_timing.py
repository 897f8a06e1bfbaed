"""Timing of the flow-shift tracker's flow stage (sleap_nn_amd/tracking/flow.py, csrc/flow_kernels.hip).

The case: 1024 x 1024 uint8 frames, window 5, 4 instances x 15 nodes per frame, ``win`` 21, 4 pyramid levels (``max_level`` 3), batches of 4 frames.  Reported,
each as the median of repeated loops with the spread (min / max) next to it:

* ``ph_flow_pyramid`` of a batch (device events around the launches of its three levels);
* ``ph_flow_track`` of a batch: all (frame, lag <= 5, instance) flows the two pyramided batches hold, 19 jobs of 60 points, one launch (device events);
* the stage end to end: ``Tracker.track_outputs`` of a batch with device frames, wall clock with a synchronisation, per frame;
* the same tracker on the host path (``pyr_lk`` on the box's host cores), in the same process, per frame.

The frames are one seeded texture moved by a few pixels per frame; the poses ride on it.  No speed-up is promised and no test depends on a time.

    python tools/tracking_flow_timing.py [--size 1024] [--iters 20] [--out profiles/tracking_flow_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _flow as TF  # noqa: E402


def stats(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "n": len(times)}


def event_ms(fn, iters):
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return stats(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_flow_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tracking_flow_timing needs the GPU")
    from sleap_nn_amd.inference.outputs import Outputs
    from sleap_nn_amd.tracking import Tracker
    from sleap_nn_amd.tracking import flow as F

    S, B, window, I, N, win, max_level = args.size, 4, 5, 4, 15, 21, 3
    n_frames = 3 * B
    shifts = np.cumsum(np.tile([[3.0, 1.5]], (n_frames, 1)), axis=0)
    frames = TF.scene_frames(77, S, S, shifts)
    g = np.random.default_rng(3)
    base = g.uniform(0.2 * S, 0.7 * S, (I, 1, 2)) + g.normal(0, 0.03 * S, (I, N, 2))
    poses = np.stack([base + shifts[t] for t in range(n_frames)])
    dev_frames = torch.from_numpy(frames).cuda()

    def batch(t0):
        return Outputs(pred_keypoints=torch.from_numpy(poses[t0 : t0 + B]), instance_scores=torch.ones(B, I, dtype=torch.float64), frame_indices=torch.arange(t0, t0 + B))

    res = {"case": {"frame": [S, S], "batch": B, "window_size": window, "instances": I, "nodes": N, "of_window_size": win, "levels": max_level + 1},
           "device": torch.cuda.get_device_name(0), "derivative_layout": "recomputed in ph_flow_track from the (win + 3)^2 patch; derivative planes were not tried"}
    # the launches
    pyr = F.pyramid_device(dev_frames[:B], win, max_level)
    torch.cuda.synchronize()
    res["pyramid_batch"] = event_ms(lambda: F.pyramid_device(dev_frames[:B], win, max_level), args.iters)
    pyr2 = F.pyramid_device(dev_frames[B : 2 * B], win, max_level)
    both = pyr + pyr2
    jobs = [(both[B + b - k], both[B + b], poses[B + b - k].reshape(-1, 2).astype(np.float32)) for b in range(B) for k in range(1, window + 1) if B + b - k >= 0]
    F.track_device(jobs, win, max_level)
    import ctypes as C

    from sleap_nn_amd import _lib as L

    # the launch alone: descriptors and points uploaded once, events around ph_flow_track
    descs = (F.JobDesc * len(jobs))()
    pts, begin = [], 0
    for d, (r, c, p) in zip(descs, jobs):
        for l in range(len(r)):
            d.ref[l], d.cur[l] = r[l].data_ptr(), c[l].data_ptr()
        d.pt_begin, d.pt_end = begin, begin + len(p)
        begin += len(p)
        pts.append(p)
    jobs_dev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
    pts_dev = torch.from_numpy(np.concatenate(pts)).cuda()
    rec = torch.empty(begin * 9, dtype=torch.uint8, device="cuda")
    launch = lambda: L.check(L.lib().ph_flow_track(C.c_void_p(jobs_dev.data_ptr()), len(jobs), I * N, C.c_void_p(pts_dev.data_ptr()), begin, S, S, win, max_level, 30, 0.01,
                                                   C.c_void_p(rec.data_ptr()), C.c_void_p(rec.data_ptr() + begin * 8), L.current_stream_ptr()))
    launch()
    torch.cuda.synchronize()
    res["track_batch"] = dict(event_ms(launch, args.iters), jobs=len(jobs), points=begin)
    found = int(rec[begin * 8 :].sum().item())
    res["track_batch"]["points_found"] = found

    # the stage end to end, device and host, same tracker configuration
    def stage(device, iters):
        times = []
        for _ in range(iters):
            tr = Tracker.from_config(use_flow=True, allow_flow=True, window_size=window, of_window_size=win, of_max_levels=max_level)
            tr.flow_device = device
            src = dev_frames if device else frames
            tr.track_outputs(batch(0), images=src[:B])  # fills the ring: the timed batch reaches back over all five lags
            tr.track_outputs(batch(B), images=src[B : 2 * B])
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = tr.track_outputs(batch(2 * B), images=src[2 * B : 3 * B])
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3 / B)
            ids = out.instance_track_ids
        return stats(times), ids

    stage(True, 2)
    res["stage_per_frame_device"], ids_dev = stage(True, args.iters)
    res["stage_per_frame_host"], ids_host = stage(False, args.host_iters)
    res["same_ids"] = bool(torch.equal(ids_dev, ids_host))
    res["host_cores"] = os.cpu_count()
    res["torch_threads"] = torch.get_num_threads()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
