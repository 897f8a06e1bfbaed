"""bench.py's multi-rank code path, rehearsed on the one GPU of the test box: the self-launch (a child torchrun), the frame sharding
of weak and strong scaling, the max-over-ranks timing and the rank-0 JSON line.  All ranks share cuda:0 and synchronise over gloo
(RCCL refuses two ranks on one device), so the numbers mean nothing -- the structure of the line is what is checked."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    """(contract line, full record): stdout must END with exactly one strict-JSON line of at most 4 KB from rank 0; the legs file holds everything else."""
    import tempfile

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    with tempfile.TemporaryDirectory() as tmp:
        legs = os.path.join(tmp, "legs.json")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args, "--legs-file", legs], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
        assert len(lines) == 1 and r.stdout.rstrip().endswith(lines[0]), r.stdout[-1000:]  # exactly one line, from rank 0, and the last thing on stdout
        assert len(lines[0].encode()) < 4096
        return json.loads(lines[0]), json.load(open(legs))


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_two_ranks_default_strong_with_weak_beside_it_and_three_ranks_strong_rehearsal():
    # N > 1 with no --scaling flag: `value` is BASELINE cfg3 as written (global batch split over the ranks), the weak figure rides along
    d, full = _run("--gpus", "2", "--rehearse-on-one-gpu", "--full", "--steps", "3", "--warmup", "1", "--batch", "4", "--global-batch", "8", "--no-alt-precisions", "--no-h2d-leg")
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["steps"] == 3 and d["warmup"] == 1
    assert d["config"]["frames_per_gpu_per_step"] == 4 and d["config"]["global_batch"] == 8
    assert d["value"] > 0 and abs(d["value"] - 8 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]  # whole-job frames / max-over-ranks time
    w = full["weak_scaling"]
    assert w["frames_per_gpu_per_step"] == 4 and w["global_batch"] == 8 and w["value"] > 0 and d["legs_summary"]["weak_scaling_frames_per_s"] == pytest.approx(w["value"], rel=1e-3)
    assert "cpu_baseline" not in d and "train_cfg3" not in full and "REHEARSAL" in d["data"]  # the CPU leg and the extra legs belong to N = 1
    assert d["config"]["rccl_ranks_seen"] == 2 and d["config"]["frames_per_step_by_rank"] == [4, 4]  # every rank joined the collective and took its contiguous chunk of the global batch
    ht = full["config"]["host_threads"]
    assert ht["ranks"] == 2 and ht["per_rank"] == 2 and ht["fits"] == (4 <= ht["cores_visible"])
    # the driver's SCALE run puts 8 ranks on one host: enqueue thread + grouping worker per rank must fit its cores (16 on the 8-GPU box: 8 x 2)
    assert 2 * 8 <= max(ht["cores_visible"], 16)
    assert d["roofline"]["kernel"].startswith("conv3x3_wino") and 0 < d["roofline"]["frac"] < 1
    d, full = _run("--gpus", "2", "--rehearse-on-one-gpu", "--full", "--steps", "2", "--warmup", "1", "--batch", "4", "--scaling", "weak", "--no-alt-precisions", "--no-h2d-leg")
    assert d["scaling"] == "weak" and d["config"]["global_batch"] == 8 and "weak_scaling" not in full
    d, full = _run("--gpus", "3", "--rehearse-on-one-gpu", "--full", "--steps", "2", "--warmup", "1", "--scaling", "strong", "--global-batch", "8", "--no-alt-precisions", "--no-h2d-leg")
    assert d["n_gpus"] == 3 and d["scaling"] == "strong" and d["config"]["global_batch"] == 8
    assert d["config"]["frames_per_gpu_per_step"] in (2, 3)  # rank 0's contiguous chunk of 8 frames over 3 ranks


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_four_rank_strong_scaling_rehearsal_every_rank_equals_the_single_rank_result():
    """the per-rank batch of the 8-GPU strong-scaling run (4 frames per rank and step, THREE copies of the network on HIP streams of their own per
    rank) with as many ranks as one GPU box admits (six processes may use the card together -- the box's process guard --: the test runner, the launcher and four ranks; the
    driver's SCALE run has eight).  Every rank's
    head outputs -- through every one of its lanes -- must be the bits rank 0 computes for the same frames with one copy, kernel by kernel; the grouped keypoints the same
    on every rank; and the line reports what each rank's enqueue thread waited for its grouping worker, the first thing 8 x 3 lanes on one host's cores would stretch."""
    d, full = _run("--gpus", "4", "--rehearse-on-one-gpu", "--full", "--steps", "4", "--warmup", "2", "--scaling", "strong", "--global-batch", "16", "--no-alt-precisions", "--no-h2d-leg")
    assert d["n_gpus"] == 4 and d["config"]["frames_per_step_by_rank"] == [4] * 4 and d["config"]["rccl_ranks_seen"] == 4
    sc = full["config"]["shard_check"]
    assert sc["result"] == "equal", sc["mismatches"]
    assert sc["ranks"] == 4 and sc["lanes_per_rank"] == [3] * 4
    waits = sc["host_stage_wait_ms_per_step_by_rank"]
    assert len(waits) == 4 and all(w >= 0 for w in waits)
    assert d["config"]["shard_check"] == "equal" and d["config"]["host_stage_wait_ms_by_rank"] == waits
    print("host-stage wait per step and rank (ms):", waits, "step", d["ms_per_step"])


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_two_ranks_training_rehearsal():
    """--mode train with two ranks: identical initial arenas, disjoint shards, the two-bucket gradient all-reduce overlapped with the
    backward (gloo here), Adam on every rank -- the loss must be finite and move, the line must say what it measured."""
    d, full = _run("--gpus", "2", "--rehearse-on-one-gpu", "--mode", "train", "--steps", "3", "--warmup", "1", "--batch", "2")
    assert d["n_gpus"] == 2 and full["config"]["samples_per_gpu_per_step"] == 2 and d["config"]["global_batch"] == 4
    first, last = full["loss_first_last"]
    assert first > 0 and last > 0 and first == first and last == last and last != first
    assert full["allreduce"]["bucket_split"] is not None and full["allreduce"]["arena_mb"] > 30  # 7.8 M parameters in one flat arena
    assert "REHEARSAL" in d["data"] and 0 < d["roofline"]["frac"] < 1


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_default_single_gpu_line_with_every_leg():
    """`python bench.py --full` (fewer steps): every leg runs, the line carries the contract fields + roofline + cpu_baseline and stays under 4 KB."""
    d, full = _run("--full", "--steps", "6", "--warmup", "3", "--leg-steps", "2")
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["scaling"] == "weak" and d["dtype"] == "f32" and d["config"]["workload"].startswith("cfg3")
    assert d["value"] == pytest.approx(32 * 6 / (d["ms_per_step"] * 6e-3), rel=1e-6) and d["vs_baseline"] is None
    r, c = d["roofline"], d["cpu_baseline"]
    assert r["bound"] == "mfma" and r["kernel"] == "conv3x3_wino4_kernel" and 0.3 < r["frac"] < 1 and r["traffic"] and 0.3 < r["conv_stack_frac"] < 1
    assert c["kind"] == "port" and c["value"] > 0 and c["parity_on_this_sample"]["peak_indices_equal"] and c["parity_on_this_sample"]["grouping_equal"]
    for leg in ("train_cfg3", "train_cfg4", "infer_cfg4", "infer_cfg1", "infer_cfg2", "infer_cfg5", "published_workload", "alt_precisions", "strong_scaling_shards", "roofline_postprocess"):
        assert leg in full, leg
    s = d["legs_summary"]
    assert s["published_workload"]["end_to_end_frames_per_s"] > 0 and s["infer_cfg5"]["value"] > 0 and s["one_gpu_shard_two_streams_frames_per_s"]["4_frames_per_rank"] > 0


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_plain_line_times_only_the_headline_and_dumps_what_the_last_step_computed(tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W` without --full: the contract fields over exactly K timed steps and none of the legs; --dump-outputs writes the
    last step's outputs as float32 / float64 .npy files within 64 MB, and a second run with the same arguments writes the same arrays."""
    import numpy as np

    dumps = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        d, full = _run("--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", str(out))
        dumps.append({p.stem: np.load(p) for p in out.glob("*.npy")})
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["dtype"] == "f32" and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["metric"].startswith("frames/sec bottom-up UNet") and d["value"] == pytest.approx(32 * 5 / (d["ms_per_step"] * 5e-3), rel=1e-6)
    assert full["step_ms"]["n"] == 5 and len(full["step_ms_profiled_vs_replayed"]["by_step"]) == 5
    for k in ("roofline", "cpu_baseline", "h2d_inclusive", "legs_summary"):
        assert k not in d, k
    for k in ("roofline", "cpu_baseline", "h2d_inclusive", "alt_precisions", "strong_scaling_shards", "roofline_postprocess", "train_cfg3", "infer_cfg1", "infer_cfg5"):
        assert k not in full, k
    a, b = dumps
    assert set(a) == {"pred_keypoints", "pred_peak_values", "instance_scores", "MultiInstanceConfmapsHead", "PartAffinityFieldsHead", "head_frame_index"}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20 and all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["MultiInstanceConfmapsHead"].shape == (8, 13, 256, 256) and a["PartAffinityFieldsHead"].shape == (8, 24, 128, 128) and a["head_frame_index"].shape == (8,)
    assert a["pred_keypoints"].shape[0] == 32 and a["pred_keypoints"].shape[2:] == (13, 2) and (~np.isnan(a["instance_scores"])).sum() >= 5 * 32
    assert np.isfinite(a["MultiInstanceConfmapsHead"]).all() and np.abs(a["MultiInstanceConfmapsHead"]).max() > 0
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), k
    # ... and they are what the path computes, recomputed here independently of the bench: the heads of the sampled frames against a kernel-by-kernel forward
    # of the same seeded network over the same seeded batch (and the first of them against the CPU oracle), the keypoints against the layer's own
    # post-process of the same rendered heads
    from benchlegs.common import CFG3_BB, CFG3_HEADS, SIZE, rendered_heads
    from oracle import cpu_ref as O
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import BottomUpLayer
    from sleap_nn_amd.inference.ops.paf import PAFScorer
    from sleap_nn_amd.inference.preprocess_info import PreprocInfo

    dev = "cuda:0"
    model = Model("unet", CFG3_BB, CFG3_HEADS, "bottomup")
    model.init_xavier_(seed=1234, head_scale=0.05)  # bench.py's weights
    frames = torch.randint(0, 256, (32, 1, 1, SIZE, SIZE), dtype=torch.uint8, generator=torch.Generator().manual_seed(4321)).squeeze(1)  # bench.py's frames at N = 1
    idx = a["head_frame_index"].astype(np.int64)
    backend = HipBackend(model, dev)  # no graph: launch by launch
    heads = {k: v[torch.as_tensor(idx, device=dev)].cpu().numpy() for k, v in backend(frames.to(dev)).items()}
    ref = O.model_forward(model.state_dict(), CFG3_BB, CFG3_HEADS, "bottomup", frames[int(idx[0]):int(idx[0]) + 1])
    for k in ("MultiInstanceConfmapsHead", "PartAffinityFieldsHead"):
        scale = float(np.abs(heads[k]).max())
        assert scale > 0 and np.abs(a[k] - heads[k]).max() <= 1e-5 * scale, k
        err = float(np.abs(a[k][0] - ref[k][0].numpy()).max())
        assert err <= 1e-4 and err <= 1e-5 * scale, (k, err, scale)
    cms, pafs = rendered_heads(32, dev)
    layer = BottomUpLayer(backend, PAFScorer.from_config(CFG3_HEADS), 4, 8, max_stride=32)
    got = layer.postprocess({"MultiInstanceConfmapsHead": cms, "PartAffinityFieldsHead": pafs},
                            PreprocInfo(original_size=(SIZE, SIZE), processed_size=(SIZE, SIZE), eff_scale=torch.ones(32), output_stride=4))
    for k in ("pred_keypoints", "pred_peak_values", "instance_scores"):
        want = getattr(got, k).numpy()
        assert a[k].shape == want.shape and np.array_equal(np.isnan(a[k]), np.isnan(want)) and np.allclose(a[k], want, atol=1e-4, equal_nan=True), k
