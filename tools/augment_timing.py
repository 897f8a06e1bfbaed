"""Timing of the on-device training augmentation (sleap_nn_amd/data/augmentation.py, ph_augment).

1. The cfg3 batch (32 x 1 x 1024 x 1024 uint8) through an ``Augmenter`` configured like the fixture run directories
   (rotation +-180 deg, scale 0.9 - 1.1, both always on) plus flip and erase: the kernel alone (parameters drawn and
   uploaded once, device events around the launches) and the whole call (host draws + one H2D + launch), as GB/s over the
   2 B C H W bytes an augmentation has to move and as a share of the 8 TB/s HBM peak, with the tile path counts.
2. A cfg3 training step fed by ``augment -> generate_multiconfmaps / generate_pafs -> training_step`` against the same
   step on a fixed batch.

    python tools/augment_timing.py [--batch 32] [--train-batch 8] [--iters 50]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchlegs.common import CFG3_BB, CFG3_HEADS, SIZE  # noqa: E402
from sleap_nn_amd.data import augmentation as A  # noqa: E402
from sleap_nn_amd.data.targets import generate_multiconfmaps, generate_pafs  # noqa: E402

HBM_PEAK = 8.0e12
GEOMETRIC = dict(rotation_min=-180.0, rotation_max=180.0, flip_p=0.5, erase_p=0.5)


def events_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--train-batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_timing needs the GPU")
    dev = "cuda:0"
    B, S = args.batch, SIZE
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (B, 1, S, S), dtype=torch.uint8, generator=g).to(dev)
    kp = torch.from_numpy(np.random.RandomState(0).uniform(200, 800, (B, 2, 13, 2)).astype(np.float32)).to(dev)
    aug = A.Augmenter(None, GEOMETRIC, rng=np.random.RandomState(0))
    nbytes = 2 * img.numel()

    draws, seed = aug.draw(B, (S, S))
    params = A._pack(draws, S, S, aug.intensity, seed)
    cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    A._launch(img, kp, params, (), cnt)
    c = cnt.cpu().tolist()
    # the launch alone: ph_augment on prepared device buffers (the Python wrapper's allocations and pinned upload would
    # otherwise set the pace of the loop)
    import ctypes as C

    from sleap_nn_amd import _lib as L

    out, kout = torch.empty_like(img), torch.empty_like(kp)
    p_dev = torch.from_numpy(np.frombuffer(bytes(params), np.uint8).copy()).to(dev)
    stream = L.current_stream_ptr()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def launch():
        L.check(L.lib().ph_augment(P(img), P(out), 0, B, 1, S, S, P(kp), P(kout), 2, 13, P(p_dev), None, 0, None, stream))

    for _ in range(5):
        launch()
    k_ms = events_ms(launch, args.iters)
    for _ in range(3):
        aug(img, kp)
    call_ms = wall_ms(lambda: aug(img, kp), args.iters)
    print(f"augment {B}x1x{S}x{S} uint8 ({nbytes / 1e6:.1f} MB moved): launch {k_ms * 1e3:.1f} us = {nbytes / k_ms / 1e6:.0f} GB/s = "
          f"{nbytes / (k_ms * 1e-3) / HBM_PEAK:.2f} of 8 TB/s; whole call (draws + H2D + launch) {call_ms * 1e3:.1f} us")
    print(f"tiles per launch: copy {c[0]}, zero {c[1]}, LDS-staged {c[2]}, direct gather {c[3]}; samples warped {sum(d.warp for d in draws)}/{B}, "
          f"flipped {sum(d.flip for d in draws)}, erased {sum(d.erase is not None for d in draws)}")

    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.module import TrainingModule

    TB = args.train_batch
    m = Model("unet", CFG3_BB, CFG3_HEADS, "bottomup")
    m.init_xavier_(seed=1234, head_scale=0.05)
    tm = TrainingModule(m, dev, lr=1e-4)
    edges = [(i, i + 1) for i in range(12)]
    timg, tkp = img[:TB].contiguous(), kp[:TB].contiguous()

    def targets(p):
        return {"MultiInstanceConfmapsHead": generate_multiconfmaps(p, (S, S), sigma=2.5, output_stride=4),
                "PartAffinityFieldsHead": generate_pafs(p, (S, S), sigma=75.0, output_stride=8, edge_inds=edges)}

    fixed = {"image": timg, **targets(tkp)}

    def plain():
        tm.training_step(fixed)

    def augmented():
        a, p = aug(timg, tkp)
        tm.training_step({"image": a, **targets(p)})

    for _ in range(3):
        plain()
        augmented()
    n = max(5, args.iters // 10)
    t_plain, t_aug = wall_ms(plain, n), wall_ms(augmented, n)
    t_plain2 = wall_ms(plain, n)
    print(f"cfg3 train step B={TB}: fixed batch {t_plain:.2f} / {t_plain2:.2f} ms, augment + targets + step {t_aug:.2f} ms "
          f"(+{t_aug - min(t_plain, t_plain2):.2f} ms)")
    tm.close()


if __name__ == "__main__":
    main()
