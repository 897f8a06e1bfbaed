"""Shared by tests/test_tiled_seg_cpu.py and tests/test_gpu_tiled_seg.py: the recorded reference runs of tests/golden/tiled_segmentation.npz
(tools/gen_tiled_seg_golden.py), a backend that replays the recorded reference tile maps, and the comparison of ``pred_masks`` entries."""
import json

import numpy as np
import torch

from tests import _golden as G

KEYS = ("SegmentationHead", "InstanceCenterHead", "CenterOffsetHead")
CHANNELS = (1, 1, 2)
_Z = {}


def golden():
    if "z" not in _Z:
        _Z["z"] = G.load("tiled_segmentation.npz")
    return _Z["z"]


def case_names(kind):
    return json.loads(str(golden()[f"{kind}/names"]))


ALL_CASES = [("bu", n) for n in ("t64", "t32", "tiny")] + [("sem", n) for n in ("t64", "t32")]


class Case:
    """One recorded run.  A semantic case reads frames / tiles / stitched from channel 0 of its bottom-up twin (the generator asserts they are the same bits)."""

    def __init__(self, kind, name):
        z = golden()
        self.kind, self.name, self.semantic = kind, name, kind == "sem"
        self.params = json.loads(str(z[f"{kind}/{name}/params"]))
        nc = 1 if self.semantic else 4
        self.frames = z[f"bu/{name}/frames"]
        self.tiles = np.ascontiguousarray(z[f"bu/{name}/tiles"][:, :nc])
        self.stitched = np.ascontiguousarray(z[f"bu/{name}/stitched"][:, :nc])
        self.uncertain = z[f"{kind}/{name}/uncertain"]
        self.F = self.frames.shape[0]
        self.T = self.tiles.shape[0] // self.F
        self.entries = [dict(n=int(z[f"{kind}/{name}/{b}/n"]), masks=z[f"{kind}/{name}/{b}/masks"], scores=z[f"{kind}/{name}/{b}/scores"],
                             scales=z[f"{kind}/{name}/{b}/scales"]) for b in range(self.F)]
        self.keys = KEYS[:1] if self.semantic else KEYS
        self.channels = CHANNELS[:1] if self.semantic else CHANNELS

    def layer_kw(self):
        p = self.params
        return dict(tile_size=p["tile_size"], overlap=p["overlap"], blend=p["blend"], tile_batch_size=p["tile_batch_size"])


class ReplayBackend:
    """Returns the recorded reference tile maps in grid order, whatever it is given: the layer under test then sees the reference's forward exactly."""

    does_baked_postproc = False

    def __init__(self, case, device="cpu"):
        self.device = device
        self.tiles = torch.from_numpy(case.tiles).to(device)
        self.channels, self.keys = case.channels, case.keys
        self.pos = 0
        self.batch_sizes = []

    def __call__(self, x):
        assert x.dim() == 5 and x.shape[1] == 1  # (n, 1, C, ts, ts), as the reference hands tiles to its backend
        n = int(x.shape[0])
        self.batch_sizes.append(n)
        maps = self.tiles[self.pos : self.pos + n]
        assert maps.shape[0] == n, "more tiles asked for than were recorded"
        self.pos += n
        return dict(zip(self.keys, torch.split(maps, list(self.channels), dim=1)))

    def warmup(self, shape):
        pass


def inner_layer(case, backend, cls=None, **kw):
    from sleap_nn_amd.inference.layers import PostprocessConfig, PreprocessConfig, SegmentationLayer, SemanticSegmentationLayer

    cls = cls or (SemanticSegmentationLayer if case.semantic else SegmentationLayer)
    return cls(backend, 2, max_stride=8, fg_threshold=case.params["fg_threshold"], preprocess_config=PreprocessConfig(ensure_grayscale=True),
               postprocess_config=PostprocessConfig(peak_threshold=case.params["peak_threshold"]), **kw)


def tiled_layer(case, backend, **kw):
    from sleap_nn_amd.inference.layers import TiledSegmentationLayer, TiledSemanticSegmentationLayer

    inner = inner_layer(case, backend)
    return (TiledSemanticSegmentationLayer if case.semantic else TiledSegmentationLayer)(inner, **dict(case.layer_kw(), **kw))


def spy_postprocess(layer):
    """Records what ``inner.postprocess`` receives: a list of ``(raw_out, info)``."""
    seen = []
    post = layer.inner.postprocess

    def spy(raw_out, info):
        seen.append(({k: v.detach().cpu().clone() for k, v in raw_out.items()}, info))
        return post(raw_out, info)

    layer.inner.postprocess = spy
    return seen


def stitched_of(case, raw_out):
    return torch.cat([raw_out[k] for k in case.keys], dim=1).numpy()


def bits(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check_entries(case, pred_masks, frames=None, tag=""):
    """Entry counts equal, masks equal outside the recorded uncertain set, scores within 1e-4, scales equal."""
    frames = list(range(case.F)) if frames is None else frames
    assert len(pred_masks) == len(frames), tag
    for got, b in zip(pred_masks, frames):
        ref = case.entries[b]
        assert case.uncertain[b].mean() <= 0.005
        assert len(got) == ref["n"], (tag, b, len(got), ref["n"])
        for i, d in enumerate(got):
            assert abs(d["score"] - ref["scores"][i]) <= 1e-4, (tag, b, i, d["score"], ref["scores"][i])
            assert tuple(d["scale"]) == tuple(ref["scales"][i]) and d["mask"].shape == ref["masks"][i].shape, (tag, b, i)
            skip = case.uncertain[b][: d["mask"].shape[0], : d["mask"].shape[1]]
            diff = d["mask"] != ref["masks"][i]
            assert not (diff & ~skip).any(), (tag, b, i, int((diff & ~skip).sum()))
