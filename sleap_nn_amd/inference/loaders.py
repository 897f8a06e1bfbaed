"""Checkpoint + config ingestion for existing sleap-nn run directories
(``best.ckpt`` + ``training_config.yaml``), without Lightning / OmegaConf installed.

Counterpart of ``sleap_nn/inference/loaders.py:87-221,1054`` (``load_model_assets``) reduced to
what the hot path needs: the ``state_dict`` (LightningModule keys ``model.*``), the backbone and
head configs, the preprocessing block and the skeleton's node/edge names.
"""
from __future__ import annotations

import os
import pickle
import types
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import yaml

MODEL_TYPES = ("single_instance", "centroid", "centered_instance", "bottomup", "multi_class_bottomup", "multi_class_topdown", "bottomup_segmentation",
               "semantic_segmentation", "centered_instance_segmentation")


class _Opaque:
    """Stand-in for classes the pickle references but this environment lacks (omegaconf, lightning...)."""

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        self.__dict__["_state"] = state


class _TolerantUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        try:
            return super().find_class(module, name)
        except Exception:
            return type(name, (_Opaque,), {})


def _pickle_module():
    pm = types.ModuleType("pickle")
    pm.Unpickler = _TolerantUnpickler
    pm.load = lambda f, **k: _TolerantUnpickler(f, **k).load()
    pm.__name__ = "pickle"
    return pm


def load_lightning_state_dict(ckpt_path: str) -> Dict[str, torch.Tensor]:
    """``state_dict`` of a Lightning checkpoint; tensors stay on the CPU."""
    ck = torch.load(ckpt_path, map_location="cpu", weights_only=False, pickle_module=_pickle_module())
    sd = ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck
    return {k: v for k, v in sd.items() if isinstance(v, torch.Tensor)}


@dataclass
class LoadedAssets:
    """What ``load_model_assets`` of the reference returns, in plain-Python form."""

    model_type: str
    backbone_type: str
    backbone_config: dict
    head_config: dict
    preprocessing: dict
    state_dict: Dict[str, torch.Tensor]
    model_dir: str
    node_names: List[str]
    edges: List[Tuple[str, str]]

    def build_model(self, pretrained_resnet: bool = False, pretrained_swinv2: bool = False, swinv2_wide: bool = False):
        """``pretrained_resnet=True`` (opt-in): a ``pretrained`` run directory of the ResNet family builds (the backbone-config key ``allow_resnet``); without it such a
        directory is refused by name, as before.  ``pretrained_swinv2=True``: the same for the Swinv2 family (``allow_swinv2``);
        ``swinv2_wide=True`` on top of it: effective windows of 9..24 build too (``allow_swinv2_wide``; alone it opens nothing)."""
        from sleap_nn_amd.architectures.model import Model

        bb_cfg = self.backbone_config
        if self.backbone_type == "pretrained":  # a relative model_name (a directory with a config.json) is looked up next to the checkpoint first; the stored config stays as the yaml has it
            bb_cfg = {**bb_cfg, "_run_dir": os.path.abspath(self.model_dir)}
            if pretrained_resnet:
                bb_cfg["allow_resnet"] = True
            if pretrained_swinv2:
                bb_cfg["allow_swinv2"] = True
            if swinv2_wide:
                bb_cfg["allow_swinv2_wide"] = True
        if self.model_type == "centered_instance_segmentation":
            # a lone SegmentationHead with the sigmoid in its epilogue: the semantic type's program, built from the same `segmentation` leaf (whose
            # anchor_part / crop_size are data-pipeline entries, not head arguments); `model_type` here keeps the real name
            m = Model(self.backbone_type, bb_cfg, {"segmentation": self.head_config["segmentation"]}, "semantic_segmentation")
        else:
            m = Model(self.backbone_type, bb_cfg, self.head_config, self.model_type)
        m.load_state_dict(self.state_dict, strict=True)
        return m


def load_model_assets(model_dir: str, ckpt_name: str = "best.ckpt") -> LoadedAssets:
    cfg_path = os.path.join(model_dir, "training_config.yaml")
    if not os.path.exists(cfg_path):
        raise FileNotFoundError(f"{cfg_path} not found")
    cfg = yaml.safe_load(open(cfg_path))
    mc = cfg["model_config"]
    heads = mc["head_configs"]
    model_type = next((k for k in MODEL_TYPES if heads.get(k)), None)
    if model_type is None:
        raise ValueError(f"no known head config in {cfg_path}: {list(heads)}")
    bb = mc["backbone_config"]
    backbone_type = next((k for k in ("unet", "convnext", "swint", "pretrained") if bb.get(k)), None)
    if backbone_type is None:
        raise ValueError(f"no backbone config in {cfg_path}")
    skels = cfg.get("data_config", {}).get("skeletons") or []
    skel = skels[0] if isinstance(skels, (list, tuple)) and skels and isinstance(skels[0], dict) else {}  # (segmentation runs may carry no skeleton, or an empty one)
    nodes = [n["name"] for n in skel.get("nodes") or []]
    edges = [(e["source"]["name"], e["destination"]["name"]) for e in skel.get("edges") or []]
    sd = load_lightning_state_dict(os.path.join(model_dir, ckpt_name))
    return LoadedAssets(model_type, backbone_type, bb[backbone_type], heads[model_type], cfg.get("data_config", {}).get("preprocessing", {}) or {},
                        sd, model_dir, nodes, edges)
