"""Swinv2 backbones with effective windows of 9..24 (the key-tiled kernel) without a GPU: id resolution (the large row, the window<X>to<Y> rule), the second opt-in and
its refusals, the program of fixtures C, D and E (tests/_swinv2_wide_cases.py), the coordinate table at wide windows against ``transformers``, the goldens of C and D
(tools/gen_pretrained_swinv2_wide_golden.py) against tests/swinv2_ref.py, and the float64 statement the kernel is held to against HuggingFace's own attention layer at
windows 12 and 16.  The bars are those of tests/test_pretrained_swinv2_cpu.py."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import _swinv2_cases as SC
from tests import _swinv2_wide_cases as WC
from tests import swinv2_ref as R

ENC, HEAD = WC.ENC, WC.HEAD
MS = "microsoft/swinv2-"


def rel(got, want):
    want = torch.as_tensor(want)
    return (torch.as_tensor(got) - want).abs().max().item() / max(1e-30, want.abs().max().item())


# ---- id resolution

SIZES = {"tiny": (96, [2, 2, 6, 2], [3, 6, 12, 24]), "small": (96, [2, 2, 18, 2], [3, 6, 12, 24]), "base": (128, [2, 2, 18, 2], [4, 8, 16, 32]),
         "large": (192, [2, 2, 18, 2], [6, 12, 24, 48])}
IDS = [(f"{MS}tiny-patch4-window16-256", "tiny", 16, 256, [0, 0, 0, 0]), (f"{MS}small-patch4-window16-256", "small", 16, 256, [0, 0, 0, 0]),
       (f"{MS}base-patch4-window16-256", "base", 16, 256, [0, 0, 0, 0]),
       (f"{MS}base-patch4-window12-192-22k", "base", 12, 192, [0, 0, 0, 0]), (f"{MS}large-patch4-window12-192-22k", "large", 12, 192, [0, 0, 0, 0]),
       (f"{MS}base-patch4-window12to16-192to256-22kto1k-ft", "base", 16, 256, [12, 12, 12, 6]), (f"{MS}large-patch4-window12to16-192to256-22kto1k-ft", "large", 16, 256, [12, 12, 12, 6]),
       (f"{MS}base-patch4-window12to24-192to384-22kto1k-ft", "base", 24, 384, [12, 12, 12, 6]), (f"{MS}large-patch4-window12to24-192to384-22kto1k-ft", "large", 24, 384, [12, 12, 12, 6])]


@pytest.mark.parametrize("model_name,size,window,image,pws", IDS, ids=[i[0][len(MS):] for i in IDS])
def test_ids_resolve_to_size_window_image_and_pretrained_windows(model_name, size, window, image, pws):
    from sleap_nn_amd.architectures import pretrained as P

    a = P.resolve_architecture(model_name, allow_swinv2=True, allow_swinv2_wide=True)
    e, d, h = SIZES[size]
    assert (a["family"], a["embed_dim"], a["depths"], a["num_heads"], a["window_size"], a["image_size"], a["pretrained_window_sizes"]) == ("swinv2", e, d, h, window, [image, image], pws)
    assert a["hidden_sizes"] == [e * 2 ** i for i in range(4)]


def test_windows_and_shifts_of_the_wide_geometries():
    from sleap_nn_amd.architectures import pretrained as P

    assert P.swinv2_windows(256, 4, 16) == [(16, 8), (16, 8), (16, 0), (8, 0)]    # window16-256 and 12to16: shifts only where the resolution exceeds the window
    assert P.swinv2_windows(192, 4, 12) == [(12, 6), (12, 6), (12, 0), (6, 0)]    # window12-192
    assert P.swinv2_windows(384, 4, 24) == [(24, 12), (24, 12), (24, 0), (12, 0)]  # 12to24
    assert P.swinv2_windows(128, 4, 16) == [(16, 8), (16, 0), (8, 0), (4, 0)]     # fixture C
    assert P.swinv2_windows(96, 4, 12) == [(12, 6), (12, 0), (6, 0), (3, 0)]      # fixture D
    assert P.swinv2_windows(192, 4, 24) == [(24, 12), (24, 0), (12, 0), (6, 0)]   # fixture E
    for name in WC.FIXTURES:
        assert R.windows_of(WC.arch_of(name)) == P.swinv2_windows(WC.FIXTURES[name]["image_size"], 4, WC.FIXTURES[name]["window_size"])


def test_a_local_config_wins_over_the_recalled_table(tmp_path):
    """The large row and the <X>to<Y> rule are as recalled and cannot be confirmed without the hub: a local ``config.json`` must override both, whatever the directory is
    called (and the module says that they are recalled, in whatever words)."""
    from sleap_nn_amd.architectures import pretrained as P

    d = tmp_path / "swinv2-large-patch4-window12to16-192to256-22kto1k-ft"
    d.mkdir()
    with open(d / "config.json", "w") as f:
        json.dump(WC.arch_of("D"), f)
    a = P.resolve_architecture(str(d), allow_swinv2=True, allow_swinv2_wide=True)
    assert (a["embed_dim"], a["window_size"], a["image_size"], a["pretrained_window_sizes"]) == (32, 12, [96, 96], [0, 0, 0, 0])
    with open(P.__file__) as f:
        assert "recalled" in f.read().lower()


def test_a_shifted_case_has_queries_whose_first_tile_is_all_masked():
    """What tests/test_gpu_window_attn_v2_wide.py relies on: at window 16, shift 8, the queries of band 3 (the last 8 rows and columns of the last window) see only other
    bands in key tile 0 (tokens 0..31 are rows 0 and 1), so their running maximum starts from scores that all carry the -200 and rises by about that much when their own
    band arrives; the kernel cases hold a shifted window-16 map whose last window has that band."""
    w, shift = 16, 8
    ty, tx = np.divmod(np.arange(w * w), w)
    band = 2 * (ty >= w - shift) + (tx >= w - shift)
    assert np.all(band[:32] != 3) and np.any(band == 3)
    assert any(c[0] == w and c[1] == shift for c in WC.KERNEL_CASES)


@pytest.mark.parametrize("name", ["C", "D", "E"])
def test_window_and_shift_equal_the_installed_layers(name):
    tr = pytest.importorskip("transformers")
    arch = WC.arch_of(name)
    enc = tr.Swinv2Backbone(tr.Swinv2Config(**{k: v for k, v in arch.items() if k != "model_type"}))
    got = [(blk.window_size, blk.shift_size) for stage in enc.encoder.layers for blk in stage.blocks]
    assert got == WC.WINDOWS[name]


# ---- the opt-in

def test_without_the_wide_opt_in_the_refusal_names_all_three(tmp_path):
    from sleap_nn_amd.architectures.model import get_backbone

    names = [i[0] for i in IDS] + [WC.hf_dir(n, tmp_path) for n in WC.FIXTURES]
    for model_name in names:
        with pytest.raises(NotImplementedError, match="window") as e:
            get_backbone("pretrained", WC.backbone_config("C", model_name, allow=True, wide=False))
        msg = str(e.value)
        assert "allow_swinv2_wide" in msg and "build_model(..., swinv2_wide=True)" in msg and "from_model_paths(..., swinv2_wide=True)" in msg, msg


def test_with_it_the_backbone_builds_and_alone_it_opens_nothing(tmp_path):
    from sleap_nn_amd.architectures.model import get_backbone

    for name in WC.FIXTURES:
        bb = get_backbone("pretrained", WC.backbone_config(name, WC.hf_dir(name, tmp_path)))
        assert bb.family == "swinv2" and bb.window_size == WC.FIXTURES[name]["window_size"] and bb.channels == [32, 64, 128, 256]
    big = get_backbone("pretrained", WC.backbone_config("C", f"{MS}base-patch4-window12to24-192to384-22kto1k-ft"))
    assert big.window_size == 24 and big.pretrained_window_sizes == [12, 12, 12, 6] and big.channels == [128, 256, 512, 1024]
    for model_name in (WC.hf_dir("C", tmp_path), IDS[0][0]):  # allow_swinv2_wide without allow_swinv2: the family's own refusal, as if the key were absent
        with pytest.raises(NotImplementedError, match="allow_swinv2=True") as e:
            get_backbone("pretrained", WC.backbone_config("C", model_name, allow=False, wide=True))
        assert "pretrained_swinv2" in str(e.value)
    # windows of 2..8 need nothing new
    assert get_backbone("pretrained", SC.backbone_config("A", WC.hf_dir("C", tmp_path, window_size=8, image_size=64, pretrained_window_sizes=[0, 0, 0, 0]))).window_size == 8


def test_windows_above_24_and_below_2_stay_refused(tmp_path):
    from sleap_nn_amd.architectures.model import get_backbone

    for over in ({"window_size": 32, "image_size": 256}, {"window_size": 25, "image_size": 400}, {"window_size": 4, "image_size": 4}):
        with pytest.raises(NotImplementedError, match="window") as e:
            get_backbone("pretrained", WC.backbone_config("C", WC.hf_dir("C", tmp_path, **over)))
        assert "2..24" in str(e.value)
    # a window_size above 24 whose EFFECTIVE windows fit builds: stage i runs min(resolution, window_size)
    assert get_backbone("pretrained", WC.backbone_config("C", WC.hf_dir("C", tmp_path, window_size=32, image_size=96))).window_size == 32


def test_the_three_spellings_of_the_opt_in(tmp_path):
    from sleap_nn_amd.inference.loaders import load_model_assets
    from sleap_nn_amd.inference.predictor import Predictor

    m0 = WC.new_model("D", tmp_path)
    sd = WC.fixture_state("D", tmp_path)
    run = WC.write_run_dir(tmp_path / "run_d", "D", sd)
    a = load_model_assets(run)
    assert "allow_swinv2" not in a.backbone_config and "allow_swinv2_wide" not in a.backbone_config  # the config as the yaml has it
    with pytest.raises(NotImplementedError, match="pretrained_swinv2"):
        a.build_model()
    with pytest.raises(NotImplementedError, match="pretrained_swinv2"):
        a.build_model(swinv2_wide=True)
    with pytest.raises(NotImplementedError, match="swinv2_wide"):
        a.build_model(pretrained_swinv2=True)
    m = a.build_model(pretrained_swinv2=True, swinv2_wide=True)
    assert m.is_swinv2 and m.backbone.window_size == 12 and list(m.param_shapes) == list(m0.param_shapes)
    for k in (f"{ENC}.encoder.layers.0.blocks.1.attention.self.logit_scale", f"head_layers.0.{HEAD}.0.weight"):
        assert torch.equal(m.state_dict()[k], sd[k])
    assert "swinv2_wide" in inspect.signature(Predictor.from_model_paths).parameters  # (the predictor itself needs a device: tests/test_gpu_pretrained_swinv2_wide.py)


def test_training_is_refused_by_name(tmp_path):
    from sleap_nn_amd.training.module import TrainingModule

    m = WC.new_model("D", tmp_path)
    with pytest.raises(NotImplementedError, match="Swinv2"):
        m.train(True, allow_pretrained=True)
    with pytest.raises(NotImplementedError, match="Swinv2"):
        TrainingModule(m, pretrained_training=True)


# ---- the program

@pytest.mark.parametrize("name", ["C", "D", "E"])
def test_program_of_the_fixture(name, tmp_path):
    from sleap_nn_amd import _lib as L

    m = WC.new_model(name, tmp_path)
    c = WC.FIXTURES[name]
    att = [o for o in m.ops if o.kind == L.OP_WINDOW_ATTN_V2]
    assert [(o.ksize, o.cmid) for o in att] == WC.WINDOWS[name] and L.OP_WINDOW_ATTN not in [o.kind for o in m.ops]
    assert [o.cin1 for o in att] == [h for h, d in zip(c["num_heads"], c["depths"]) for _ in range(d)]
    assert all(o.flags & L.FLAG_NO_TRAIN for o in att)
    assert m.ops[0].kind == L.OP_PATCH_STEM and sum(o.kind == L.OP_PATCH_MERGE for o in m.ops) == 3
    sd = WC.fixture_state(name, tmp_path)
    m.load_state_dict(sd, strict=True)
    d = m.backbone.derived_params(m._state, m.buffers)
    for o in att:
        assert tuple(d[o.weight].shape) == (o.cin1, (2 * o.ksize - 1) ** 2) and d[o.weight].dtype == torch.float32  # the table follows the block's effective window
        assert tuple(d[o.weight2].shape) == (o.cin1,) and tuple(d[o.bias].shape) == (3 * 32 * o.cin1,)
        assert float(d[o.bias][32 * o.cin1: 64 * o.cin1].abs().max()) == 0.0  # a padded token's key is exactly 0
        assert 0.0 < float(d[o.weight].min()) and float(d[o.weight].max()) < 16.0


@pytest.mark.parametrize("window,pretrained", [(16, 12), (12, 0), (24, 12), (12, 6), (9, 0)])
def test_coords_table_equals_the_installed_buffer(window, pretrained):
    tr = pytest.importorskip("transformers")
    from transformers.models.swinv2.modeling_swinv2 import Swinv2SelfAttention

    from sleap_nn_amd.architectures import pretrained as P

    att = Swinv2SelfAttention(tr.Swinv2Config(), dim=96, num_heads=3, window_size=window, pretrained_window_size=[pretrained, pretrained])
    mine = P.swinv2_coords_table(window, pretrained)
    assert mine.dtype == torch.float32 and mine.shape == ((2 * window - 1) ** 2, 2) and torch.equal(mine, att.relative_coords_table.view(-1, 2))  # the same bits
    N = window * window
    ty, tx = np.divmod(np.arange(N), window)
    idx = torch.from_numpy((ty[:, None] - ty[None, :] + window - 1) * (2 * window - 1) + (tx[:, None] - tx[None, :] + window - 1))  # the kernels' index: (query - key)
    assert torch.equal(idx, att.relative_position_index)


def test_abi_and_signatures():
    from sleap_nn_amd import _lib as L

    with open(os.path.join(WC.ROOT, "include", "posehip.h")) as f:
        header = f.read()
    assert int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", header, re.M).group(1)) >= 133
    assert "int ph_debug_window_attn_v2_wide_run(" in header and "#define PH_KV_WINDOW_ATTN_V2_WIDE 35" in header
    assert "ph_debug_window_attn_v2_wide_run" in L.SIGNATURES and L.SIGNATURES["ph_debug_window_attn_v2_wide_run"] == L.SIGNATURES["ph_debug_window_attn_v2_run"]
    assert L.SWINV2_KV_WINDOW_ATTN_WIDE == 35 and L.SWINV2_KV_WINDOW_ATTN == 32


# ---- goldens and the restatement

@pytest.mark.parametrize("name", ["C", "D"])
def test_restatement_reproduces_the_reference(name, tmp_path):
    g, sd = WC.golden(name), WC.fixture_state(name, tmp_path)
    img = torch.from_numpy(g["frames"])
    bb, arch = WC.backbone_config(name, "unused"), WC.arch_of(name)
    col = {}
    bo = R.backbone_forward(sd, bb, arch, img.float() / 255.0, col)
    assert len(bo["feature_maps"]) == 5
    for i, f in enumerate(bo["feature_maps"]):
        assert rel(f, g[f"feat/{i}"]) <= 1e-5, i
    layers = [k[len("layer/"):] for k in g if k.startswith("layer/")]
    assert len(layers) == 3 * sum(WC.FIXTURES[name]["depths"]) + 3
    for k in layers:  # (stored for frame 1 only)
        assert rel(col[k][1:2], g["layer/" + k]) <= 1e-5, k
    n_dec = sum(1 for k in g if k.startswith("dec/"))
    assert n_dec == len(bo["outputs"]) == 2
    for i, o in enumerate(bo["outputs"]):
        assert int(g[f"dec_stride/{i}"]) == bo["strides"][i]
        assert rel(o, g[f"dec/{i}"]) <= 1e-5, i
    out = R.model_forward(sd, bb, arch, WC.head_config(name), "single_instance", img)
    assert rel(out[HEAD], g["head"]) <= 1e-5


def test_goldens_are_small_and_hold_no_weights():
    import glob

    files = sorted(glob.glob(os.path.join(WC.GOLD, "pretrained_swinv2_[cd]*.npz")))
    assert len(files) >= 4
    for f in files:
        assert os.path.getsize(f) < 900 * 1024, f
        assert not any(k.endswith((".weight", ".bias", "logit_scale")) for k in np.load(f).files), f


@pytest.mark.parametrize("w,shift,H,W", [(12, 6, 12, 24), (16, 8, 16, 32), (16, 0, 16, 16)])
def test_float64_statement_equals_the_installed_attention(w, shift, H, W):
    """``window_attn_v2_f64`` on a qkv map against ``Swinv2SelfAttention`` (float64) on the windows of the same map, with HuggingFace's own mask: what the kernel is held
    to is what the layer computes, at wide windows too.  The map is window-aligned (padded tokens are the existing CPU tests')."""
    tr = pytest.importorskip("transformers")
    from transformers.models.swinv2.modeling_swinv2 import Swinv2SelfAttention

    from sleap_nn_amd.architectures import pretrained as P

    heads, Cc, B = 2, 64, 1
    att = Swinv2SelfAttention(tr.Swinv2Config(), dim=Cc, num_heads=heads, window_size=w, pretrained_window_size=[0, 0]).eval()
    seed = 31 + w
    sd = {k: torch.from_numpy(SC.draw_tensor("x.blocks.1.attention.self." + k, tuple(v.shape), seed)) for k, v in att.state_dict().items()}
    att.load_state_dict(sd)
    att = att.double()
    x = torch.randn(B, H, W, Cc, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    with torch.no_grad():
        q, k, v = att.query(x), att.key(x), att.value(x)
        xs = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2)) if shift else x
        win = R.partition(xs, w).view(-1, w * w, Cc)
        mask = R.shift_mask(H, W, w, shift, torch.float64)
        ctx = att(win, attention_mask=mask)[0]
        y = R.reverse(ctx.view(-1, w, w, Cc), w, H, W)
        want = (torch.roll(y, shifts=(shift, shift), dims=(1, 2)) if shift else y).numpy()
    mlp = "continuous_position_bias_mlp"
    table = P.swinv2_bias_table(P.swinv2_coords_table(w, 0), sd[mlp + ".0.weight"], sd[mlp + ".0.bias"], sd[mlp + ".2.weight"]).numpy()
    scale = P.swinv2_logit_scale(sd["logit_scale"]).numpy()
    qkv = torch.cat([q, k, v], dim=-1).numpy()
    bias = np.concatenate([sd["query.bias"].numpy(), np.zeros(Cc, np.float32), sd["value.bias"].numpy()])
    got = SC.window_attn_v2_f64(qkv, bias, scale, table, heads, w, shift)
    err = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
    assert got.shape == want.shape and err <= 2e-5, err  # (table and scale are rounded to float32 once, as the library is handed them)
    if shift:
        assert float(np.abs(SC.window_attn_v2_f64(qkv, bias, scale, table, heads, w, 0) - want).max()) > 1e-2


def test_the_statement_sees_shift_bias_index_and_padded_keys_at_window_16():
    """What the kernel's bound would hide if the float64 statement ignored it, at a wide window: each of these changes the statement by order one."""
    case = (16, 8, 1, 20, 36, 1, False, False)
    qkv, bias, scale, table = WC.operands(case)
    base = SC.window_attn_v2_f64(qkv, bias, scale, table, 1, 16, 8)
    assert np.abs(SC.window_attn_v2_f64(qkv, bias, scale, table, 1, 16, 0) - base).max() > 1e-2            # the shift and its band mask
    assert np.abs(SC.window_attn_v2_f64(qkv * 2.0, bias, scale, table, 1, 16, 8) - 2.0 * base).max() > 1e-2   # padded tokens do not scale with the map: they are keys
    assert np.abs(SC.window_attn_v2_f64(qkv, bias, scale, np.roll(table, 1, axis=1), 1, 16, 8) - base).max() > 1e-2  # the bias index
    half = qkv.copy()
    half[..., :32] *= 0.5  # q is normalised: halving it changes nothing
    assert np.abs(SC.window_attn_v2_f64(half, bias, scale, table, 1, 16, 8) - base).max() < 1e-9


def test_reference_order_fp32_is_the_existing_tests(tmp_path):
    """The restated ``operands`` / ``hf_order_fp32`` are those of tests/test_gpu_window_attn_v2.py, bit for bit (the bound is measured against the same evaluation)."""
    from tests import test_gpu_window_attn_v2 as T

    case = (7, 3, 2, 9, 15, 3, False, True)
    for a, b in zip(WC.operands(case), T.operands(case)):
        assert np.array_equal(a, b)
    ops = WC.operands(case)
    assert np.array_equal(WC.hf_order_fp32(*ops, 3, 7, 3), T.hf_order_fp32(*ops, 3, 7, 3))


def test_forced_rescale_operands_do_force_it():
    """The construction of the forced-rescale inputs, in float64: query A's maximum sits in the last key tile and exceeds every earlier tile's by more than 20; query B's
    tile maximum rises at every tile."""
    for w in (16, 24):
        (qkv, _bias, scale, table), (ta, tb) = WC.forced_rescale_operands(w)
        N, T = w * w, (w * w + 31) // 32
        flat = qkv.reshape(N, 96).astype(np.float64)
        kn = flat[:, 32:64] / np.linalg.norm(flat[:, 32:64], axis=1, keepdims=True)
        for t, rising in ((ta, False), (tb, True)):
            s = float(scale[0]) * kn @ (flat[t, :32] / np.linalg.norm(flat[t, :32])) + float(table[0, 0])
            tile_max = np.array([s[32 * j: 32 * j + 32].max() for j in range(T)])
            if rising:
                assert np.all(np.diff(tile_max) > 0), (w, tile_max)
            else:
                assert tile_max[-1] - tile_max[:-1].max() > 20.0 and int(np.argmax(s)) == N - 1, (w, tile_max)
