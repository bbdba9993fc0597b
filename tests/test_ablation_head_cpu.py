"""CPU: the model surface of the paper's ablation heads (CORNER_PREDICTION direct / offset / iterative, CENTERNESS none):
submodules and state-dict keys per mode equal the reference's (tests/golden/head_ablation.npz), reference-format checkpoints
load strictly, the weights pack per mode, and what stays out of scope is still refused.  No kernel runs."""
import glob
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_MODES = {
    "direct_none": ("direct", "none"),
    "offset_oriented": ("offset", "oriented"),
    "iterative_plain": ("iterative", "plain"),
    "c2c_none": ("center-to-corner", "none"),
    "iterative_none_c2": ("iterative", "none"),
}


def _cfg(name="dota-1.0_r50.yaml", opts=()):
    from dafne_amd.config import load_cfg
    return load_cfg(os.path.join(ROOT, "configs", name), list(opts))


def _head(strategy, centerness, num_classes=15, extra=()):
    from dafne_amd.modeling.dafne.dafne import DAFNeHead
    cfg = _cfg(opts=["MODEL.DAFNE.CORNER_PREDICTION", strategy, "MODEL.DAFNE.CENTERNESS", centerness,
                     "MODEL.DAFNE.NUM_CLASSES", str(num_classes)] + list(extra))
    return DAFNeHead(cfg, [types.SimpleNamespace(channels=256)] * 5)


@pytest.mark.parametrize("name", sorted(HEAD_MODES))
def test_state_dict_keys_and_shapes_equal_the_reference(golden, name):
    g = golden("head_ablation")
    head = _head(*HEAD_MODES[name], num_classes=int(g[name + "_cfg"][0]))
    sd = head.state_dict()
    want = {str(k): tuple(int(v) for v in s if v >= 0) for k, s in zip(g[name + "_keys"], g[name + "_shapes"])}
    assert set(sd) == set(want)
    for k, v in sd.items():
        assert tuple(v.shape) == want[k], k
    if name.startswith("offset"):
        assert torch.equal(head.base_corners.reshape(8), torch.from_numpy(g[name + "_base_corners"]))


@pytest.mark.parametrize("strategy", ["offset", "iterative"])
def test_reference_format_checkpoint_loads_strictly(tmp_path, strategy):
    """A detectron2-style checkpoint ({"model": state_dict}) of a whole detector with an ablation head."""
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.checkpoint import load_weights
    from dafne_amd.registry import build_model
    from oracle.model import fill_params
    cfg = _cfg(opts=["MODEL.DAFNE.CORNER_PREDICTION", strategy, "MODEL.DAFNE.CENTERNESS", "oriented"])
    src = build_model(cfg)
    fill_params(src.proposal_generator.dafne_head, seed=3)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    hp = "proposal_generator.dafne_head."
    assert (hp + "base_corners" in sd) == (strategy == "offset")
    assert (hp + "c3_pred.weight" in sd) == (strategy == "iterative")
    assert hp + "center_pred.weight" not in sd and hp + "center_tower.0.weight" not in sd
    path = str(tmp_path / "model_final.pth")
    torch.save({"model": sd, "iteration": 1}, path)
    m = build_model(cfg)
    missing, unexpected = load_weights(m, path, strict=True)
    assert not missing and not unexpected
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # a released-head checkpoint is not an ablation head's: strict loading refuses it
    rel = build_model(_cfg())
    path2 = str(tmp_path / "released.pth")
    torch.save({"model": rel.state_dict()}, path2)
    with pytest.raises(Exception):
        load_weights(build_model(cfg), path2, strict=True)


@pytest.mark.parametrize("strategy,centerness,pred_c", [("direct", "none", 8), ("offset", "plain", 9), ("iterative", "oriented", 9),
                                                        ("iterative", "none", 8), ("center-to-corner", "none", 8)])
def test_head_weights_pack_per_mode(strategy, centerness, pred_c):
    from dafne_amd import engine
    from oracle.model import fill_params
    head = _head(strategy, centerness)
    fill_params(head, seed=4)
    if strategy == "offset":
        with torch.no_grad():
            head.base_corners.copy_(torch.tensor([-2.0, 2.0, 2.0, 2.0, 2.0, -2.0, -2.0, -2.0]).view(1, 8, 1, 1))
    sd = head.state_dict()
    P = engine.pack_head_weights(sd, "cpu", prefix="")
    assert P["head_mode"] == (strategy, centerness != "none") == head.head_mode
    towers = ("cls_tower", "center_tower", "corners_tower") if strategy == "center-to-corner" else ("cls_tower", "corners_tower")
    assert set(k.split(".")[0] for k in P if "_tower." in k) == set(towers)
    assert ("center_pred" in P) == (strategy == "center-to-corner")
    w, b = P["corners_ctrness"]
    # rows beyond pred_c are the kernel's zero padding
    assert bool((w[pred_c:] == 0).all()) and bool((b[pred_c:] == 0).all())
    if strategy == "iterative":
        chain = P["corner_chain"]
        assert chain.numel() == 216 and chain.dtype == torch.float32
        assert torch.equal(chain[:36], sd["c1_pred.weight"][:, 256:].reshape(-1))
        assert torch.equal(chain[108:], sd["c3_pred.weight"][:, 256:].reshape(-1))
        want_b = torch.cat([sd["c%d_pred.bias" % k] for k in range(4)])
    elif strategy == "offset":
        want_b = sd["corners_pred.bias"] + sd["base_corners"].reshape(8)       # the base folded into the bias
    else:
        want_b = sd["corners_pred.bias"]
    if centerness != "none":
        want_b = torch.cat([want_b, sd["ctrness.bias"]])
    assert torch.equal(b[:pred_c], want_b)


def test_fp8_with_an_ablation_head_is_refused_at_build():
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.registry import build_model
    for strategy, centerness in (("direct", "none"), ("iterative", "oriented"), ("center-to-corner", "none")):
        with pytest.raises(NotImplementedError, match="fp8"):
            build_model(_cfg("ucas_aod_r101_fp8.yaml", ["MODEL.DAFNE.CORNER_PREDICTION", strategy,
                                                        "MODEL.DAFNE.CENTERNESS", centerness]))
    build_model(_cfg("ucas_aod_r101_fp8.yaml"))            # the released head stays buildable in fp8


@pytest.mark.parametrize("opts", [
    ["MODEL.DAFNE.CORNER_PREDICTION", "angle"],
    ["MODEL.DAFNE.MERGE_CORNER_CENTER_PRED", "True"],
    ["MODEL.DAFNE.CORNER_TOWER_ON_CENTER_TOWER", "False"],
    ["MODEL.DAFNE.CTR_ON_REG", "False"],
    ["MODEL.DAFNE.CTR_ON_REG", "False", "MODEL.DAFNE.CORNER_PREDICTION", "direct"],
    ["MODEL.DAFNE.USE_DEFORMABLE", "True", "MODEL.DAFNE.CORNER_PREDICTION", "iterative"],
    ["MODEL.DAFNE.NORM", "BN", "MODEL.DAFNE.CORNER_PREDICTION", "direct"],
    ["MODEL.DAFNE.NORM", "none"],
    ["MODEL.DAFNE.NUM_SHARE_CONVS", "1", "MODEL.DAFNE.CORNER_PREDICTION", "offset"],
    ["MODEL.DAFNE.NUM_BOX_CONVS", "2", "MODEL.DAFNE.CORNER_PREDICTION", "direct"],
])
def test_out_of_scope_heads_still_raise(opts):
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.registry import build_model
    with pytest.raises(NotImplementedError, match="direct, offset or iterative"):
        build_model(_cfg(opts=opts))


def test_ablation_configs_load_and_build():
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.registry import build_model
    names = [os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "configs", "*_ablation.yaml"))]
    assert {"dota-1.0_r50_ablation.yaml", "hrsc_r50_ablation.yaml"} <= set(names)
    for n in names:
        cfg = _cfg(n)
        assert (cfg.MODEL.DAFNE.CORNER_PREDICTION, cfg.MODEL.DAFNE.CENTERNESS) == ("direct", "none")
        m = build_model(cfg)
        keys = set(m.state_dict())
        assert not any(".center_tower." in k or ".center_pred." in k or ".ctrness." in k for k in keys)
        assert m.proposal_generator.dafne_outputs.has_centerness is False
    d10 = _cfg("dota-1.0_r50_ablation.yaml")
    assert d10.MODEL.DAFNE.THRESH_WITH_CTR is True and d10.MODEL.DAFNE.NUM_CLASSES == 15
    assert _cfg("hrsc_r50_ablation.yaml").MODEL.DAFNE.NUM_CLASSES == 1


def test_head_outputs_follow_the_mode():
    """engine.HeadOutputs (the whole-batch buffers of the sub-batch layout) hold what the mode's head writes."""
    from dafne_amd import engine
    for mode, names in ((engine.RELEASED_HEAD, {"logits", "center", "delta_ctr"}),
                        (("direct", False), {"logits", "delta_ctr"}),
                        (("iterative", True), {"logits", "delta_ctr", "corners"})):
        ho = engine.HeadOutputs(4, 64, 96, 3, [1.0] * 5, "cpu", head_mode=mode)
        v = ho.views(1, 3)
        assert set(v) == names
        assert v["delta_ctr"][0].shape == (2, 8, 12, engine.head_pred_channels(mode))
        if "corners" in v:
            assert v["corners"][4].shape == (2, 1, 1, 8)
    assert np.array_equal(np.array(engine.head_mode_of({"x.c0_pred.weight": 0}, "x.")), np.array(("iterative", False)))
