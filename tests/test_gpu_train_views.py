"""GPU: augmented training views and their ground truth on the device (dafne_amd/data/train_views.py; train_views_kernel in
csrc/resize.hip behind dafne_train_views_u8_hip, csrc/train_views_kernels.h behind dafne_train_gt_hip).  Every comparison is
exact, against the numpy restatement tests/_train_views_np.py (pinned to PIL and np.rot90 by tests/test_train_views_cpu.py).

  * pixels: 37 x 53 HWC and 40 x 64 CHW sources; windows inside, overhanging right / bottom, the whole image; all 16
    orientations x {new == win, 35 x 51, 70 x 90, 53 -> 19}; a slab larger than every view, pre-filled with 0xFF (the padding
    is written 0 by the launch); 20 views with more than 8 distinct axes; a 1 x 1 window; a steep downscale (a small tile
    edge); refusals; two runs give equal bits;
  * ground truth: the fixture made by the reference's own DAFNeDatasetMapper (tests/golden/train_views.npz); 20 seeded batches with 0 .. 150 objects per view, first and last view empty, one batch whose objects are
    all dropped, sorted and unsorted; offsets, src, classes and the float arrays bitwise;
  * end to end (R50, seeded weights, a 400 x 330 scene, patch 256, overlap 64): identity parameters against gather_tiles,
    TileGroundTruth.instances and validation_losses_scenes; seeded random parameters with two view sizes in one batch against
    host-made pixels and make_gt_instances ground truth; a backward through losses(); detect_packed before and after."""
import itertools
import os

import numpy as np
import pytest
import torch

import _scene_labels_np as sl
import _train_views_np as tv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIENTATIONS = list(itertools.product((0, 1), (0, 1), (0, 1, 2, 3)))


def dev():
    return torch.device("cuda", 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def sources():
    rs = np.random.RandomState(0)
    a = rs.randint(0, 256, size=(37, 53, 3)).astype(np.uint8)             # HWC
    b = rs.randint(0, 256, size=(40, 64, 3)).astype(np.uint8)             # handed over as CHW
    return {"a": (a, torch.from_numpy(a).to(dev()), True),
            "b": (b, torch.from_numpy(np.ascontiguousarray(b.transpose(2, 0, 1))).to(dev()), False)}


def run_views(sources, views, cap_hw):
    """views: [(source key, left, up, win_h, win_w, hflip, vflip, new_h, new_w, rot)] -> (device result, restatement)."""
    from dafne_amd.data.train_views import ViewParams, augment_views
    srcs = [(sources[v[0]][1], sources[v[0]][2]) for v in views]
    windows = [v[1:5] for v in views]
    params = [ViewParams(*v[5:]) for v in views]
    out = torch.full((len(views), 3) + tuple(cap_hw), 0xFF, dtype=torch.uint8, device=dev())
    tb = augment_views(srcs, windows, params, cap_hw=cap_hw, out=out)
    torch.cuda.synchronize()
    want, hw = tv.batch_pixels([(sources[v[0]][0],) + tuple(v[1:]) for v in views], *cap_hw)
    return tb, want, hw


def assert_views(tb, want, hw):
    got = tb.images.cpu().numpy()
    assert np.array_equal(tb.valid_hw.cpu().numpy(), hw) and [tuple(v) for v in tb.valid_hw_host] == [tuple(v) for v in hw.tolist()]
    bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(1))[0]
    assert bad.size == 0, ("views that differ", bad[:8].tolist())


# (left, up, win_h, win_w) per source: inside, overhanging right and bottom (zero pad), the whole image
WINDOWS = {"a": [(4, 6, 30, 40), (30, 20, 30, 40), (0, 0, 37, 53)], "b": [(8, 3, 30, 40), (40, 25, 30, 40), (0, 0, 40, 64)]}


def sizes_for(win_h, win_w):
    return [(win_h, win_w), (35, 51), (70, 90), (max(1, round(win_h * 19 / 53)), max(1, round(win_w * 19 / 53)))]


@pytest.mark.parametrize("key", ["a", "b"])
def test_pixels_every_orientation_and_size(sources, key):
    views = []
    for k, (o, si) in enumerate(itertools.product(ORIENTATIONS, range(4))):
        left, up, wh, ww = WINDOWS[key][k % 3]
        nh, nw = sizes_for(wh, ww)[si]
        views.append((key, left, up, wh, ww, o[0], o[1], nh, nw, o[2]))
    assert len(views) == 64
    tb, want, hw = run_views(sources, views, (96, 100))                     # larger than every view: 0xFF must be gone
    assert_views(tb, want, hw)
    assert {tuple(v) for v in hw.tolist()} >= {(35, 51), (51, 35), (70, 90), (90, 70)}


def test_pixels_downscale_53_to_19_and_mixed_sources(sources):
    views = [("a", 0, 0, 37, 53, hf, vf, 13, 19, rot) for (hf, vf, rot) in ORIENTATIONS]
    views += [("b", 0, 0, 40, 64, hf, vf, 23, 19, rot) for (hf, vf, rot) in ORIENTATIONS]
    tb, want, hw = run_views(sources, views, (32, 24))
    assert_views(tb, want, hw)


def test_pixels_twenty_views_many_axes(sources):
    views = []
    for k in range(20):
        key = "ab"[k % 2]
        wh, ww = 20 + k, 25 + 2 * k % 17 + k
        views.append((key, k % 5, k % 3, wh, ww, k & 1, (k >> 1) & 1, 16 + 3 * k, 70 - 2 * k, k % 4))
    assert len({(v[4], v[8]) for v in views}) > 8 and len({(v[3], v[7]) for v in views}) > 8
    tb, want, hw = run_views(sources, views, (80, 76))
    assert_views(tb, want, hw)


def test_pixels_one_by_one_window(sources):
    for rot in range(4):
        tb, want, hw = run_views(sources, [("a", 7, 5, 1, 1, 1, 1, 1, 1, rot)], (1, 4))
        assert_views(tb, want, hw)
        assert tb.images[0, :, 0, 0].cpu().tolist() == sources["a"][0][5, 7].tolist()
    tb, want, hw = run_views(sources, [("b", 63, 39, 1, 1, 0, 0, 3, 5, 1)], (8, 4))         # ... blown up and turned
    assert_views(tb, want, hw)


def test_pixels_steep_downscale_small_tile_edge():
    """A 25x vertical downscale makes the kernel choose a tile edge below 64 (its LDS rows per output tile grow with the scale)."""
    from dafne_amd.data.train_views import ViewParams, augment_views
    rs = np.random.RandomState(4)
    img = rs.randint(0, 256, size=(1000, 90, 3)).astype(np.uint8)
    t = torch.from_numpy(img).to(dev())
    params = [ViewParams(k & 1, k >> 1 & 1, 40, 70, k) for k in range(4)]
    tb = augment_views([t] * 4, [(0, 0, 1000, 90)] * 4, params, cap_hw=(72, 72))
    want, hw = tv.batch_pixels([(img, 0, 0, 1000, 90) + p.astuple() for p in params], 72, 72)
    assert_views(tb, want, hw)


def test_pixels_refusals_and_repeat(sources):
    from dafne_amd import _lib
    from dafne_amd.data.train_views import ViewParams, augment_views
    t = sources["a"][1]
    one = ([t], [(0, 0, 37, 53)])
    with pytest.raises(_lib.DafneHipError, match="multiple of 4"):
        augment_views(*one, [ViewParams(0, 0, 37, 53, 0)], cap_hw=(40, 54))
    with pytest.raises(_lib.DafneHipError, match="does not fit"):
        augment_views(*one, [ViewParams(0, 0, 37, 53, 1)], cap_hw=(40, 56))          # turned: 53 x 37
    with pytest.raises(_lib.DafneHipError, match="downscale"):
        augment_views(*one, [ViewParams(0, 0, 1, 53, 0)], cap_hw=(40, 56))            # 37 -> 1 needs more than 64 taps
    with pytest.raises(_lib.DafneHipError):
        augment_views([(t, True)], [(0, -1, 37, 53)], [ViewParams(0, 0, 37, 53, 0)])
    with pytest.raises(_lib.DafneHipError):
        augment_views([sources["a"][1].cpu()], [(0, 0, 37, 53)], [ViewParams(0, 0, 37, 53, 0)])
    views = [("a", 2, 3, 30, 41, 1, 0, 35, 51, 1), ("b", 0, 0, 40, 64, 0, 1, 70, 90, 3)]
    x, _, _ = run_views(sources, views, (96, 96))
    y, _, _ = run_views(sources, views, (96, 96))
    assert torch.equal(x.images, y.images) and torch.equal(x.valid_hw, y.valid_hw)
    auto = augment_views([(sources[v[0]][1], sources[v[0]][2]) for v in views], [v[1:5] for v in views],
                         [ViewParams(*v[5:]) for v in views])
    assert tuple(auto.images.shape) == (2, 3, 96, 96)                                  # 51 x 35 and 90 x 70, rounded up to 32s
    assert torch.equal(auto.images, x.images)


# ------------------------------------------------------------------------------------------------ ground truth
def random_gt_case(seed):
    rs = np.random.RandomState(seed)
    n = int(rs.randint(3, 9))
    counts = [0] + [int(rs.randint(0, 151)) for _ in range(n - 2)] + [0]
    counts[1 + seed % (n - 2)] = 150 if seed % 3 == 0 else counts[1 + seed % (n - 2)]
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    G = int(off[-1])
    wins = [(int(rs.randint(20, 1100)), int(rs.randint(20, 1100))) for _ in range(n)]
    views, corners = [], np.zeros((G, 8), np.float32)
    for v, (wh, ww) in enumerate(wins):
        nh, nw = (wh, ww) if rs.rand() < 0.3 else (int(rs.randint(10, 1300)), int(rs.randint(10, 1300)))
        views.append((wh, ww, int(rs.randint(2)), int(rs.randint(2)), nh, nw, int(rs.randint(4))))
        for g in range(off[v], off[v + 1]):
            kind = rs.randint(6)
            cx, cy = rs.uniform(0, ww), rs.uniform(0, wh)
            a, b = rs.uniform(1, 80, size=2)
            if kind == 0:                                   # axis-aligned, integer corners: ties in the sort's argmin
                x0, y0, a, b = np.floor(cx), np.floor(cy), np.ceil(a), np.ceil(b)
                q = [x0, y0, x0 + a, y0, x0 + a, y0 + b, x0, y0 + b]
            elif kind == 1:                                 # no width / no height / a point: dropped
                q = [[cx, cy, cx, cy + a, cx, cy + b, cx, cy - 1], [cx, cy, cx + a, cy, cx + b, cy, cx - 1, cy], [cx, cy] * 4][rs.randint(3)]
            else:
                th = rs.uniform(0, np.pi)
                u, w_ = np.array([np.cos(th), np.sin(th)]) * a / 2, np.array([-np.sin(th), np.cos(th)]) * b / 2
                c = np.array([cx, cy])
                q = np.concatenate([c - u - w_, c + u - w_, c + u + w_, c - u + w_])
                q = np.roll(q.reshape(4, 2), rs.randint(4), axis=0)[::(1 if rs.rand() < 0.5 else -1)].reshape(8)
            corners[g] = q
    classes = rs.randint(0, 15, size=G).astype(np.int32)
    return views, corners, classes, off


def assert_gt(got, want):
    off = got.host_offsets()
    assert np.array_equal(off, want["offsets"]), (off, want["offsets"])
    k = int(off[-1])
    assert np.array_equal(got.src[:k].cpu().numpy(), want["src"])
    assert np.array_equal(got.classes[:k].cpu().numpy(), want["classes"])
    for name in ("corners", "hbox", "area"):
        g, w = bits(getattr(got, name)[:k].cpu().numpy()), bits(want[name])
        assert g.shape == w.shape and np.array_equal(g, w), (name, np.nonzero((g != w).reshape(k, -1).any(1))[0][:8])


@pytest.mark.parametrize("seed", range(20))
def test_gt_seeded_against_restatement(seed):
    from dafne_amd.data.train_views import ViewParams, train_gt
    views, corners, classes, off = random_gt_case(seed)
    windows = [(0, 0, v[0], v[1]) for v in views]
    params = [ViewParams(*v[2:]) for v in views]
    counts = np.diff(off)
    assert counts[0] == 0 and counts[-1] == 0 and (seed % 3 or counts.max() == 150)
    for sort in (True, False):
        got = train_gt(windows, params, corners, classes, off, sort=sort, device=dev())
        want = tv.batch_gt(views, corners, classes, off, sort=sort)
        assert_gt(got, want)
    if seed == 0:
        assert counts.max() > 64 and 0 < want["offsets"][-1] < off[-1]            # a wave boundary inside a view; rows were dropped


def test_gt_golden_cases_equal_the_reference_mapper():
    """The fixture of tests/golden/make_golden_train_views.py (the reference's DAFNeDatasetMapper on build_train_loader's
    augmentation list): all cases of one sort setting in one call, against the fixture itself."""
    from dafne_amd.data.train_views import ViewParams, train_gt
    z = np.load(os.path.join(ROOT, "tests", "golden", "train_views.npz"))
    n = len(z["names"])
    assert n >= 21
    for sort in (1, 0):
        ids = [i for i in range(n) if int(z["case_%d_params" % i][7]) == sort]
        assert ids
        prm = [[int(v) for v in z["case_%d_params" % i]] for i in ids]
        cin = [z["case_%d_corners_in" % i].reshape(-1, 8) for i in ids]
        off = np.concatenate(([0], np.cumsum([c.shape[0] for c in cin]))).astype(np.int32)
        got = train_gt([(0, 0, p[0], p[1]) for p in prm], [ViewParams(*p[2:7]) for p in prm], np.concatenate(cin),
                       np.arange(off[-1]) % 15, off, sort=bool(sort), device=dev())
        want = {k: np.concatenate([z["case_%d_%s" % (i, k)] for i in ids]) for k in ("corners", "hbox", "area")}
        want["src"] = np.concatenate([z["case_%d_src" % i] + off[j] for j, i in enumerate(ids)]).astype(np.int32)
        want["classes"] = (want["src"] % 15).astype(np.int32)
        want["offsets"] = np.concatenate(([0], np.cumsum([z["case_%d_src" % i].shape[0] for i in ids]))).astype(np.int32)
        assert_gt(got, want)


def test_gt_all_dropped_no_objects_and_device_offsets():
    from dafne_amd.data.train_views import ViewParams, train_gt
    flat = np.array([[5, 5, 5, 9, 5, 12, 5, 7]] * 70 + [[5, 5, 9, 5, 12, 5, 7, 5]] * 3, dtype=np.float32)
    off = np.array([0, 70, 70, 73], dtype=np.int32)
    views = [(48, 64, 1, 0, 30, 40, 1), (48, 64, 0, 0, 48, 64, 0), (48, 64, 0, 1, 96, 128, 2)]
    windows, params = [(0, 0, 48, 64)] * 3, [ViewParams(*v[2:]) for v in views]
    got = train_gt(windows, params, flat, np.arange(73), off, device=dev())
    assert got.host_offsets().tolist() == [0, 0, 0, 0]
    got = train_gt(windows, params, np.zeros((0, 8), np.float32), np.zeros(0, np.int32), np.zeros(4, np.int32), device=dev())
    assert got.host_offsets().tolist() == [0, 0, 0, 0]
    # offsets that are already on the device (what F9's kept_offsets are) and an allocation bound above the row count
    views2, corners, classes, off2 = random_gt_case(1)
    pad = np.concatenate([corners, np.full((9, 8), np.nan, np.float32)])
    got = train_gt([(0, 0, v[0], v[1]) for v in views2], [ViewParams(*v[2:]) for v in views2], torch.from_numpy(pad).to(dev()),
                   torch.from_numpy(np.concatenate([classes, np.zeros(9, np.int32)])).to(dev()), torch.from_numpy(off2).to(dev()))
    assert_gt(got, tv.batch_gt(views2, corners, classes, off2))


# ------------------------------------------------------------------------------------------------ end to end
H, W, PATCH, OVERLAP = 400, 330, 256, 64


@pytest.fixture(scope="module")
def e2e():
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    from oracle import model as om
    cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"))
    m = build_model(cfg)
    m.load_state_dict(om.make_params(cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.DAFNE.NUM_CLASSES, seed=5))
    m.to(dev())
    m.invalidate()
    from dafne_amd.evaluation import dota_evaluation as de
    classnames = list(de.CLASSNAMES_DOTA_1_0)
    objs = sl.random_objects(H, W, 25, 7, classnames[:6], side_a=(8, 40), side_b=(8, 20), box=(10, 20, W - 10, 100))
    labels = sl.labels_from_objects([objs], ["S"], classnames)
    scene = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    return {"model": m, "cfg": cfg, "labels": labels, "scene": scene, "classnames": classnames}


def test_identity_parameters_equal_the_unaugmented_route(e2e):
    from dafne_amd.data.loader import inference_resize_shape
    from dafne_amd.data.train_views import ViewParams, scene_train_batches
    from dafne_amd.scene import gather_tiles
    from dafne_amd.scene_labels import split_scene_labels
    m, cfg = e2e["model"], e2e["cfg"]
    scene = e2e["scene"].to(dev())
    sort = bool(cfg.MODEL.DAFNE.SORT_CORNERS_DATALOADER)
    ident = lambda ids: [ViewParams(0, 0, PATCH, PATCH, 0) for _ in ids]      # noqa: E731
    (tb,) = list(scene_train_batches(cfg, [scene], e2e["labels"], batch=8, seed=0, patch_size=PATCH, overlap=OVERLAP,
                                     params_fn=ident, shuffle=False, epochs=1))
    gt = split_scene_labels(e2e["labels"], [(H, W)], PATCH, OVERLAP, min_area=cfg.INPUT.MIN_AREA, min_side=cfg.INPUT.MIN_SIDE,
                            ratio=(1, 1), sort=sort, device=dev())
    kept = gt.kept_counts()
    ids = [t for t in range(4) if kept[t] > 0]
    assert tb.tile_ids == ids and len(ids) == 2
    tiles = gather_tiles([scene], [[(int(gt.origins[t, 0]), int(gt.origins[t, 1])) for t in ids]], PATCH)
    assert tuple(tb.images.shape) == (2, 3, PATCH, PATCH) and torch.equal(tb.images, tiles.permute(0, 3, 1, 2))
    for a, b in zip(tb.instances(), gt.instances(ids)):
        assert len(a) == len(b) > 0
        assert torch.equal(a.gt_corners.view(torch.int32), b.gt_corners.view(torch.int32))
        assert torch.equal(a.gt_boxes.tensor.view(torch.int32), b.gt_boxes.tensor.view(torch.int32))
        assert torch.equal(a.gt_corners_area.view(torch.int32), b.gt_corners_area.view(torch.int32))
        assert torch.equal(a.gt_classes, b.gt_classes)
    # no flip, no turn, the loader's own resize: the losses of validation_losses_scenes, bit for bit
    nh, nw = inference_resize_shape(cfg, PATCH, PATCH)
    assert (nh, nw) != (PATCH, PATCH)
    plain = lambda t: [ViewParams(0, 0, nh, nw, 0) for _ in t]               # noqa: E731
    got = m.augmented_losses_scenes([scene], e2e["labels"], seed=0, patch_size=PATCH, overlap=OVERLAP, batch=3, params_fn=plain,
                                    shuffle=False)
    want = m.validation_losses_scenes([scene], e2e["labels"], patch_size=PATCH, overlap=OVERLAP, batch=3)
    print("augmented route:", got, "validation_losses_scenes:", want)
    assert got["tile_ids"] == want["tile_ids"] and got["tiles"] == want["tiles"]
    for k in want:
        if k.startswith("loss/"):
            assert got[k] == want[k], (k, got[k], want[k])


def test_random_parameters_equal_host_made_batch_and_backward(e2e):
    from dafne_amd.data.targets import make_gt_instances
    from dafne_amd.data.train_views import ViewParams, scene_train_batches
    m, cfg = e2e["model"], e2e["cfg"]
    scene = e2e["scene"].to(dev())
    img = e2e["scene"].numpy()
    sort = bool(cfg.MODEL.DAFNE.SORT_CORNERS_DATALOADER)
    ims = torch.randint(0, 256, (2, 3, 128, 160), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).to(dev())
    rows0, counts0 = m.detect_packed(ims)
    rows0, counts0 = rows0.clone(), counts0.clone()
    rng = np.random.default_rng(21)
    sizes = [(320, 320), (416, 416)]

    def draw(ids):        # seeded; two view sizes in one batch, a flip and a quarter turn among them
        out = [ViewParams(int(rng.random() < 0.5), int(rng.random() < 0.5), *sizes[k % 2], int(rng.integers(4))) for k in range(len(ids))]
        out[0] = ViewParams(1, out[0].vflip, *sizes[0], 1)
        return out
    (tb,) = list(scene_train_batches(cfg, [scene], e2e["labels"], batch=8, seed=21, patch_size=PATCH, overlap=OVERLAP,
                                     filter_empty=False, params_fn=draw, shuffle=True, epochs=1))
    assert len(tb) == 4 and sorted(tb.tile_ids) == [0, 1, 2, 3] and len({p.out_hw() for p in tb.params}) == 2
    assert tuple(tb.images.shape) == (4, 3, 416, 416)
    inputs = tb.batched_inputs()
    got = m.validation_losses(inputs)
    got = {k: float(v) for k, v in got.items()}
    # the TrainBatch itself: the padded slab and the packed rows with their device offsets, no copy
    direct = {k: float(v) for k, v in m.validation_losses(tb).items()}
    assert direct == got, (direct, got)
    # the same batch made on the host: restated pixels, make_gt_instances ground truth
    ref = sl.split_labels(e2e["labels"], [(H, W)], PATCH, OVERLAP, min_area=cfg.INPUT.MIN_AREA, min_side=cfg.INPUT.MIN_SIDE, sort=False)
    host = []
    n_gt = 0
    for t, p, x in zip(tb.tile_ids, tb.params, inputs):
        left, up = [int(v) for v in ref["origins"][t]]
        px = tv.view_pixels(img, left, up, PATCH, PATCH, *p.astuple())
        assert torch.equal(x["image"].cpu(), torch.from_numpy(px.transpose(2, 0, 1)))
        a, b = int(ref["kept_offsets"][t]), int(ref["kept_offsets"][t + 1])
        g = tv.view_gt(ref["kept_corners"][a:b], ref["kept_classes"][a:b], PATCH, PATCH, *p.astuple(), sort=False)
        inst = make_gt_instances(g["corners"], g["classes"], p.out_hw(), sort=sort)
        assert torch.equal(x["instances"].gt_corners.cpu().view(torch.int32), inst.gt_corners.view(torch.int32))
        assert torch.equal(x["instances"].gt_boxes.tensor.cpu().view(torch.int32), inst.gt_boxes.tensor.view(torch.int32))
        assert torch.equal(x["instances"].gt_classes.cpu(), inst.gt_classes)
        n_gt += len(inst)
        host.append({"image": torch.from_numpy(np.ascontiguousarray(px.transpose(2, 0, 1))).to(dev()), "height": PATCH, "width": PATCH,
                     "instances": inst})
    assert n_gt > 0
    want = {k: float(v) for k, v in m.validation_losses(host).items()}
    print("device batch:", got, "host batch:", want)
    assert got == want
    # a backward through losses() on the device batch's ground truth (leaves of the pyramid's shapes)
    outs = m.proposal_generator.dafne_outputs
    shapes = m._last_validation["targets"].shapes
    gen = torch.Generator().manual_seed(9)
    leaf = lambda c: [(torch.randn(len(tb), c, h, w, generator=gen) * 0.1).to(dev()).requires_grad_(True) for h, w in shapes]   # noqa: E731
    lg, co, ce, ct = leaf(outs.num_classes), leaf(8), leaf(2), leaf(1)
    _, losses = outs.losses(lg, co, ce, None, ct, None, tb.instances())
    assert all(v.grad_fn is not None for v in losses.values())
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in lg + co)
    assert any(bool(t.grad.abs().sum() > 0) for t in co)
    rows1, counts1 = m.detect_packed(ims)
    torch.cuda.synchronize()
    assert torch.equal(counts0, counts1) and int(counts0.sum()) > 0
    for i, c in enumerate(counts0.cpu().tolist()):
        assert torch.equal(rows0[i, :c], rows1[i, :c])


def test_refusals(e2e):
    from dafne_amd import _lib
    m = e2e["model"]
    scene = e2e["scene"].to(dev())
    with pytest.raises(_lib.DafneHipError):
        m.augmented_losses_scenes([e2e["scene"]], e2e["labels"], patch_size=PATCH, overlap=OVERLAP)
    with pytest.raises(ValueError):
        m.augmented_losses_scenes([scene, scene], e2e["labels"], patch_size=PATCH, overlap=OVERLAP)
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            m.augmented_losses_scenes([scene], e2e["labels"], patch_size=PATCH, overlap=OVERLAP)
    finally:
        m.eval()


def test_build_train_loader_from_files(tmp_path):
    """Records with "annotations" -> an endless shuffled stream of TrainBatch: pixels and ground truth equal the restatement
    applied to the decoded files with the parameters the batch reports; the same seed gives the same stream."""
    import copy
    from PIL import Image
    from dafne_amd.config import get_cfg
    from dafne_amd.data.train_views import build_train_loader
    cfg = copy.deepcopy(get_cfg())
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN = [40, 56], 70
    rs = np.random.RandomState(8)
    records, images = [], {}
    for k, (h, w) in enumerate([(48, 64), (50, 50), (64, 40)]):
        img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        path = os.path.join(str(tmp_path), "im%d.png" % k)
        Image.fromarray(img[:, :, ::-1]).save(path)                       # the loader reads BGR
        ann = [{"bbox": [5 + k, 6, 30, 8 + k, 28, 25, 4, 20], "category_id": k}, {"bbox": [10, 10, 10, 20, 10, 30, 10, 15], "category_id": 9}]
        records.append({"file_name": path, "image_id": "im%d" % k, "height": h, "width": w, "annotations": ann})
        images[path] = img
    loader = build_train_loader(cfg, records, batch_size=2, seed=4, device=dev(), num_workers=0)
    it = iter(loader)
    batches = [next(it) for _ in range(3)]                                 # one epoch and a half
    again = [tb.params for tb, _ in zip(iter(build_train_loader(cfg, records, batch_size=2, seed=4, device=dev(), num_workers=0)), range(3))]
    assert [tb.params for tb in batches] == again
    assert [len(tb) for tb in batches] == [2, 1, 2]
    order = list(np.random.default_rng(4).permutation(3))
    first = [records[i] for i in order]
    for tb, recs in ((batches[0], first[:2]), (batches[1], first[2:])):
        views = [(images[r["file_name"]], 0, 0, r["height"], r["width"]) + p.astuple() for r, p in zip(recs, tb.params)]
        want, hw = tv.batch_pixels(views, *tb.images.shape[2:])
        assert_views(tb, want, hw)
        corners = np.array([o["bbox"] for r in recs for o in r["annotations"]], dtype=np.float32)
        classes = np.array([o["category_id"] for r in recs for o in r["annotations"]], dtype=np.int32)
        off = np.arange(len(recs) + 1, dtype=np.int32) * 2
        ref = tv.batch_gt([(r["height"], r["width"]) + p.astuple() for r, p in zip(recs, tb.params)], corners, classes, off, sort=True)
        assert_gt(tb.gt, ref)
        assert ref["offsets"].tolist() == list(range(len(recs) + 1))      # the flat box of every record is dropped
        assert all(tuple(x["image"].shape[1:]) == tuple(h) for x, h in zip(tb.batched_inputs(), hw.tolist()))
