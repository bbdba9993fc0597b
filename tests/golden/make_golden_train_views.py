#!/usr/bin/env python3
"""tests/golden/train_views.npz: RUNS the reference's DAFNeDatasetMapper.__call__ on the augmentation list of build_train_loader.

What runs from /root/reference, unmodified, imported from where it lies:
  DAFNeDatasetMapper.__call__      (dafne/data/datasets/dafne_dataset_mapper.py:13-47): the 8-coordinate polygon check,
                                   filter_empty_instances(by_mask=True), np.stack(...).squeeze(1), the float32 cast,
                                   sort_quadrilateral under MODEL.DAFNE.SORT_CORNERS_DATALOADER, gt_masks.area().float()
  sort_quadrilateral               (dafne/utils/sort_corners.py:26-92)
The augmentation list is built here as tools/plain_train_net.py:229-256 builds it (hflip, vflip, ResizeShortestEdge,
RandomRotation); that file itself imports detectron2's engine and is not loaded.

What is a stand-in (detectron2 v0.5 / fvcore are not installed; their semantics are [recalled]):
  DatasetMapper.__call__ (apply the augmentations, transform_instance_annotations, annotations_to_instances with polygon
  masks, filter_empty_instances by box), RandomFlip / ResizeShortestEdge / RandomRotation (draws from the global np.random),
  HFlip / VFlip / Resize / RotationTransform.apply_coords in float64, PolygonMasks (iteration, nonempty, area =
  0.5 |dot(x, roll(y, 1)) - dot(y, roll(x, 1))|), Boxes.nonempty(1e-5), filter_empty_instances.  No image is read: the
  fixture pins coordinates, filtering, order, sorting, area and dtypes, not pixels (those are pinned to PIL live).
  RotationTransform uses the float64 matrix of cv2.getRotationMatrix2D (cos / sin of the angle in radians, the centre offset
  of expand=True) [recalled; cv2 is not installed].  The project pins the quarter turn to the exact permutation instead; this
  maker ASSERTS that on its inputs both forms give the same float32 corners and the same float32 area, and refuses to write
  the fixture otherwise (pick another SEED then: 808 - 810 each fail on one coordinate that sits on a float32 rounding tie, 811 passes).

The fixture holds numbers only.  Usage: python tests/golden/make_golden_train_views.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

SEED = 811
EXACT_ROTATION = False        # the second pass of main() turns it on: the same cases through the exact permutation


# ------------------------------------------------------------------ transforms (fvcore / d2 [recalled])
class HFlipTransform:
    def __init__(self, width):
        self.width = width

    def apply_coords(self, c):
        c[:, 0] = self.width - c[:, 0]
        return c


class VFlipTransform:
    def __init__(self, height):
        self.height = height

    def apply_coords(self, c):
        c[:, 1] = self.height - c[:, 1]
        return c


class NoOpTransform:
    def apply_coords(self, c):
        return c


class ResizeTransform:
    def __init__(self, h, w, new_h, new_w):
        self.h, self.w, self.new_h, self.new_w = h, w, new_h, new_w

    def apply_coords(self, c):
        c[:, 0] = c[:, 0] * (self.new_w * 1.0 / self.w)
        c[:, 1] = c[:, 1] * (self.new_h * 1.0 / self.h)
        return c


class RotationTransform:
    """expand=True, center=None: the matrix of cv2.getRotationMatrix2D((w / 2, h / 2), angle, 1) moved to the new centre."""

    def __init__(self, h, w, angle):
        self.h, self.w, self.angle = h, w, angle
        a = np.deg2rad(angle)
        ca, sa = np.cos(a), np.sin(a)
        self.bound_w, self.bound_h = np.rint([h * abs(sa) + w * abs(ca), h * abs(ca) + w * abs(sa)]).astype(int)
        cx, cy = w / 2.0, h / 2.0
        rm = np.array([[ca, sa, (1 - ca) * cx - sa * cy], [-sa, ca, sa * cx + (1 - ca) * cy]], dtype=np.float64)
        rot_center = rm[:, :2] @ np.array([cx, cy]) + rm[:, 2]
        rm[:, 2] += np.array([self.bound_w / 2.0, self.bound_h / 2.0]) - rot_center
        self.rm = rm

    def apply_coords(self, c):
        c = np.asarray(c, dtype=float)
        if EXACT_ROTATION:
            k = int(round(self.angle / 90.0)) % 4
            x, y = c[:, 0].copy(), c[:, 1].copy()
            W, H = float(self.w), float(self.h)
            if k == 1:
                x, y = y, W - x
            elif k == 2:
                x, y = W - x, H - y
            elif k == 3:
                x, y = H - y, x
            return np.stack((x, y), axis=1)
        return c @ self.rm[:, :2].T + self.rm[:, 2]


class TransformList:
    def __init__(self, ts):
        self.transforms = ts

    def apply_coords(self, c):
        for t in self.transforms:
            c = t.apply_coords(c)
        return c

    def apply_box(self, box):
        idx = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
        c = np.asarray(box, dtype=np.float64).reshape(-1, 4)[:, idx].reshape(-1, 2)
        c = self.apply_coords(c).reshape((-1, 4, 2))
        return np.concatenate((c.min(axis=1), c.max(axis=1)), axis=1)

    def apply_polygons(self, polys):
        return [self.apply_coords(p) for p in polys]


# ------------------------------------------------------------------ augmentations (d2 [recalled]): global np.random
class RandomFlip:
    def __init__(self, prob=0.5, *, horizontal=True, vertical=False):
        self.prob, self.horizontal, self.vertical = prob, horizontal, vertical

    def get_transform(self, hw):
        h, w = hw
        if np.random.uniform() < self.prob:
            return HFlipTransform(w) if self.horizontal else VFlipTransform(h)
        return NoOpTransform()


class ResizeShortestEdge:
    def __init__(self, short_edge_length, max_size=sys.maxsize, sample_style="range"):
        self.is_range = sample_style == "range"
        self.sizes = (short_edge_length, short_edge_length) if isinstance(short_edge_length, int) else short_edge_length
        self.max_size = max_size

    def get_transform(self, hw):
        h, w = hw
        size = np.random.randint(self.sizes[0], self.sizes[1] + 1) if self.is_range else np.random.choice(self.sizes)
        if size == 0:
            return NoOpTransform()
        scale = size * 1.0 / min(h, w)
        newh, neww = (size, scale * w) if h < w else (scale * h, size)
        if max(newh, neww) > self.max_size:
            scale = self.max_size * 1.0 / max(newh, neww)
            newh, neww = newh * scale, neww * scale
        return ResizeTransform(h, w, int(newh + 0.5), int(neww + 0.5))


class RandomRotation:
    def __init__(self, angle, expand=True, center=None, sample_style="range", interp=None):
        assert sample_style == "choice" and expand and center is None
        self.angle = angle

    def get_transform(self, hw):
        h, w = hw
        angle = np.random.choice(self.angle)
        if angle % 360 == 0:
            return NoOpTransform()
        return RotationTransform(h, w, angle)


def out_hw(hw, t):
    if isinstance(t, ResizeTransform):
        return (t.new_h, t.new_w)
    if isinstance(t, RotationTransform):
        return (int(t.bound_h), int(t.bound_w))
    return hw


# ------------------------------------------------------------------ structures (d2 [recalled])
class Boxes(mg.Boxes):
    def __getitem__(self, i):
        return Boxes(self.tensor[i].reshape(-1, 4))

    def nonempty(self, threshold=0.0):
        box = self.tensor
        return ((box[:, 2] - box[:, 0]) > threshold) & ((box[:, 3] - box[:, 1]) > threshold)


def polygon_area(x, y):
    return 0.5 * np.abs(np.dot(x, np.roll(y, 1)) - np.dot(y, np.roll(x, 1)))


class PolygonMasks:
    def __init__(self, polygons):
        self.polygons = [[np.asarray(p, dtype=np.float64) for p in per] for per in polygons]

    def __len__(self):
        return len(self.polygons)

    def __iter__(self):
        return iter(self.polygons)

    def __getitem__(self, item):
        if isinstance(item, torch.Tensor) and item.dtype == torch.bool:
            item = item.nonzero().squeeze(1).tolist()
        return PolygonMasks([self.polygons[i] for i in item])

    def nonempty(self):
        return torch.from_numpy(np.asarray([1 if len(per) > 0 else 0 for per in self.polygons], dtype=bool))

    def area(self):
        return torch.tensor([sum(polygon_area(p[0::2], p[1::2]) for p in per) for per in self.polygons])


def filter_empty_instances(instances, by_box=True, by_mask=True, box_threshold=1e-5):
    r = []
    if by_box:
        r.append(instances.gt_boxes.nonempty(threshold=box_threshold))
    if instances.has("gt_masks") and by_mask:
        r.append(instances.gt_masks.nonempty())
    if not r:
        return instances
    m = r[0]
    for x in r[1:]:
        m = m & x
    return instances[m]


class DatasetMapper:
    def __init__(self, cfg, is_train=True, use_instance_mask=False, augmentations=()):
        self.is_train, self.use_instance_mask, self.augmentations = is_train, use_instance_mask, list(augmentations)

    def __call__(self, dataset_dict):
        d = dict(dataset_dict)
        hw = (d["height"], d["width"])
        ts = []
        for a in self.augmentations:
            t = a.get_transform(hw)
            hw = out_hw(hw, t)
            ts.append(t)
        tl = TransformList(ts)
        d["transforms"] = ts
        d["image_hw"] = hw
        boxes, classes, polys = [], [], []
        for o in d.pop("annotations"):
            bbox = np.minimum(tl.apply_box(np.array([o["bbox"]]))[0].clip(min=0), list(hw + hw)[::-1])
            boxes.append(bbox)
            classes.append(int(o["category_id"]))
            polys.append([p.reshape(-1) for p in tl.apply_polygons([np.asarray(p, dtype=np.float64).reshape(-1, 2)
                                                                     for p in o["segmentation"]])])
        inst = mg.Instances(hw)
        inst.gt_boxes = Boxes(torch.as_tensor(np.asarray(boxes, dtype=np.float64).reshape(-1, 4), dtype=torch.float32))
        inst.gt_classes = torch.tensor(classes, dtype=torch.int64)
        inst.gt_masks = PolygonMasks(polys)
        d["instances"] = filter_empty_instances(inst)
        return d


# ------------------------------------------------------------------ cases
def objects(rng, h, w, kinds):
    rows = []
    for kind in kinds:
        cx, cy = rng.uniform(0.25 * w, 0.75 * w), rng.uniform(0.25 * h, 0.75 * h)
        a, b = rng.uniform(4, 0.2 * w), rng.uniform(3, 0.2 * h)
        if kind == "rect":                    # axis-aligned, integer corners: ties in sort_quadrilateral's argmin
            x0, y0, a, b = np.floor(cx), np.floor(cy), np.ceil(a), np.ceil(b)
            q = [x0, y0, x0 + a, y0, x0 + a, y0 + b, x0, y0 + b]
        elif kind == "zero_w":
            q = [cx, cy, cx, cy + b, cx, cy + 2 * b, cx, cy + b / 2]
        elif kind == "zero_h":
            q = [cx, cy, cx + a, cy, cx + 2 * a, cy, cx + a / 2, cy]
        else:
            th = rng.uniform(0, np.pi)
            u, v = np.array([np.cos(th), np.sin(th)]) * a, np.array([-np.sin(th), np.cos(th)]) * b
            c = np.array([cx, cy])
            q = np.concatenate([c - u - v, c + u - v, c + u + v, c - u + v])
            q = np.roll(q.reshape(4, 2), int(rng.integers(4)), axis=0)[::(1 if rng.random() < 0.5 else -1)].reshape(8)
        rows.append(np.asarray(q, dtype=np.float32))
    return np.asarray(rows, dtype=np.float32).reshape(-1, 8)


def run_case(mapper_cls, cfg, h, w, corners, sizes, max_size, angles, seed):
    augs = [RandomFlip(prob=0.5, horizontal=True, vertical=False), RandomFlip(prob=0.5, horizontal=False, vertical=True),
            ResizeShortestEdge(sizes, max_size, "choice")]
    if len(angles) > 0:
        augs.append(RandomRotation(sample_style="choice", angle=angles))
    mapper = mapper_cls(cfg, is_train=True, use_instance_mask=True, augmentations=augs)
    ann = []
    for i, q in enumerate(corners):
        q64 = [float(v) for v in q]
        ann.append({"bbox": [min(q64[0::2]), min(q64[1::2]), max(q64[0::2]), max(q64[1::2])], "bbox_mode": 0,
                    "category_id": i, "segmentation": [q64]})
    np.random.seed(seed)
    out = mapper({"height": h, "width": w, "annotations": ann})
    ts = out["transforms"]
    hf, vf = int(isinstance(ts[0], HFlipTransform)), int(isinstance(ts[1], VFlipTransform))
    nh, nw = (ts[2].new_h, ts[2].new_w) if isinstance(ts[2], ResizeTransform) else (h, w)
    rot = int(round(ts[3].angle / 90.0)) % 4 if len(ts) > 3 and isinstance(ts[3], RotationTransform) else 0
    inst = out["instances"]
    return (hf, vf, nh, nw, rot), {"corners": inst.gt_corners.numpy().reshape(-1, 8), "hbox": inst.gt_boxes.tensor.numpy().reshape(-1, 4),
                                   "area": inst.gt_corners_area.numpy().reshape(-1), "src": inst.gt_classes.numpy().reshape(-1),
                                   "image_hw": out["image_hw"]}


def make(mapper_cls):
    rng = np.random.default_rng(SEED)
    H, W = 96, 120
    angles = [0.0, 90.0, 180.0, 270.0]
    cases = []
    cfg_on = mg.AttrDict({"MODEL": {"DAFNE": {"SORT_CORNERS_DATALOADER": True}}})
    cfg_off = mg.AttrDict({"MODEL": {"DAFNE": {"SORT_CORNERS_DATALOADER": False}}})
    kinds = ["rect", "quad", "zero_w", "quad", "zero_h", "rect", "quad"]
    seen, seed = set(), SEED * 1000
    while len(seen) < 16:                       # all 16 (hflip, vflip, rot) combinations at one size
        corners = objects(rng, H, W, kinds)
        p, out = run_case(mapper_cls, cfg_on, H, W, corners, [96], 4000, angles, seed)
        seed += 1
        if (p[0], p[1], p[4]) in seen:
            continue
        seen.add((p[0], p[1], p[4]))
        cases.append(("o%d%d%d" % (p[0], p[1], p[4]), H, W, corners, p, 1, out))
    for name, size in (("up", 131), ("down", 48), ("nondyadic", 70)):
        corners = objects(rng, H, W, kinds + ["quad"] * 3)
        p, out = run_case(mapper_cls, cfg_on, H, W, corners, [size], 4000, angles, seed)
        seed += 1
        cases.append((name, H, W, corners, p, 1, out))
    corners = objects(rng, H, W, kinds)
    p, out = run_case(mapper_cls, cfg_on, H, W, corners, [300], 333, angles, seed)       # MAX_SIZE_TRAIN bites
    cases.append(("maxsize", H, W, corners, p, 1, out))
    p, out = run_case(mapper_cls, cfg_on, H, W, np.zeros((0, 8), np.float32), [70], 4000, angles, seed + 1)
    cases.append(("empty", H, W, np.zeros((0, 8), np.float32), p, 1, out))
    corners = objects(rng, H, W, kinds)
    p, out = run_case(mapper_cls, cfg_off, H, W, corners, [70], 4000, angles, seed + 2)
    cases.append(("unsorted", H, W, corners, p, 0, out))
    return cases


def main():
    global EXACT_ROTATION
    assert os.path.isdir(mg.REF)
    mg.install_stubs()
    mg._mod("detectron2.config", configurable=lambda f=None, **kw: f)
    mg._mod("detectron2.data", DatasetMapper=DatasetMapper)
    mg._mod("detectron2.data.detection_utils", filter_empty_instances=filter_empty_instances)
    mg._mod("detectron2.structures.instances", Instances=mg.Instances)
    for pkg in ("dafne.data", "dafne.data.datasets"):
        m = mg._mod(pkg)
        m.__path__ = [os.path.join(mg.REF, *pkg.split("."))]
    mg.load_ref("dafne.utils.sort_corners")
    mapper_mod = mg.load_ref("dafne.data.datasets.dafne_dataset_mapper")
    cases = make(mapper_mod.DAFNeDatasetMapper)
    EXACT_ROTATION = True
    exact = make(mapper_mod.DAFNeDatasetMapper)
    res = {"names": np.array([c[0] for c in cases])}
    for i, (a, b) in enumerate(zip(cases, exact)):
        name, h, w, corners, p, sort, out = a
        assert p == b[4] and np.array_equal(corners, b[3])
        for k in ("corners", "hbox", "area", "src"):       # the matrix form and the exact permutation: the same float32 bits
            assert np.array_equal(out[k].view(np.int32) if out[k].dtype == np.float32 else out[k],
                                  b[6][k].view(np.int32) if out[k].dtype == np.float32 else b[6][k]), (name, k, "pick another SEED")
        oh, ow = (p[3], p[2]) if p[4] & 1 else (p[2], p[3])
        assert tuple(out["image_hw"]) == (oh, ow), (name, out["image_hw"], p)
        res["case_%d_params" % i] = np.array([h, w, p[0], p[1], p[2], p[3], p[4], sort], dtype=np.int64)
        res["case_%d_corners_in" % i] = corners
        for k in ("corners", "hbox", "area"):
            assert out[k].dtype == np.float32
            res["case_%d_%s" % (i, k)] = out[k]
        res["case_%d_src" % i] = out["src"].astype(np.int64)
        print("train_views", name, "params", p, "objects", corners.shape[0], "kept", out["src"].shape[0])
    assert {c[0] for c in cases} >= {"o%d%d%d" % (a, b, r) for a in (0, 1) for b in (0, 1) for r in range(4)}
    np.savez_compressed(os.path.join(HERE, "train_views.npz"), **res)


if __name__ == "__main__":
    main()
