"""Ground truth for DAFNeOutputs' target assignment, as the reference's training contract carries it.

The reference's DAFNeDatasetMapper hands every image an ``Instances`` with ``gt_corners`` (sorted by
dafne/utils/sort_corners.py when INPUT / MODEL.DAFNE.SORT_CORNERS_DATALOADER), ``gt_boxes`` (the hull),
``gt_corners_area`` (detectron2's PolygonMasks.area: the shoelace formula) and ``gt_classes``
(dafne/data/dataset_mapper.py); ``compute_targets_for_locations`` reads exactly those four.  This module builds them on
the host from plain corner arrays (the loader's scale), with numpy only.
"""
import numpy as np
import torch

from ..structures import Boxes, Instances


def _cross(a, b):
    return a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]


def sort_quadrilateral_np(boxes):
    """dafne.utils.sort_corners.sort_quadrilateral on the host: [n, 8] -> [n, 8] float32, the same selection the device
    function makes (csrc/sort_quad.h), with its fp32 cross products."""
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 8)
    n = b.shape[0]
    if n == 0:
        return b.copy()
    S = b.reshape(n, 4, 2)
    ar = np.arange(n)
    k1 = np.argmin(S[:, :, 0], axis=1)               # the first vertex of minimal x
    p1 = S[ar, k1]
    keep = np.ones((n, 4), bool)
    keep[ar, k1] = False
    R = S[keep].reshape(n, 3, 2)
    p3, A, B = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
    done = np.zeros(n, bool)
    for i in range(3):
        i2, i3 = (1 if i == 0 else 0), (1 if i == 2 else 2)
        d = R[:, i] - p1
        cond = ((_cross(d, R[:, i2] - p1) * _cross(d, R[:, i3] - p1)) < 0) & ~done
        p3[cond], A[cond], B[cond] = R[cond, i], R[cond, i2], R[cond, i3]
        done |= cond
    e = p3 - p1
    swap = ~(_cross(e, A - p1) > 0) & (_cross(e, B - p1) > 0)
    p2 = np.where(swap[:, None], B, A)
    p4 = np.where(swap[:, None], A, B)
    return np.stack((p1, p2, p3, p4), axis=1).reshape(n, 8)


def polygon_area(corners):
    """Shoelace area of [n, 8] quadrilaterals in fp64, rounded to fp32: 0.5 |sum x_i y_(i+1) - x_(i+1) y_i|."""
    c = np.asarray(corners, dtype=np.float64).reshape(-1, 4, 2)
    x, y = c[:, :, 0], c[:, :, 1]
    a = 0.5 * np.abs(np.sum(x * np.roll(y, -1, axis=1), axis=1) - np.sum(y * np.roll(x, -1, axis=1), axis=1))
    return a.astype(np.float32)


def make_gt_instances(corners, classes, image_size, sort=True):
    """corners [G, 8] (x0, y0, .., x3, y3 at the network's input scale), classes [G] -> Instances(image_size) with gt_corners
    (sorted when ``sort``: cfg.MODEL.DAFNE.SORT_CORNERS_DATALOADER), gt_boxes (min / max of the corners), gt_corners_area and
    gt_classes, host tensors."""
    c = np.ascontiguousarray(np.asarray(corners, dtype=np.float32).reshape(-1, 8))
    cls = np.asarray(classes, dtype=np.int64).reshape(-1)
    if cls.shape[0] != c.shape[0]:
        raise ValueError("make_gt_instances: %d boxes, %d classes" % (c.shape[0], cls.shape[0]))
    if sort:
        c = sort_quadrilateral_np(c)
    xs, ys = c[:, 0::2], c[:, 1::2]
    if c.shape[0]:
        hbox = np.stack((xs.min(1), ys.min(1), xs.max(1), ys.max(1)), axis=1)
    else:
        hbox = np.zeros((0, 4), np.float32)
    inst = Instances(tuple(int(v) for v in image_size))
    inst.gt_corners = torch.from_numpy(c)
    inst.gt_boxes = Boxes(torch.from_numpy(np.ascontiguousarray(hbox)))
    inst.gt_corners_area = torch.from_numpy(polygon_area(c))
    inst.gt_classes = torch.from_numpy(cls)
    return inst


def gt_instances_from_objects(objects, classnames, image_size, ratio=1.0, sort=True, skip_difficult=False):
    """dota_evaluation.parse_gt objects ({"name", "difficult", "bbox": 8 floats}) of one image -> make_gt_instances, the
    corners multiplied by the loader's resize ``ratio`` (a number, or (ratio_x, ratio_y)).  Objects of a class outside
    ``classnames`` are dropped."""
    rx, ry = (ratio, ratio) if np.isscalar(ratio) else ratio
    index = {n: i for i, n in enumerate(classnames)}
    rows, cls = [], []
    for o in objects:
        if o["name"] not in index or (skip_difficult and o.get("difficult", 0)):
            continue
        b = np.asarray(o["bbox"], dtype=np.float64).reshape(4, 2) * np.array([rx, ry], dtype=np.float64)
        rows.append(b.reshape(8))
        cls.append(index[o["name"]])
    c = np.asarray(rows, dtype=np.float32).reshape(-1, 8)
    return make_gt_instances(c, np.asarray(cls, dtype=np.int64), image_size, sort=sort)
