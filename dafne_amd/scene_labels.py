"""Scene labels -> the ground truth of every tile of a split scene, on the device.

The reference gets its tile-level training / validation ground truth from an offline chain on files:
  1. tools/prepare_dota/ImgSplit_multi_process.py (splitbase.savepatches, shapely + cv2) cuts every object of a scene's
     labelTxt against every tile of the split and writes <scene>__1__<left>___<up>.txt: objects inside a tile shifted, cut
     objects re-made into four corners (GetPoly4FromPoly5, choose_best_pointorder_fit_another), objects of which <= thresh
     is left marked difficult 2;
  2. DOTA2COCO.py drops the rows marked 2;
  3. dafne/data/datasets/dota.py (load_dota_json) drops rows by INPUT.MIN_AREA / INPUT.MIN_SIDE and rows with coinciding corners.
Here the labels of whole scenes (evaluation.scene_eval.load_scene_labels, what score_scenes reads) go through two launches:
dafne_scene_split_labels_hip, one thread per (tile, object) pair, and dafne_scene_pack_tile_gt_hip, an ordered compaction
per tile.  The packed kept rows are the arrays dafne_assign_targets_hip reads, so OneStageDetector.validation_losses_scenes
gets the loss values of whole scenes without tile files.  Rate 1 only.

  split_scene_labels(labels, sizes, ...)          -> TileGroundTruth
  TileGroundTruth.instances(tile_ids)             Instances per tile for validation_losses (the one host read: the offsets)
  write_tile_labels(gt, scene_names, classnames, dst)   the tile labelTxt files, as savepatches writes them
  validation_losses_scenes(model, scenes, labels, ...)  OneStageDetector.validation_losses_scenes

The definition (operation order, tie rules) is in csrc/scene_labels_kernels.h and DESIGN.md; tests/_scene_labels_np.py restates it.
One deviation from the reference: a non-convex or self-intersecting object (shapely raises on it, or GEOS cuts it into several
parts) gives no row on any tile and is counted in stats["nonconvex"].
"""
import os

import numpy as np
import torch

from . import _lib
from .scene import split_origins
from .structures import Boxes, Instances

OUTCOMES = ("none", "inside", "cut4", "cut5", "dropped_lt4", "dropped_gt5", "nonconvex")
NONE, INSIDE, CUT4, CUT5, DROP_LT4, DROP_GT5, NONCONVEX = range(7)
RECORD = 12


class TileGroundTruth:
    """What split_scene_labels returns; device tensors unless said otherwise.
      origins [T, 2] / tile_scene [T]      host int64: every tile's (left, up) and scene, scenes in call order, split order
      records [P, 12] int32                the dense per-pair result (outcome, 8 coordinates, difficult, kept, 0), tile-major
      pair_offsets [T + 1]                 host int64: tile t owns records[pair_offsets[t]:pair_offsets[t + 1]]
      offsets [T + 1] int32, corners [., 8] int32, classes, difficult int32, src int64        the written rows (ImgSplit's files)
      kept_offsets [T + 1] int32, kept_corners [., 8] f32, kept_hbox [., 4] f32, kept_area f32, kept_classes int32, kept_src int64
                                           the rows kept for training, at the loader's scale (`ratio`)
      stats [9] int32                      OUTCOMES' counts over the pairs, written rows, kept rows (stats_dict() reads them)
    src / kept_src index labels["boxes"].  The row arrays are allocated for P rows; rows past offsets[-1] are unset."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._host_offsets = None

    def host_offsets(self):
        """(offsets, kept_offsets) as host int64 arrays: the one host read, made once."""
        if self._host_offsets is None:
            both = torch.stack([self.offsets, self.kept_offsets]).cpu().numpy().astype(np.int64)
            self._host_offsets = (both[0], both[1])
        return self._host_offsets

    def kept_counts(self):
        return np.diff(self.host_offsets()[1])

    def stats_dict(self):
        v = self.stats.cpu().tolist()
        out = {k: int(x) for k, x in zip(OUTCOMES, v)}
        out["written"], out["kept"] = int(v[7]), int(v[8])
        return out

    def instances(self, tile_ids):
        """One Instances per tile id -- gt_corners, gt_boxes, gt_corners_area, gt_classes as data.targets.make_gt_instances
        forms them, views into the packed device arrays.  Costs the one host read of the offsets (host_offsets)."""
        ko = self.host_offsets()[1]
        out = []
        for t in tile_ids:
            a, b = int(ko[t]), int(ko[t + 1])
            inst = Instances(tuple(self.image_size))
            inst.gt_corners = self.kept_corners[a:b]
            inst.gt_boxes = Boxes(self.kept_hbox[a:b])
            inst.gt_corners_area = self.kept_area[a:b]
            inst.gt_classes = self.kept_classes[a:b].to(torch.int64)
            out.append(inst)
        return out


def scene_object_order(labels):
    """-> (order [G] int64: labels' rows scene by scene in label-file order, obj_off [S + 1], classes [G] int32 of labels' rows)."""
    if "file_index" not in labels:
        raise ValueError("split_scene_labels: the labels carry no \"file_index\" (load them with scene_eval.load_scene_labels)")
    C, S = len(labels["classnames"]), len(labels["scene_names"])
    off = np.asarray(labels["offsets"], dtype=np.int64)
    if off.shape[0] != S * C + 1:
        raise ValueError("split_scene_labels: labels hold %d buckets for %d scenes x %d classes" % (off.shape[0] - 1, S, C))
    bucket = np.repeat(np.arange(S * C, dtype=np.int64), np.diff(off))
    scene = bucket // max(C, 1)
    order = np.lexsort((np.asarray(labels["file_index"], dtype=np.int64), scene))
    obj_off = np.zeros(S + 1, dtype=np.int64)
    obj_off[1:] = np.cumsum(np.bincount(scene, minlength=S)[:S])
    return order, obj_off, (bucket % max(C, 1)).astype(np.int32)


def split_scene_labels(labels, sizes, patch_size=1024, overlap=200, thresh=0.7, min_area=10, min_side=2, ratio=(1, 1), sort=True,
                       device=None):
    """labels: scene_eval.load_scene_labels' dict; sizes: (h, w) per scene, in the labels' scene order.  Tiles are
    split_origins(h, w, patch_size, overlap) with SplitSingle's rectangle [left, min(left + patch, w - 1)] x [up, min(up +
    patch, h - 1)].  min_area / min_side: INPUT.MIN_AREA / INPUT.MIN_SIDE; ratio = (rx, ry) and sort: the loader's resize ratio
    and MODEL.DAFNE.SORT_CORNERS_DATALOADER, applied to the kept rows as data.targets.gt_instances_from_objects applies them.
    -> TileGroundTruth.  Nothing is read back."""
    S = len(labels["scene_names"])
    if len(sizes) != S:
        raise ValueError("split_scene_labels: %d sizes for the labels of %d scenes" % (len(sizes), S))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _lib.DafneHipError("split_scene_labels: the MI355X engine has no CPU path")
    patch = int(patch_size)
    order, obj_off, cls = scene_object_order(labels)
    G = int(order.shape[0])
    tiles, origins, tile_scene = [], [], []
    for s, (h, w) in enumerate(sizes):
        h, w = int(h), int(w)
        for left, up in split_origins(h, w, patch, overlap):
            tiles.append((s, left, up, min(left + patch, w - 1), min(up + patch, h - 1)))
            origins.append((left, up))
            tile_scene.append(s)
    T = len(tiles)
    if T == 0:
        raise ValueError("split_scene_labels: no scenes")
    tile_scene = np.asarray(tile_scene, dtype=np.int64)
    pair_off = np.zeros(T + 1, dtype=np.int64)
    pair_off[1:] = np.cumsum(np.diff(obj_off)[tile_scene])
    P = int(pair_off[-1])
    if P >= 2 ** 31:
        raise ValueError("split_scene_labels: %d (tile, object) pairs overflow the int32 pair index; split the call by scenes" % P)
    rx, ry = (float(ratio), float(ratio)) if np.isscalar(ratio) else (float(ratio[0]), float(ratio[1]))
    diff = np.asarray(labels["difficult_value"] if "difficult_value" in labels else labels["difficult"]).astype(np.int32)
    L = _lib.load()
    n = max(P, 1)
    with torch.cuda.device(dev):
        def up_(a, dtype):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
        d_tiles = up_(np.asarray(tiles, dtype=np.int32).reshape(T, 5), np.int32)
        d_pair = up_(pair_off, np.int32)
        d_obj = up_(obj_off, np.int32)
        d_boxes = up_(np.asarray(labels["boxes"], dtype=np.float64).reshape(-1, 8)[order].reshape(G, 8), np.float64)
        d_diff = up_(diff[order], np.int32)
        d_cls = up_(cls[order], np.int32)
        d_order = up_(order, np.int64)
        if G == 0:          # (the kernels are handed valid pointers even when a call has no objects)
            d_boxes, d_diff, d_cls = (torch.zeros((1, 8), dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                                      torch.zeros(1, dtype=torch.int32, device=dev))
        rec = torch.empty((n, RECORD), dtype=torch.int32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        off_a, off_k = torch.empty(T + 1, **i32), torch.empty(T + 1, **i32)
        a_corners, a_cls, a_diff, a_src = torch.empty((n, 8), **i32), torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(n, **i32)
        k_corners, k_hbox, k_area = torch.empty((n, 8), **f32), torch.empty((n, 4), **f32), torch.empty(n, **f32)
        k_cls, k_src = torch.empty(n, **i32), torch.empty(n, **i32)
        stats = torch.empty(9, **i32)
        st = _lib.current_stream()
        _lib.check(L.dafne_scene_split_labels_hip(_lib.ptr(d_tiles), _lib.ptr(d_pair), T, _lib.ptr(d_obj), S, _lib.ptr(d_boxes),
                                                  _lib.ptr(d_diff), G, patch, float(thresh), float(min_area), float(min_side),
                                                  _lib.ptr(rec), P, st), "dafne_scene_split_labels_hip")
        nbytes = L.dafne_scene_pack_tile_gt_workspace_bytes(T)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(L.dafne_scene_pack_tile_gt_hip(
            _lib.ptr(rec), _lib.ptr(d_pair), _lib.ptr(d_tiles), T, _lib.ptr(d_obj), _lib.ptr(d_cls), rx, ry, int(bool(sort)),
            _lib.ptr(off_a), _lib.ptr(a_corners), _lib.ptr(a_cls), _lib.ptr(a_diff), _lib.ptr(a_src),
            _lib.ptr(off_k), _lib.ptr(k_corners), _lib.ptr(k_hbox), _lib.ptr(k_area), _lib.ptr(k_cls), _lib.ptr(k_src),
            _lib.ptr(stats), _lib.ptr(ws), nbytes, st), "dafne_scene_pack_tile_gt_hip")
        # the kernels' src is a row of the file-ordered objects; hand out rows of labels["boxes"].  Rows past the packed
        # counts are unset: clamp before the gather.
        if G:
            a_src = d_order[a_src.to(torch.int64).clamp_(0, G - 1)]
            k_src = d_order[k_src.to(torch.int64).clamp_(0, G - 1)]
        else:
            a_src, k_src = a_src.to(torch.int64), k_src.to(torch.int64)
    return TileGroundTruth(origins=np.asarray(origins, dtype=np.int64).reshape(T, 2), tile_scene=tile_scene, pair_offsets=pair_off,
                           records=rec[:P], offsets=off_a, corners=a_corners, classes=a_cls, difficult=a_diff, src=a_src,
                           kept_offsets=off_k, kept_corners=k_corners, kept_hbox=k_hbox, kept_area=k_area, kept_classes=k_cls,
                           kept_src=k_src, stats=stats, patch_size=patch, ratio=(rx, ry),
                           image_size=(int(round(patch * ry)), int(round(patch * rx))))


def format_row(row8, name, difficult):
    """savepatches' line (:165-166, :199-204): the coordinates are np.float64 values printed with str(), e.g. 12.0."""
    return " ".join(str(np.float64(v)) for v in row8) + " " + name + " " + str(difficult)


def write_tile_labels(gt, scene_names, classnames, dst):
    """<dst>/<scene>__1__<left>___<up>.txt for every tile (also the empty ones), byte for byte what savepatches writes for the
    rows of `gt`.  -> the file paths in tile order."""
    os.makedirs(dst, exist_ok=True)
    off = gt.host_offsets()[0]
    n = int(off[-1])
    corners = gt.corners[:n].cpu().numpy()
    cls = gt.classes[:n].cpu().numpy()
    diff = gt.difficult[:n].cpu().numpy()
    paths = []
    for t in range(gt.origins.shape[0]):
        path = os.path.join(dst, "%s__1__%d___%d.txt" % (scene_names[int(gt.tile_scene[t])], gt.origins[t, 0], gt.origins[t, 1]))
        with open(path, "w") as f:
            for k in range(int(off[t]), int(off[t + 1])):
                f.write(format_row(corners[k], classnames[int(cls[k])], int(diff[k])) + "\n")
        paths.append(path)
    return paths


def validation_losses_scenes(model, scenes, labels, patch_size=1024, overlap=200, batch=8, layout_hwc=None, filter_empty=True):
    """OneStageDetector.validation_losses_scenes (see there)."""
    from .data.loader import _to_chw_resized, inference_resize_shape
    from .scene import gather_tiles, scene_layout
    if model.training:
        raise NotImplementedError("training is outside the scope of the MI355X inference engine")
    if len(scenes) != len(labels["scene_names"]):
        raise ValueError("validation_losses_scenes: %d scenes, labels of %d scenes" % (len(scenes), len(labels["scene_names"])))
    for img in scenes:
        if not img.is_cuda:
            raise _lib.DafneHipError("validation_losses_scenes: the MI355X engine has no CPU path (got a CPU scene)")
    cfg = model.cfg
    dev = model.device
    patch = int(patch_size)
    sizes = [scene_layout(img, layout_hwc)[:2] for img in scenes]
    nh, nw = inference_resize_shape(cfg, patch, patch)
    gt = split_scene_labels(labels, sizes, patch, overlap, min_area=cfg.INPUT.MIN_AREA, min_side=cfg.INPUT.MIN_SIDE,
                            ratio=(nw / patch, nh / patch), sort=bool(cfg.MODEL.DAFNE.SORT_CORNERS_DATALOADER), device=dev)
    gt.image_size = (nh, nw)
    T = gt.origins.shape[0]
    kept = gt.kept_counts()                                # the one host read
    ids = [t for t in range(T) if not filter_empty or kept[t] > 0]
    if not ids:
        raise ValueError("validation_losses_scenes: no tile with a kept object is left")
    origins = [[] for _ in scenes]
    for t in ids:
        origins[int(gt.tile_scene[t])].append((int(gt.origins[t, 0]), int(gt.origins[t, 1])))
    sums, keys = None, None
    with torch.cuda.device(dev):
        tiles = gather_tiles([x.to(dev) for x in scenes], origins, patch, layout_hwc)       # scene order = ascending tile id
        for b0 in range(0, len(ids), max(1, int(batch))):
            part = ids[b0:b0 + max(1, int(batch))]
            inst = gt.instances(part)
            inputs = []
            for i, g in enumerate(inst):
                x = tiles[b0 + i]
                x = _to_chw_resized(x, nh, nw) if (nh, nw) != (patch, patch) else x.permute(2, 0, 1).contiguous()
                inputs.append({"image": x, "height": patch, "width": patch, "instances": g})
            vals = model.validation_losses(inputs)
            keys = sorted(vals)
            row = torch.stack([vals[k].double() for k in keys]) * len(inputs)
            sums = row if sums is None else sums + row
    mean = (sums / len(ids)).cpu().tolist()
    out = {k: v for k, v in zip(keys, mean)}
    out["tiles"] = len(ids)
    out["tile_ids"] = ids
    return out
