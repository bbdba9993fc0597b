"""The batch the reference trains on, made on the device: random flips, ResizeShortestEdge / Resize, quarter turns, and the
ground truth that follows the pixels.

Reference: `build_train_loader` (tools/plain_train_net.py:219-277) puts every image through
    T.RandomFlip(horizontal, p = 0.5), T.RandomFlip(vertical, p = 0.5),
    T.ResizeShortestEdge(MIN_SIZE_TRAIN, MAX_SIZE_TRAIN, MIN_SIZE_TRAIN_SAMPLING) | T.Resize((RESIZE_HEIGHT_TRAIN, RESIZE_WIDTH_TRAIN)),
    T.RandomRotation(ROTATION_AUG_ANGLES, sample_style=ROTATION_AUG_SAMPLE_STYLE)
and `DAFNeDatasetMapper` (dafne/data/datasets/dafne_dataset_mapper.py:13-47) rebuilds the ground truth from the transformed
polygons: empty instances filtered, sort_quadrilateral, the shoelace area.

Here a *view* is (source, window, hflip, vflip, (new_h, new_w), rot); rot counts quarter turns counter-clockwise (detectron2's
RandomRotation / cv2.getRotationMatrix2D for a positive angle).  One launch of dafne_train_views_u8_hip writes a whole batch of
views of mixed sizes, zero padded (ImageList's padding); dafne_train_gt_hip transforms, filters, sorts and packs their ground
truth in the layout dafne_assign_targets_hip reads.  The definition is DESIGN.md row F10; tests/_train_views_np.py restates it.
The quarter turn is the exact permutation (np.rot90): detectron2's route through cv2.warpAffine is not pinned by the reference
tree, and for multiples of 90 degrees with expand=True it is the same permutation up to cv2's interpolation rounding.

  TrainAugmentation(cfg).sample(windows_hw, rng)    per-view parameters from a numpy Generator the caller seeds
  augment_views(sources, windows, params, gt=None)  -> TrainBatch
  train_gt(params_views, corners, classes, offsets) the packed ground truth of a batch of views
  scene_train_batches(cfg, scenes, labels, ...)     batches of augmented tiles cut from scenes, with their ground truth
  DAFNeTrainMapper / build_train_loader             the file-based stream (records with "annotations")

The random stream is THIS repository's: per view, in this order, hflip (rng.random() < 0.5), vflip (rng.random() < 0.5), the
size (choice: rng.integers(len(sizes)); range: rng.integers(lo, hi + 1); RESIZE_TYPE both draws nothing), the angle
(rng.integers(len(angles)), nothing without angles).  detectron2 draws from the global np.random in its own order.
"""
import numpy as np
import torch

from .. import _lib
from ..structures import Boxes, Instances
from .loader import shortest_edge_size

__all__ = ["TrainAugmentation", "TrainBatch", "ViewParams", "augment_views", "train_gt", "scene_train_batches", "DAFNeTrainMapper",
           "build_train_loader"]


class ViewParams:
    """hflip, vflip 0 / 1; (new_h, new_w) the resize target of the (flipped) window; rot quarter turns counter-clockwise."""
    __slots__ = ("hflip", "vflip", "new_h", "new_w", "rot")

    def __init__(self, hflip=0, vflip=0, new_h=0, new_w=0, rot=0):
        self.hflip, self.vflip, self.new_h, self.new_w, self.rot = int(bool(hflip)), int(bool(vflip)), int(new_h), int(new_w), int(rot) % 4

    def out_hw(self):
        return (self.new_w, self.new_h) if self.rot & 1 else (self.new_h, self.new_w)

    def astuple(self):
        return (self.hflip, self.vflip, self.new_h, self.new_w, self.rot)

    def __repr__(self):
        return "ViewParams(hflip=%d, vflip=%d, new_h=%d, new_w=%d, rot=%d)" % self.astuple()

    def __eq__(self, other):
        return isinstance(other, ViewParams) and self.astuple() == other.astuple()


class TrainAugmentation:
    """The random part of build_train_loader's augmentation list (see the module text for the draw order)."""

    def __init__(self, cfg):
        inp = cfg.INPUT
        if bool(inp.USE_COLOR_AUGMENTATIONS):
            raise NotImplementedError("INPUT.USE_COLOR_AUGMENTATIONS: the colour augmentations have no device form (no released config sets it)")
        self.resize_type = str(inp.RESIZE_TYPE)
        if self.resize_type == "shortest-edge":
            sizes = inp.MIN_SIZE_TRAIN
            self.min_sizes = [int(s) for s in (sizes if isinstance(sizes, (list, tuple)) else [sizes])]
            self.max_size = int(inp.MAX_SIZE_TRAIN)
            self.sampling = str(inp.get("MIN_SIZE_TRAIN_SAMPLING", "choice"))          # detectron2's default
            if self.sampling not in ("choice", "range"):
                raise ValueError("INPUT.MIN_SIZE_TRAIN_SAMPLING %r (choice or range)" % (self.sampling,))
            if self.sampling == "range" and len(self.min_sizes) != 2:
                raise ValueError("INPUT.MIN_SIZE_TRAIN_SAMPLING range needs two sizes, got %r" % (self.min_sizes,))
            if not self.min_sizes:
                raise ValueError("INPUT.MIN_SIZE_TRAIN is empty")
        elif self.resize_type == "both":
            self.fixed_hw = (int(inp.RESIZE_HEIGHT_TRAIN), int(inp.RESIZE_WIDTH_TRAIN))
            if min(self.fixed_hw) <= 0:
                raise ValueError("INPUT.RESIZE_TYPE 'both' needs INPUT.RESIZE_HEIGHT_TRAIN / RESIZE_WIDTH_TRAIN")
        else:
            raise RuntimeError("Invalid resize-type: %s" % (self.resize_type,))
        if str(inp.ROTATION_AUG_SAMPLE_STYLE) != "choice":
            raise NotImplementedError("INPUT.ROTATION_AUG_SAMPLE_STYLE %r: only quarter turns have a device form (no released config "
                                      "samples a range)" % (inp.ROTATION_AUG_SAMPLE_STYLE,))
        self.rots = []
        for a in inp.ROTATION_AUG_ANGLES:
            q = float(a) / 90.0
            if q != int(q):
                raise NotImplementedError("INPUT.ROTATION_AUG_ANGLES %r: only multiples of 90 degrees have a device form" % (a,))
            self.rots.append(int(q) % 4)

    def output_size(self, h, w, size=None):
        if self.resize_type == "both":
            return self.fixed_hw
        if int(size) == 0:                       # detectron2: size 0 disables the resize
            return int(h), int(w)
        return shortest_edge_size(int(h), int(w), int(size), self.max_size)

    def sample(self, windows_hw, rng):
        """windows_hw: (win_h, win_w) per view; rng: numpy.random.Generator -> [ViewParams]."""
        out = []
        for h, w in windows_hw:
            hf = int(rng.random() < 0.5)
            vf = int(rng.random() < 0.5)
            if self.resize_type == "both":
                nh, nw = self.fixed_hw
            else:
                if self.sampling == "choice":
                    size = self.min_sizes[int(rng.integers(len(self.min_sizes)))]
                else:
                    size = int(rng.integers(self.min_sizes[0], self.min_sizes[1] + 1))
                nh, nw = self.output_size(h, w, size)
            rot = self.rots[int(rng.integers(len(self.rots)))] if self.rots else 0
            out.append(ViewParams(hf, vf, nh, nw, rot))
        return out


def _view_array(windows, params, sources=None):
    n = len(params)
    arr = (_lib.TrainView * n)()
    keep = []
    for k, ((left, up, wh, ww), p) in enumerate(zip(windows, params)):
        a = arr[k]
        if sources is not None:
            from ..scene import scene_layout
            img, hwc = sources[k]
            h, w, hwc = scene_layout(img, hwc)
            img = img.contiguous()
            keep.append(img)
            a.d_src, a.h, a.w, a.layout_hwc = img.data_ptr(), h, w, int(hwc)
        a.left, a.up, a.win_h, a.win_w = int(left), int(up), int(wh), int(ww)
        a.hflip, a.vflip, a.new_h, a.new_w, a.rot = p.hflip, p.vflip, p.new_h, p.new_w, p.rot
    return arr, keep


class PackedGT:
    """dafne_train_gt_hip's outputs, device tensors: corners [G, 8], hbox [G, 4], area [G] f32, classes [G] int32, offsets
    [N + 1] int32, src [G] int32 (the input row of every kept row).  Rows past offsets[-1] are unset."""

    def __init__(self, corners, hbox, area, classes, offsets, src):
        self.corners, self.hbox, self.area, self.classes, self.offsets, self.src = corners, hbox, area, classes, offsets, src
        self._host = None

    def host_offsets(self):
        if self._host is None:
            self._host = self.offsets.cpu().numpy().astype(np.int64)          # the one host read
        return self._host


def train_gt(windows, params, corners, classes, offsets, sort=True, device=None):
    """windows: (left, up, win_h, win_w) per view (the origin is not read: the corners are at window scale); corners [G, 8]
    f32, classes [G] int32, offsets [N + 1] int32 -- device tensors (host arrays are uploaded) -> PackedGT.  Nothing is read back."""
    L = _lib.load()
    n = len(params)
    if n == 0 or len(windows) != n:
        raise ValueError("train_gt: %d views, %d windows" % (n, len(windows)))
    dev = device
    if dev is None:
        dev = corners.device if torch.is_tensor(corners) and corners.is_cuda else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise _lib.DafneHipError("train_gt: the MI355X engine has no CPU path")

    def up_(a, dtype, shape):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
        return t.to(device=dev, dtype=dtype).reshape(shape).contiguous()
    corners = up_(corners, torch.float32, (-1, 8))
    classes = up_(classes, torch.int32, (-1,))
    offsets = up_(offsets, torch.int32, (-1,))
    G = int(corners.shape[0])
    if classes.shape[0] != G or offsets.shape[0] != n + 1:
        raise ValueError("train_gt: %d corner rows, %d classes, %d offsets for %d views" % (G, classes.shape[0], offsets.shape[0], n))
    arr, _ = _view_array(windows, params)
    with torch.cuda.device(dev):
        m = max(G, 1)
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        o_c, o_h, o_a = torch.empty((m, 8), **f32), torch.empty((m, 4), **f32), torch.empty(m, **f32)
        o_k, o_s, o_off = torch.empty(m, **i32), torch.empty(m, **i32), torch.empty(n + 1, **i32)
        nbytes = L.dafne_train_gt_workspace_bytes(n, G)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.check(L.dafne_train_gt_hip(arr, n, _lib.ptr(corners), _lib.ptr(classes), _lib.ptr(offsets), G, int(bool(sort)),
                                        _lib.ptr(o_c), _lib.ptr(o_h), _lib.ptr(o_a), _lib.ptr(o_k), _lib.ptr(o_off), _lib.ptr(o_s),
                                        _lib.ptr(ws), nbytes, _lib.current_stream()), "dafne_train_gt_hip")
        for t in (corners, classes, offsets, ws):
            t.record_stream(torch.cuda.current_stream())
    return PackedGT(o_c, o_h, o_a, o_k, o_off, o_s)


class TrainBatch:
    """images [N, 3, cap_h, cap_w] uint8 (view v in [:oh, :ow], 0 elsewhere), valid_hw [N, 2] int32 on the device,
    valid_hw_host the same numbers as a host list (they follow from the parameters: no read), params [ViewParams], windows,
    gt: PackedGT or None."""

    def __init__(self, images, valid_hw, valid_hw_host, params, windows, gt):
        self.images, self.valid_hw, self.valid_hw_host, self.params, self.windows, self.gt = images, valid_hw, valid_hw_host, params, windows, gt

    def __len__(self):
        return len(self.params)

    def instances(self):
        """One Instances per view (image_size = the view's own (oh, ow)): views into the packed device arrays, as
        TileGroundTruth.instances.  Costs the one host read of the offsets."""
        if self.gt is None:
            raise ValueError("TrainBatch.instances: the batch was made without ground truth")
        off = self.gt.host_offsets()
        out = []
        for v, hw in enumerate(self.valid_hw_host):
            a, b = int(off[v]), int(off[v + 1])
            inst = Instances(tuple(hw))
            inst.gt_corners = self.gt.corners[a:b]
            inst.gt_boxes = Boxes(self.gt.hbox[a:b])
            inst.gt_corners_area = self.gt.area[a:b]
            inst.gt_classes = self.gt.classes[a:b].to(torch.int64)
            out.append(inst)
        return out

    def batched_inputs(self):
        """The reference's training contract: {"image": uint8 CHW view cropped to valid_hw, "instances", "height", "width"}."""
        inst = self.instances() if self.gt is not None else [None] * len(self)
        out = []
        for v, (oh, ow) in enumerate(self.valid_hw_host):
            d = {"image": self.images[v, :, :oh, :ow], "height": int(self.windows[v][2]), "width": int(self.windows[v][3])}
            if inst[v] is not None:
                d["instances"] = inst[v]
            out.append(d)
        return out


def augment_views(sources, windows, params, gt=None, sort=True, size_divisibility=32, cap_hw=None, out=None, device=None):
    """sources: per view a device uint8 BGR image ([H, W, 3] or [3, H, W]; or (image, layout_hwc) where the shape is
    ambiguous); windows: per view (left, up, win_h, win_w), pixels past the source read 0; params: per view ViewParams.
    gt: None or (corners [G, 8] at window scale, classes [G], offsets [N + 1]) as train_gt takes them.  The slab is the
    largest view rounded up to size_divisibility (the backbone's), or cap_hw.  One pixel launch -> TrainBatch."""
    L = _lib.load()
    n = len(params)
    if n == 0 or len(sources) != n or len(windows) != n:
        raise ValueError("augment_views: %d sources, %d windows, %d parameter sets" % (len(sources), len(windows), n))
    srcs = []
    for s in sources:
        img, hwc = (s if isinstance(s, (tuple, list)) else (s, None))
        if not img.is_cuda:
            raise _lib.DafneHipError("augment_views: the MI355X engine has no CPU path (got a CPU image)")
        srcs.append((img, hwc))
    dev = srcs[0][0].device if device is None else torch.device(device)
    valid = [p.out_hw() for p in params]
    if cap_hw is None:
        d = max(1, int(size_divisibility))
        d = d * 4 // int(np.gcd(d, 4))                  # the kernel stores words: the slab's width is a multiple of 4
        cap_h = (max(h for h, _ in valid) + d - 1) // d * d
        cap_w = (max(w for _, w in valid) + d - 1) // d * d
    else:
        cap_h, cap_w = int(cap_hw[0]), int(cap_hw[1])
    arr, keep = _view_array(windows, params, srcs)
    with torch.cuda.device(dev):
        images = out if out is not None else torch.empty((n, 3, cap_h, cap_w), dtype=torch.uint8, device=dev)
        if tuple(images.shape) != (n, 3, cap_h, cap_w) or images.dtype != torch.uint8 or not images.is_contiguous():
            raise ValueError("augment_views: out must be a contiguous uint8 [%d, 3, %d, %d]" % (n, cap_h, cap_w))
        vhw = torch.empty((n, 2), dtype=torch.int32, device=dev)
        nbytes = L.dafne_train_views_workspace_bytes(arr, n)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.check(L.dafne_train_views_u8_hip(arr, n, cap_h, cap_w, _lib.ptr(images), _lib.ptr(vhw), _lib.ptr(ws), nbytes,
                                              _lib.current_stream()), "dafne_train_views_u8_hip")
        for t in keep + [ws]:
            t.record_stream(torch.cuda.current_stream())
    packed = None
    if gt is not None:
        packed = train_gt(windows, params, gt[0], gt[1], gt[2], sort=sort, device=dev)
    return TrainBatch(images, vhw, valid, list(params), [tuple(int(v) for v in w) for w in windows], packed)


def scene_train_batches(cfg, scenes, labels, batch=8, seed=0, patch_size=1024, overlap=200, filter_empty=True, layout_hwc=None,
                        params_fn=None, shuffle=True, epochs=None, device=None):
    """Augmented training batches of the tiles of whole scenes.  split_scene_labels runs once, at ratio (1, 1): the kept rows
    are the tiles' ground truth at window scale.  Every batch is cut FROM THE SCENES (window = tile) by one pixel launch, and its
    ground truth goes kept_* -> dafne_train_gt_hip on the device: the rows of a batch's tiles are gathered with device index
    arithmetic from kept_offsets, no row is copied to the host.  Tiles without a kept object are left out when filter_empty
    (the one host read: the kept counts).  One permutation of the tiles per epoch from `seed` (numpy default_rng; this
    repository's order, not detectron2's TrainingSampler); the augmentation parameters are drawn from the same generator after
    each batch's tiles are chosen.  params_fn(tile_ids) -> [ViewParams] replaces the random draw (tests).  epochs=None: endless.
    Yields TrainBatch with .tile_ids."""
    from ..scene import scene_layout
    from ..scene_labels import split_scene_labels
    if len(scenes) != len(labels["scene_names"]):
        raise ValueError("scene_train_batches: %d scenes, labels of %d scenes" % (len(scenes), len(labels["scene_names"])))
    for img in scenes:
        if not img.is_cuda:
            raise _lib.DafneHipError("scene_train_batches: the MI355X engine has no CPU path (got a CPU scene)")
    dev = scenes[0].device if device is None else torch.device(device)
    patch = int(patch_size)
    aug = TrainAugmentation(cfg)
    sort = bool(cfg.MODEL.DAFNE.SORT_CORNERS_DATALOADER)
    sizes = [scene_layout(img, layout_hwc)[:2] for img in scenes]
    tg = split_scene_labels(labels, sizes, patch, overlap, min_area=cfg.INPUT.MIN_AREA, min_side=cfg.INPUT.MIN_SIDE, ratio=(1, 1),
                            sort=False, device=dev)
    kept = tg.kept_counts()
    ids = [t for t in range(tg.origins.shape[0]) if not filter_empty or kept[t] > 0]
    if not ids:
        raise ValueError("scene_train_batches: no tile with a kept object is left")
    rng = np.random.default_rng(seed)
    bs = max(1, int(batch))
    koff = tg.kept_offsets.to(torch.int64)
    epoch = 0
    while epochs is None or epoch < epochs:
        order = [ids[i] for i in rng.permutation(len(ids))] if shuffle else list(ids)
        for b0 in range(0, len(order), bs):
            part = order[b0:b0 + bs]
            windows = [(int(tg.origins[t, 0]), int(tg.origins[t, 1]), patch, patch) for t in part]
            params = params_fn(part) if params_fn is not None else aug.sample([(patch, patch)] * len(part), rng)
            with torch.cuda.device(dev):
                # the rows of the batch's tiles, gathered on the device: counts and starts come from kept_offsets there
                tid = torch.as_tensor(part, dtype=torch.int64).to(dev)
                start, cnt = koff[tid], koff[tid + 1] - koff[tid]
                off = torch.zeros(len(part) + 1, dtype=torch.int64, device=dev)
                off[1:] = torch.cumsum(cnt, 0)
                G = int(sum(int(kept[t]) for t in part))                      # (host numbers already read: no sync)
                view_of = torch.repeat_interleave(torch.arange(len(part), device=dev), cnt, output_size=G)
                rows = start[view_of] + (torch.arange(G, device=dev) - off[view_of])
                gt = (tg.kept_corners[rows], tg.kept_classes[rows], off.to(torch.int32))
            tb = augment_views([(scenes[int(tg.tile_scene[t])], layout_hwc) for t in part], windows, params, gt=gt, sort=sort, device=dev)
            tb.tile_ids = part
            yield tb
        epoch += 1


def augmented_losses_scenes(model, scenes, labels, seed=0, steps=None, patch_size=1024, overlap=200, batch=8, layout_hwc=None,
                            filter_empty=True, params_fn=None, shuffle=True):
    """OneStageDetector.augmented_losses_scenes (see there)."""
    if model.training:
        raise NotImplementedError("training is outside the scope of the MI355X inference engine")
    if len(scenes) != len(labels["scene_names"]):
        raise ValueError("augmented_losses_scenes: %d scenes, labels of %d scenes" % (len(scenes), len(labels["scene_names"])))
    dev = model.device
    stream = scene_train_batches(model.cfg, [x.to(dev) if x.is_cuda else x for x in scenes], labels, batch=batch, seed=seed,
                                 patch_size=patch_size, overlap=overlap, filter_empty=filter_empty, layout_hwc=layout_hwc,
                                 params_fn=params_fn, shuffle=shuffle, epochs=1 if steps is None else None, device=dev)
    sums, keys, n, k = None, None, 0, 0
    drawn = {"hflip": [0, 0], "vflip": [0, 0], "rot": [0, 0, 0, 0], "size": {}}
    tile_ids = []
    with torch.cuda.device(dev):
        for tb in stream:
            if steps is not None and k >= int(steps):
                break
            vals = model.validation_losses(tb)           # the slab and the packed rows as they are: no host read
            keys = sorted(vals)
            row = torch.stack([vals[key].double() for key in keys]) * len(tb)
            sums = row if sums is None else sums + row
            n += len(tb)
            k += 1
            tile_ids.extend(tb.tile_ids)
            for p in tb.params:
                drawn["hflip"][p.hflip] += 1
                drawn["vflip"][p.vflip] += 1
                drawn["rot"][p.rot] += 1
                key = "%dx%d" % (p.new_h, p.new_w)
                drawn["size"][key] = drawn["size"].get(key, 0) + 1
    if n == 0:
        raise ValueError("augmented_losses_scenes: no step was run")
    out = dict(zip(keys, (sums / n).cpu().tolist()))
    out.update(tiles=n, steps=k, seed=seed, tile_ids=tile_ids, drawn=drawn)
    return out


class DAFNeTrainMapper:
    """record -> one view of a training batch.  `decode` is the host half (the image file; safe on a worker thread), the device
    half is augment_views over the whole batch (build_train_loader).  Records carry "annotations": [{"bbox": 8 numbers (the
    corners at the file's scale), "category_id": int}] or the {"name", "bbox"} objects of dota_evaluation.parse_gt together
    with `classnames`."""

    def __init__(self, cfg, device=None, classnames=None):
        from .loader import DAFNeTestMapper
        self.cfg = cfg
        self.aug = TrainAugmentation(cfg)
        self.sort = bool(cfg.MODEL.DAFNE.SORT_CORNERS_DATALOADER)
        self.device = torch.device(device) if device is not None else None
        self._decode = DAFNeTestMapper(cfg, None).decode
        self.index = {n: i for i, n in enumerate(classnames)} if classnames is not None else None

    def decode(self, record):
        return self._decode(record)

    def annotations(self, record):
        """-> (corners [g, 8] float32, classes [g] int32) of a record."""
        rows, cls = [], []
        for o in record.get("annotations", []):
            if "category_id" in o:
                c = int(o["category_id"])
            elif self.index is not None and o.get("name") in self.index:
                c = self.index[o["name"]]
            else:
                continue
            rows.append(np.asarray(o["bbox"], dtype=np.float64).reshape(8))
            cls.append(c)
        return np.asarray(rows, dtype=np.float32).reshape(-1, 8), np.asarray(cls, dtype=np.int32)

    def batch(self, records, images, rng, staging=None):
        """records + their decoded HWC uint8 images -> TrainBatch on self.device."""
        dev = self.device
        if dev is None or dev.type != "cuda":
            raise _lib.DafneHipError("train loader: the MI355X engine has no CPU path")
        srcs, windows, corners, classes, off = [], [], [], [], [0]
        for r, img in zip(records, images):
            t = img if torch.is_tensor(img) else torch.from_numpy(img)
            if staging is not None:
                t = staging.stage(t)
            srcs.append((t.to(dev, non_blocking=True), True))
            if staging is not None:
                staging.mark(dev)
            windows.append((0, 0, int(t.shape[0]), int(t.shape[1])))
            c, k = self.annotations(r)
            corners.append(c)
            classes.append(k)
            off.append(off[-1] + c.shape[0])
        params = self.aug.sample([(w[2], w[3]) for w in windows], rng)
        gt = (np.concatenate(corners, 0), np.concatenate(classes, 0), np.asarray(off, dtype=np.int32))
        return augment_views(srcs, windows, params, gt=gt, sort=self.sort, device=dev)


class _TrainLoader:
    """An endless iterable of TrainBatch: one permutation of the records per epoch from `seed`, decoded ahead on
    InferenceLoader's host threads, through its pinned staging ring."""

    def __init__(self, cfg, records, batch_size, seed, device, num_workers, prefetch_batches, classnames):
        from .loader import InferenceLoader
        self.cfg, self.records, self.batch_size, self.seed = cfg, list(records), max(1, int(batch_size)), seed
        self.mapper = DAFNeTrainMapper(cfg, device, classnames)
        self._mk = lambda recs: InferenceLoader(cfg, recs, batch_size=self.batch_size, device=None, num_workers=num_workers,
                                                prefetch_batches=prefetch_batches, shard=(0, 1))
        if not self.records:
            raise ValueError("build_train_loader: no records")

    def __iter__(self):
        from .loader import _Staging
        rng = np.random.default_rng(self.seed)
        staging = _Staging(2 * self.batch_size)
        while True:
            recs = [self.records[i] for i in rng.permutation(len(self.records))]
            done = 0
            for imgs in self._mk(recs)._decoded_batches():
                yield self.mapper.batch(recs[done:done + len(imgs)], imgs, rng, staging)
                done += len(imgs)


def build_train_loader(cfg, dataset, batch_size=None, seed=0, device=None, num_workers=8, prefetch_batches=2, classnames=None):
    """`build_train_loader(cfg)` of tools/plain_train_net.py:219-277 for this engine.  dataset: a name registered in
    loader.DatasetCatalog or a list of records with "file_name" and "annotations".  Endless; the order is this repository's
    (one permutation per epoch from `seed`), not detectron2's TrainingSampler."""
    from .loader import DatasetCatalog
    records = DatasetCatalog.get(dataset) if isinstance(dataset, str) else list(dataset)
    bs = int(cfg.SOLVER.IMS_PER_BATCH) if batch_size is None else int(batch_size)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return _TrainLoader(cfg, records, bs, seed, dev, num_workers, prefetch_batches, classnames)
