"""Whole-scene inference: a scene goes in, scene-coordinate detections come out (DOTA's split -> detect -> merge in one call).

The reference's test workflow on DOTA scenes (up to ~4000 x 4000 px) is three offline steps:
  1. tools/prepare_dota/split_dota.py (SplitOnlyImage_multi_process.splitbase.SplitSingle) writes patch x patch PNG tiles
     with an overlap, named <scene>__<rate>__<left>___<up>, zero-padded past the scene edge;
  2. the detector runs on the tile files; dota_evaluation._generate_task_1_files writes "%s %.4f %.2f .. %.2f" lines;
  3. ResultMerge_multi_process.mergebypoly parses them back, shifts them into scene coordinates and runs greedy polygon
     NMS at 0.1 per (class, scene) -> Task1_merged/, the submitted files.
Here the tiles are cropped on the device (dafne_scene_tiles_u8_hip, one launch), run through detect_packed, and their rows
become the merge's f64 rows on the device (dafne_scene_merge_rows_hip: the "%.2f" / "%.4f" round trip restated as
rint(v * 10^k) / 10^k, bit for bit), which go to the tile merge's own NMS (dafne_poly_nms_f64_batched_hip, thresh 0.1,
strict hull test).  write_task1_merged then writes what mergebypoly writes, byte for byte.

  split_origins(h, w, patch_size, overlap)      SplitSingle's tile origins at rate 1, in its emission order
  gather_tiles(scenes, origins, patch)          [T, patch, patch, 3] uint8 BGR tiles of all scenes, one launch
  scaled_size(h, w, scale)                      the size of a scene resampled by `scale`
  gather_scaled_tiles(scenes, scales, origins, patch)   the same tiles of the RESAMPLED scenes, cut from the scenes, one launch
  merge_tile_rows(...)                          tile rows -> per-(scene, class) f64 merge rows + back-index
  merge_scenes(...)                             the above + NMS + the kept rows per scene
  detect_scenes(model, scenes, ...)             OneStageDetector.detect_scenes
  scene_views(srcs, out_h, out_w)               TTA views cut from scenes / tiles: [V, 3, out_h, out_w] uint8, one launch
  tta_view_table(mapper, h, w, orig_hw)         per view: its resize target, flips and inverse transform (host)
  tta_candidates(views, n_images, k_cap)        per-view packed rows -> the TTA merge's Candidates (device, one launch)
  tta_tile_rows(tta, scenes, ...)               every tile's merged TTA rows
  detect_scenes_tta(tta, scenes, ...)           OneStageRCNNWithTTA.detect_scenes
  write_task1_merged(results, names, classes, dst)
  write_task2_merged(results, names, classes, dst)

DOTA Task2 (horizontal boxes) is a second merge of the SAME tile rows: with tasks=("task1", "task2") the rows also become
mergebyrec's f64 rows (dafne_scene_merge_hbb_rows_hip: dots4ToRec4 of the Task1 row) and go through py_cpu_nms on the device
(dafne_hbb_nms_f64_batched_hip, thresh 0.1); every scene dict gains a "task2" entry and write_task2_merged writes what
mergebyrec writes for the Task2 files task1_to_task2 makes of the tile-level Task1 files.  The detector runs once.

Multi-scale: detect_scenes(scales=(1, 0.5)) splits every scene once per scale -- the tiles of a scale s are the split of the
scene resampled to scaled_size(h, w, s), cut and resampled from the scene itself in one launch
(dafne_scene_scaled_tiles_u8_hip: Pillow's 8-bit resize of the whole scene, bicubic by default) -- and all tiles of a scene go
through ONE merge: the rows of a tile of scale s are divided by s (dafne_scene_merge_rows_scaled_hip: poly2origpoly's
float(poly + x) / float(rate)), so the results are in the scene's own coordinates.  The pixels of a scaled tile are NOT the
reference's (its split resizes with cv2.resize(INTER_CUBIC); split_origins(rate != 1) names that split and keeps refusing);
everything after the pixels is mergebypoly / mergebyrec on tile files named <scene>__<scale>__<left>___<up>.

Scene-level TTA runs the per-image TTA of every tile (modeling/tta.py: DotaDatasetMapperTTA's views, detect_packed without
post-process, the inverse transforms, one rotated NMS + cap per tile) with views of many tiles batched: per TTA size one
dafne_scene_views_u8_hip launch cuts and resamples the plain / hflip / vflip views of all tiles of a batch straight from
the scenes (no tile files, no per-view resize calls), detect_packed runs them in calls that keep the per-image path's view
chunks (a few tiles per call), and dafne_tta_candidates_hip maps
every view's rows back into its tile's merge candidates on the device, where pp.select / pp.gather finish the merge.
The tiles' merged rows then go through merge_scenes like detect_scenes' tile rows.
"""
import os

import numpy as np
import torch

from . import _lib

NMS_THRESH = 0.1          # ResultMerge_multi_process.py:22
# NMS workspace per launch: the buckets of a call are cut into launches of at most this many bytes
_NMS_WS_LIMIT = 1 << 31
# scene TTA: views per detector call, whole tiles' share of a view chunk (R101, 27 views, batch 8 on one MI355X: 6 / 9 / 24
# views per call ran at 1.14 / 0.98 / 0.72x the per-tile route; scripts/scene_bench.py --tta --views-per-call)
_TTA_VIEWS_PER_CALL = 6


def split_origins(h, w, patch_size=1024, overlap=200, rate=1):
    """[(left, up), ...] of SplitSingle's tiles for an h x w scene (SplitOnlyImage_multi_process.py:46-78): outer loop over
    left, inner over up, step patch_size - overlap, an edge tile shifted back to max(size - patch_size, 0)."""
    if rate != 1:
        raise NotImplementedError("split rate %r: the reference resizes the scene with cv2.resize(INTER_CUBIC) first, which "
                                  "has no bit-exact counterpart here; only rate 1 is supported" % (rate,))
    h, w, patch_size, overlap = int(h), int(w), int(patch_size), int(overlap)
    slide = patch_size - overlap
    if h < 1 or w < 1 or patch_size < 1 or slide < 1:
        raise ValueError("split_origins: bad scene %dx%d / patch %d / overlap %d" % (h, w, patch_size, overlap))
    out = []
    left = 0
    while left < w:
        if left + patch_size >= w:
            left = max(w - patch_size, 0)
        up = 0
        while up < h:
            if up + patch_size >= h:
                up = max(h - patch_size, 0)
            out.append((left, up))
            if up + patch_size >= h:
                break
            up += slide
        if left + patch_size >= w:
            break
        left += slide
    return out


def scene_layout(img, layout_hwc=None):
    """(h, w, layout_hwc) of a uint8 BGR scene tensor, [H,W,3] or [3,H,W]."""
    if img.dim() != 3 or img.dtype != torch.uint8:
        raise ValueError("a scene is a uint8 [H,W,3] or [3,H,W] tensor, got %s %s" % (img.dtype, tuple(img.shape)))
    if layout_hwc is None:
        hwc, chw = img.shape[2] == 3, img.shape[0] == 3
        if hwc == chw:
            raise ValueError("scene of shape %s: pass layout_hwc (HWC and CHW are both possible or neither is)" % (tuple(img.shape),))
        layout_hwc = hwc
    if layout_hwc:
        if img.shape[2] != 3:
            raise ValueError("HWC scene needs 3 channels, got %s" % (tuple(img.shape),))
        return int(img.shape[0]), int(img.shape[1]), True
    if img.shape[0] != 3:
        raise ValueError("CHW scene needs 3 channels, got %s" % (tuple(img.shape),))
    return int(img.shape[1]), int(img.shape[2]), False


def gather_tiles(scenes, origins, patch, layout_hwc=None):
    """scenes: device uint8 images; origins: per scene a list of (left, up).  -> [T, patch, patch, 3] uint8, the tiles of all
    scenes in scene order, each zero-padded past its scene's edge (one launch)."""
    L = _lib.load()
    descs = []
    keep = []
    for img, org in zip(scenes, origins):
        if not img.is_cuda:
            raise _lib.DafneHipError("gather_tiles: the MI355X engine has no CPU path (got a CPU scene)")
        h, w, hwc = scene_layout(img, layout_hwc)
        img = img.contiguous()
        keep.append(img)
        for left, up in org:
            descs.append((img.data_ptr(), h, w, int(hwc), int(left), int(up)))
    n = len(descs)
    if n == 0:
        raise ValueError("gather_tiles: no tiles")
    dev = scenes[0].device
    arr = (_lib.SceneTile * n)()
    for k, (p, h, w, hwc, left, up) in enumerate(descs):
        arr[k].d_scene, arr[k].h, arr[k].w, arr[k].layout_hwc, arr[k].left, arr[k].up = p, h, w, hwc, left, up
    with torch.cuda.device(dev):
        out = torch.empty((n, patch, patch, 3), dtype=torch.uint8, device=dev)
        nbytes = L.dafne_scene_tiles_workspace_bytes(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(L.dafne_scene_tiles_u8_hip(arr, n, int(patch), _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.current_stream()),
                   "dafne_scene_tiles_u8_hip")
    return out


RESAMPLE = {"bilinear": _lib.FILTER_BILINEAR, "bicubic": _lib.FILTER_BICUBIC}


def scaled_size(h, w, scale):
    """(new_h, new_w) of an h x w scene resampled by `scale`: max(1, rint(size * scale)), round half to even -- cv2.resize's
    dsize for dsize=None, saturate_cast<int>(size * fx) [recalled: OpenCV imgproc resize.cpp; cvRound rounds half to even]."""
    return max(1, int(np.rint(int(h) * float(scale)))), max(1, int(np.rint(int(w) * float(scale))))


def _check_scales(scales, resample):
    """-> the scales as a tuple of floats; ValueError on an empty list, a repeated, non-finite or out-of-range scale, or an
    unknown filter."""
    try:
        scales = tuple(float(s) for s in scales)
    except TypeError:
        raise ValueError("scales %r: a sequence of numbers" % (scales,))
    if not scales:
        raise ValueError("scales: at least one scale")
    for s in scales:
        if not np.isfinite(s) or not 0.0 < s <= 4.0:
            raise ValueError("scale %r: outside (0, 4]" % (s,))
    if len(set(scales)) != len(scales):
        raise ValueError("scales %r: a scale is repeated" % (scales,))
    if resample not in RESAMPLE:
        raise ValueError("resample %r: one of %r" % (resample, tuple(sorted(RESAMPLE))))
    return scales


def scale_plan(sizes, scales, patch_size=1024, overlap=200):
    """The tiles of a multi-scale call, in the order the merge buckets see them: for every scene (sizes: its (h, w)), then
    every scale in the given order, split_origins of the resampled size in split order.  -> per scene a list of
    (scale, (new_h, new_w), origins)."""
    plan = []
    for h, w in sizes:
        per = []
        for s in scales:
            nh, nw = (int(h), int(w)) if s == 1.0 else scaled_size(h, w, s)
            per.append((s, (nh, nw), split_origins(nh, nw, patch_size, overlap)))
        plan.append(per)
    return plan


def gather_scaled_tiles(scenes, scales, origins, patch, resample="bicubic", layout_hwc=None):
    """scenes: device uint8 images; scales: one scale per scene; origins: per scene a list of (left, up) in the coordinates of
    the scene resampled to scaled_size(h, w, scale).  -> [T, patch, patch, 3] uint8: tile t is the patch x patch window at its
    origin of PIL.Image.resize(scene, (new_w, new_h), resample) -- of the whole scene, bit for bit --, zero past the resampled
    scene's edge.  One launch; the resampled scenes are never written.  (A scene may appear several times, once per scale.)"""
    L = _lib.load()
    if resample not in RESAMPLE:
        raise ValueError("resample %r: one of %r" % (resample, tuple(sorted(RESAMPLE))))
    descs = []
    keep = []
    for img, scale, org in zip(scenes, scales, origins):
        if not img.is_cuda:
            raise _lib.DafneHipError("gather_scaled_tiles: the MI355X engine has no CPU path (got a CPU scene)")
        h, w, hwc = scene_layout(img, layout_hwc)
        nh, nw = scaled_size(h, w, scale)
        img = img.contiguous()
        keep.append(img)
        for left, up in org:
            descs.append((img.data_ptr(), h, w, int(hwc), nh, nw, int(left), int(up)))
    n = len(descs)
    if n == 0:
        raise ValueError("gather_scaled_tiles: no tiles")
    dev = scenes[0].device
    arr = (_lib.ScaledTile * n)()
    for k, (p, h, w, hwc, nh, nw, left, up) in enumerate(descs):
        a = arr[k]
        a.d_scene, a.h, a.w, a.layout_hwc, a.new_h, a.new_w, a.left, a.up = p, h, w, hwc, nh, nw, left, up
        a.filter = RESAMPLE[resample]
    with torch.cuda.device(dev):
        out = torch.empty((n, patch, patch, 3), dtype=torch.uint8, device=dev)
        nbytes = L.dafne_scene_scaled_tiles_workspace_bytes(arr, n)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.check(L.dafne_scene_scaled_tiles_u8_hip(arr, n, int(patch), _lib.ptr(out), _lib.ptr(ws), nbytes,
                                                     _lib.current_stream()), "dafne_scene_scaled_tiles_u8_hip")
    return out


def task1_score_mode(cfg):
    """1 where evaluation.task1.task1_scores writes score^2 / centerness (CENTERNESS != none, not CENTERNESS_USE_IN_SCORE)."""
    d = cfg.MODEL.DAFNE
    return 1 if (d.CENTERNESS != "none" and not d.CENTERNESS_USE_IN_SCORE) else 0


def skip_mask(cfg):
    """Labels _generate_task_1_files leaves out: DOTA-1.5's container-crane (15) with DATASETS.DOTA_REMOVE_CONTAINER_CRANE."""
    return (1 << 15) if bool(cfg.DATASETS.DOTA_REMOVE_CONTAINER_CRANE) else 0


def merge_tile_rows(rows, counts, tile_info, n_scenes, n_classes, skip=0, score_mode=0, m_cap=None, overflow=None, hbb=False,
                    tile_scales=None):
    """rows [T,k_cap,18] f32 + counts [T] (device) + tile_info [T,3] int32 (left, up, scene) -> (dets [B,m_cap,9] f64,
    bucket counts [B] int32, src [B,m_cap] int32, m_cap) with B = n_scenes * n_classes.  m_cap None: sized from the bucket
    counts (a host read of B integers).  overflow: optional device int tensor, read in that same host read; nonzero
    raises (rows the caller truncated).  hbb: the Task2 rows instead, dets [B,m_cap,5] f64 (xmin, ymin, xmax, ymax, score);
    buckets, counts and src are the same.  tile_scales: optional [T] split rates (tile_info's left / up are in the resampled
    scene's coordinates); the rows are (q + left | up) / scale in fp64, i.e. in the scene's own coordinates."""
    L = _lib.load()
    dev = rows.device
    T, k_cap = int(rows.shape[0]), int(rows.shape[1])
    if rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[2] != _lib.DET_ROW:
        raise ValueError("merge_tile_rows: rows must be float32 [T, k_cap, %d]" % _lib.DET_ROW)
    nb = int(n_scenes) * int(n_classes)
    with torch.cuda.device(dev):
        rows = rows.contiguous()
        counts = counts.to(device=dev, dtype=torch.int32).contiguous()
        info = torch.as_tensor(tile_info, dtype=torch.int32).reshape(T, 3).to(dev).contiguous()
        nbytes = L.dafne_scene_merge_workspace_bytes(T, int(n_classes))
        if nbytes == 0:
            raise _lib.DafneHipError("scene merge: bad size (%d tiles, %d classes)" % (T, n_classes))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        bcount = torch.empty(nb, dtype=torch.int32, device=dev)

        if tile_scales is None:
            fn, what = (L.dafne_scene_merge_hbb_rows_hip, "dafne_scene_merge_hbb_rows_hip") if hbb else \
                (L.dafne_scene_merge_rows_hip, "dafne_scene_merge_rows_hip")
            extra = ()
        else:
            fn, what = (L.dafne_scene_merge_hbb_rows_scaled_hip, "dafne_scene_merge_hbb_rows_scaled_hip") if hbb else \
                (L.dafne_scene_merge_rows_scaled_hip, "dafne_scene_merge_rows_scaled_hip")
            sc = torch.as_tensor(tile_scales, dtype=torch.float64).reshape(-1)
            if int(sc.numel()) != T or not bool((torch.isfinite(sc) & (sc > 0)).all()):
                raise ValueError("merge_tile_rows: tile_scales must be %d finite positive numbers" % T)
            sc = sc.to(dev).contiguous()
            extra = (_lib.ptr(sc),)

        def call(cap, dets, src):
            _lib.check(fn(_lib.ptr(rows), _lib.ptr(counts), T, k_cap, _lib.ptr(info), *extra, int(n_scenes),
                          int(n_classes), int(skip), int(score_mode), int(cap), _lib.ptr(dets),
                          _lib.ptr(bcount), _lib.ptr(src), _lib.ptr(ws), nbytes, _lib.current_stream()), what)
        if m_cap is None:
            call(0, None, None)
            if overflow is None:
                m_cap = max(int(bcount.max().item()), 1)
            else:
                mx, ovf = torch.stack([bcount.max(), overflow.to(torch.int32).max()]).cpu().tolist()
                if ovf:
                    raise _lib.DafneHipError("tile detections exceed the packed row capacity (%d): rows would be dropped" % k_cap)
                m_cap = max(int(mx), 1)
        dets = torch.empty((nb, m_cap, 5 if hbb else 9), dtype=torch.float64, device=dev)
        src = torch.empty((nb, m_cap), dtype=torch.int32, device=dev)
        call(m_cap, dets, src)
    return dets, bcount, src, m_cap


def nms_buckets(dets, bcount, m_cap, thresh=NMS_THRESH):
    """The tile merge's NMS on every bucket, on the device: -> keep [B,m_cap] int64, num_keep [B].  dets [B,m_cap,9]: the
    polygon NMS with the strict hull test (mergebypoly); [B,m_cap,5]: the horizontal-box NMS (mergebyrec)."""
    L = _lib.load()
    dev = dets.device
    nb = int(dets.shape[0])
    hbb = int(dets.shape[2]) == 5
    ws_bytes = L.dafne_hbb_nms_f64_workspace_bytes if hbb else L.dafne_poly_nms_f64_workspace_bytes
    what = "dafne_hbb_nms_f64_batched_hip" if hbb else "dafne_poly_nms_f64_batched_hip"
    keep = torch.empty((nb, m_cap), dtype=torch.int64, device=dev)
    nk = torch.zeros(nb, dtype=torch.int32, device=dev)
    per = max(ws_bytes(1, m_cap), 1)
    step = max(1, min(nb, _NMS_WS_LIMIT // per))
    with torch.cuda.device(dev):
        nbytes = ws_bytes(step, m_cap)
        if nbytes == 0:
            raise _lib.DafneHipError("%s: bad size %d x %d" % (what, step, m_cap))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        for b0 in range(0, nb, step):
            n = min(step, nb - b0)
            if hbb:
                rc = L.dafne_hbb_nms_f64_batched_hip(_lib.ptr(dets[b0:b0 + n]), _lib.ptr(bcount[b0:b0 + n]), n, m_cap, float(thresh),
                                                     _lib.ptr(keep[b0:b0 + n]), _lib.ptr(nk[b0:b0 + n]), _lib.ptr(ws), nbytes,
                                                     _lib.current_stream())
            else:
                rc = L.dafne_poly_nms_f64_batched_hip(_lib.ptr(dets[b0:b0 + n]), _lib.ptr(bcount[b0:b0 + n]), n, m_cap,
                                                      float(thresh), 1, _lib.ptr(keep[b0:b0 + n]), _lib.ptr(nk[b0:b0 + n]),
                                                      _lib.ptr(ws), nbytes, 0, _lib.current_stream())
            _lib.check(rc, what)
    return keep, nk


TASKS = ("task1", "task2")


def _check_tasks(tasks):
    tasks = tuple(tasks)
    bad = [t for t in tasks if t not in TASKS]
    if bad or "task1" not in tasks:
        raise ValueError("tasks %r: a subset of %r that holds \"task1\" (the Task2 boxes are made of the Task1 rows)" % (tasks, TASKS))
    return tasks


def _kept_rows(dets, bcount, src, m_cap, n_scenes, n_classes, k_cap, box_key):
    """NMS on every bucket + the kept rows per scene: class by class, each class in keep order."""
    keep, nk = nms_buckets(dets, bcount, m_cap)
    dev = dets.device
    nb = dets.shape[0]
    wd = int(dets.shape[2])
    # the kept rows of every bucket, bucket-major (scene, then class): one host read, the kept counts
    valid = torch.arange(m_cap, device=dev)[None, :] < nk[:, None].to(torch.int64)
    flat = (torch.arange(nb, device=dev, dtype=torch.int64)[:, None] * m_cap + keep.clamp(0, m_cap - 1))[valid]
    d = dets.reshape(-1, wd)[flat]
    s = src.reshape(-1)[flat].to(torch.int64)
    lab = (torch.arange(nb, device=dev, dtype=torch.int64)[:, None].expand(nb, m_cap) % n_classes)[valid]
    per_scene = nk.reshape(n_scenes, n_classes).sum(1).cpu().tolist()
    out = []
    o = 0
    for k in per_scene:
        out.append({box_key: d[o:o + k, :wd - 1], "scores": d[o:o + k, wd - 1], "labels": lab[o:o + k],
                    "tile": s[o:o + k] // k_cap, "row": s[o:o + k] % k_cap})
        o += k
    return out


def merge_scenes(rows, counts, tile_info, n_scenes, n_classes, skip=0, score_mode=0, overflow=None, tasks=("task1",),
                 tile_scales=None):
    """Tile rows -> per scene {"corners" [K,8] f64, "scores" [K] f64, "labels" [K] int64, "tile" [K], "row" [K]}: class by
    class, each class in the NMS keep order (descending score) -- what mergebypoly writes for that scene.  overflow: see
    merge_tile_rows.  With "task2" in tasks every dict also holds "task2": {"boxes" [K2,4] f64 (xmin, ymin, xmax, ymax),
    "scores", "labels", "tile", "row"}, what mergebyrec writes for that scene, merged from the same tile rows.  tile_scales:
    see merge_tile_rows (None: the unscaled entries)."""
    tasks = _check_tasks(tasks)
    k_cap = int(rows.shape[1])
    kw = {} if tile_scales is None else {"tile_scales": tile_scales}
    dets, bcount, src, m_cap = merge_tile_rows(rows, counts, tile_info, n_scenes, n_classes, skip, score_mode,
                                               overflow=overflow, **kw)
    out = _kept_rows(dets, bcount, src, m_cap, n_scenes, n_classes, k_cap, "corners")
    if "task2" in tasks:
        # the same buckets and counts: m_cap is known, no second read
        dets5, bcount5, src5, _ = merge_tile_rows(rows, counts, tile_info, n_scenes, n_classes, skip, score_mode, m_cap=m_cap, hbb=True,
                                                   **kw)
        for r, r2 in zip(out, _kept_rows(dets5, bcount5, src5, m_cap, n_scenes, n_classes, k_cap, "boxes")):
            r["task2"] = r2
    return out


def _detect_tiles(model, tiles, patch, batch):
    """[T, patch, patch, 3] uint8 tiles -> (rows, counts) of detect_packed(pipelined=True) in batches of `batch`."""
    from .data.loader import _to_chw_resized, inference_resize_shape
    cfg = model.cfg
    nh, nw = inference_resize_shape(cfg, patch, patch)
    resize = (nh, nw) != (patch, patch)
    splits = max(1, int(cfg.ENGINE.PIPELINE_SPLITS))
    T = int(tiles.shape[0])
    parts = []
    for b0 in range(0, T, max(1, int(batch))):
        x = tiles[b0:b0 + batch]
        n = int(x.shape[0])
        if resize:
            # what the test loader does with a patch x patch tile file (data.loader.DAFNeTestMapper.finish): Pillow-exact
            # resize to the test size, detections scaled back to the tile's own size
            x = torch.stack([_to_chw_resized(x[i], nh, nw) for i in range(n)])
            parts.append(model.detect_packed(x, out_hw=[(patch, patch)] * n, pipelined=True, splits=splits))
        else:
            parts.append(model.detect_packed(x, layout_hwc=True, pipelined=True, splits=splits))
    torch.cuda.current_stream().wait_stream(model.side_stream)
    return torch.cat([r for r, _ in parts]), torch.cat([c for _, c in parts])


def detect_scenes(model, scenes, patch_size=1024, overlap=200, batch=8, layout_hwc=None, tasks=("task1",), scales=(1,),
                  resample="bicubic"):
    """OneStageDetector.detect_scenes: device uint8 BGR scenes (HWC or CHW) -> one result per scene (merge_scenes' dicts,
    plus "origins": the scene's tile origins in split order; tasks: see merge_scenes).  Tiles of all scenes go through detect_packed(pipelined=True)
    in batches of `batch` (the engine is batch-invariant: a tile's detections do not depend on its batch).

    scales: the split rates.  (1,) is the single-scale route.  Otherwise every scene is split once per scale, in the given
    order (scale_plan): the tiles of scale s are cut from the scene resampled to scaled_size(h, w, s) with Pillow's `resample`
    filter ("bicubic" / "bilinear"; gather_scaled_tiles; scale 1 is the plain crop), all tiles of a scene are merged in one
    NMS in the scene's own coordinates, and every result also holds "tile_scales", one per tile, parallel to "origins" (which
    are in the resampled scene's coordinates)."""
    tasks = _check_tasks(tasks)
    scales = _check_scales(scales, resample)
    if not scenes:
        return []
    cfg = model.cfg
    dev = model.device
    patch = int(patch_size)
    if scales != (1.0,):
        return _detect_scenes_scaled(model, scenes, patch, overlap, batch, layout_hwc, tasks, scales, resample)
    origins = []
    info = []
    for s, img in enumerate(scenes):
        h, w, _ = scene_layout(img, layout_hwc)
        org = split_origins(h, w, patch, overlap)
        origins.append(org)
        info.extend((left, up, s) for left, up in org)
    with torch.cuda.device(dev):
        tiles = gather_tiles([x.to(dev) for x in scenes], origins, patch, layout_hwc)
        rows, counts = _detect_tiles(model, tiles, patch, batch)
        res = merge_scenes(rows, counts, info, len(scenes), int(cfg.MODEL.DAFNE.NUM_CLASSES), skip_mask(cfg), task1_score_mode(cfg),
                           tasks=tasks)
    for r, org in zip(res, origins):
        r["origins"] = org
    return res


def _detect_scenes_scaled(model, scenes, patch, overlap, batch, layout_hwc, tasks, scales, resample):
    cfg = model.cfg
    dev = model.device
    plan = scale_plan([scene_layout(img, layout_hwc)[:2] for img in scenes], scales, patch, overlap)
    info, tile_scales = [], []
    plain = [[] for _ in scenes]                  # scale 1: origins per scene (gather_tiles)
    plain_at, scaled_at = [], []                  # positions of the two launches' tiles in the merge order
    sc_scenes, sc_scales, sc_origins = [], [], []
    with torch.cuda.device(dev):
        on_dev = [x.to(dev) for x in scenes]
        for s, per in enumerate(plan):
            for scale, _, org in per:
                at = range(len(info), len(info) + len(org))
                info.extend((left, up, s) for left, up in org)
                tile_scales.extend([scale] * len(org))
                if scale == 1.0:
                    plain[s] = org
                    plain_at.extend(at)
                else:
                    sc_scenes.append(on_dev[s])
                    sc_scales.append(scale)
                    sc_origins.append(org)
                    scaled_at.extend(at)
        tiles = torch.empty((len(info), patch, patch, 3), dtype=torch.uint8, device=dev)
        if plain_at:
            tiles[torch.as_tensor(plain_at, device=dev)] = gather_tiles(on_dev, plain, patch, layout_hwc)
        tiles[torch.as_tensor(scaled_at, device=dev)] = gather_scaled_tiles(sc_scenes, sc_scales, sc_origins, patch, resample,
                                                                            layout_hwc)
        rows, counts = _detect_tiles(model, tiles, patch, batch)
        res = merge_scenes(rows, counts, info, len(scenes), int(cfg.MODEL.DAFNE.NUM_CLASSES), skip_mask(cfg), task1_score_mode(cfg),
                           tasks=tasks, tile_scales=tile_scales)
    o = 0
    for r, per in zip(res, plan):
        r["origins"] = [xy for _, _, org in per for xy in org]
        r["tile_scales"] = tile_scales[o:o + len(r["origins"])]
        o += len(r["origins"])
    return res


def scene_views(srcs, out_h, out_w):
    """srcs: per view (img, layout_hwc, left, up, win_h, win_w, hflip, vflip), img a device uint8 BGR image ([H,W,3] with
    layout_hwc, else [3,H,W]) -> [V, 3, out_h, out_w] uint8: view v is resize_u8 of the zero-padded win_h x win_w window at
    (left, up), flipped -- bit for bit -- in one launch."""
    L = _lib.load()
    n = len(srcs)
    if n == 0:
        raise ValueError("scene_views: no views")
    arr = (_lib.ViewSrc * n)()
    keep = []
    for k, (img, hwc, left, up, wh, ww, hf, vf) in enumerate(srcs):
        if not img.is_cuda:
            raise _lib.DafneHipError("scene_views: the MI355X engine has no CPU path (got a CPU image)")
        h, w, hwc = scene_layout(img, hwc)
        img = img.contiguous()
        keep.append(img)
        a = arr[k]
        a.d_src, a.h, a.w, a.layout_hwc, a.left, a.up = img.data_ptr(), h, w, int(hwc), int(left), int(up)
        a.win_h, a.win_w, a.hflip, a.vflip = int(wh), int(ww), int(bool(hf)), int(bool(vf))
    dev = keep[0].device
    with torch.cuda.device(dev):
        out = torch.empty((n, 3, int(out_h), int(out_w)), dtype=torch.uint8, device=dev)
        nbytes = L.dafne_scene_views_workspace_bytes(arr, n, int(out_h), int(out_w))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.check(L.dafne_scene_views_u8_hip(arr, n, int(out_h), int(out_w), _lib.ptr(out), _lib.ptr(ws), nbytes,
                                              _lib.current_stream()), "dafne_scene_views_u8_hip")
    return out


def tta_view_table(mapper, h, w, orig_hw):
    """The views of an (h, w) loader image whose original is orig_hw, in DotaDatasetMapperTTA.view_specs' order: per view
    (new_h, new_w, hflip, vflip, width, height, rx1, ry1, rx2, ry2) -- the pixels' resize target and flips, and the inverse
    of the view's transform list as _invert_and_concat_fast applies it: un-flip by width / height, then (x * rx1) * rx2, the
    ratios float32 of the python double (1 where there is no pre-resize)."""
    from .modeling.tta import HFlipT, ResizeT, VFlipT
    out = []
    for nh, nw, tfl in mapper.view_specs(int(h), int(w), tuple(int(v) for v in orig_hw)):
        ops = list(tfl.tfms)
        hf = vf = False
        wv = hv = 0.0
        if ops and isinstance(ops[-1], HFlipT):
            hf, wv = True, float(ops.pop().width)
        elif ops and isinstance(ops[-1], VFlipT):
            vf, hv = True, float(ops.pop().height)
        if not ops or len(ops) > 2 or not all(isinstance(t, ResizeT) for t in ops):
            raise NotImplementedError("scene TTA: a view transform other than [pre-resize,] resize [, one flip]")
        inv = [t.inverse() for t in reversed(ops)]           # un-resize of the view first, then of the pre-resize
        rx = [t.new_w * 1.0 / t.w for t in inv] + [1.0]
        ry = [t.new_h * 1.0 / t.h for t in inv] + [1.0]
        f32 = np.float32
        out.append((int(nh), int(nw), hf, vf, f32(wv), f32(hv), f32(rx[0]), f32(ry[0]), f32(rx[1]), f32(ry[1])))
    return out


def tta_candidates(views, n_images, k_cap, m_cap=None):
    """views: per view (rows [k_cap, 18] f32 device view, count [1] int32 device view, image, slot, table row of
    tta_view_table) -> (postprocess.Candidates [n_images, m_cap], overflow [n_images] int32), one launch.  m_cap None:
    k_cap x the most views of one image."""
    from . import postprocess as pp
    L = _lib.load()
    n = len(views)
    if n == 0:
        raise ValueError("tta_candidates: no views")
    per = {}
    for v in views:
        per[v[2]] = per.get(v[2], 0) + 1
    if m_cap is None:
        m_cap = int(k_cap) * max(per.values())
    arr = (_lib.TtaView * n)()
    dev = views[0][0].device
    for k, (rows, cnt, img, slot, t) in enumerate(views):
        if rows.dtype != torch.float32 or rows.dim() != 2 or tuple(rows.shape) != (k_cap, _lib.DET_ROW) or not rows.is_contiguous():
            raise ValueError("tta_candidates: rows of a view must be contiguous float32 [%d, %d]" % (k_cap, _lib.DET_ROW))
        if cnt.dtype != torch.int32:
            raise ValueError("tta_candidates: counts must be int32")
        a = arr[k]
        a.d_rows, a.d_count, a.tile, a.slot = rows.data_ptr(), cnt.data_ptr(), int(img), int(slot)
        a.flip_x, a.flip_y, a.width, a.height = int(t[2]), int(t[3]), float(t[4]), float(t[5])
        a.rx1, a.ry1, a.rx2, a.ry2 = float(t[6]), float(t[7]), float(t[8]), float(t[9])
    with torch.cuda.device(dev):
        cand = pp.Candidates(int(n_images), int(m_cap), dev)
        ovf = torch.empty(int(n_images), dtype=torch.int32, device=dev)
        nbytes = L.dafne_tta_candidates_workspace_bytes(n, int(n_images))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.check(L.dafne_tta_candidates_hip(arr, n, int(n_images), int(k_cap), int(m_cap), _lib.ptr(cand.corners),
                                              _lib.ptr(cand.scores), _lib.ptr(cand.ctr), _lib.ptr(cand.classes),
                                              _lib.ptr(cand.locs), _lib.ptr(cand.levels), _lib.ptr(cand.hbox),
                                              _lib.ptr(cand.counts), _lib.ptr(ovf), _lib.ptr(ws), nbytes, _lib.current_stream()),
                   "dafne_tta_candidates_hip")
    return cand, ovf


class _CandSlice:
    """Images [i0, i1) of a Candidates (views of its tensors) for pp.select."""

    def __init__(self, cand, i0, i1):
        self.n, self.m_cap = i1 - i0, cand.m_cap
        for f in ("corners", "scores", "ctr", "classes", "locs", "levels", "hbox", "counts"):
            setattr(self, f, getattr(cand, f)[i0:i1])


def tta_select(cand, nms_thresh, post_topk):
    """pp.select over every image of `cand`, cut into launches whose NMS workspace stays under the limit nms_buckets uses."""
    from . import postprocess as pp
    L = _lib.load()
    per = max(L.dafne_poly_nms_workspace_bytes(1, cand.m_cap), 1)
    step = max(1, min(cand.n, _NMS_WS_LIMIT // per))
    if step >= cand.n:
        return pp.select(cand, nms_thresh, post_topk)
    parts = [pp.select(_CandSlice(cand, i0, min(i0 + step, cand.n)), nms_thresh, post_topk) for i0 in range(0, cand.n, step)]
    return torch.cat([k for k, _ in parts]), torch.cat([c for _, c in parts])


def _tta_scene_plan(tta, scenes, patch_size, overlap, layout_hwc):
    from .data.loader import inference_resize_shape
    m = tta.model
    cfg = m.cfg
    outs = m.proposal_generator.dafne_outputs
    if not outs.nms_thresh > 0:
        raise NotImplementedError("scene TTA with MODEL.DAFNE.NMS_TH <= 0 (the merge without NMS) is not supported")
    if len(getattr(tta.tta_mapper, "rotation_angles", ())):
        raise NotImplementedError("rotation TTA is not supported")
    patch = int(patch_size)
    origins, tiles = [], []
    for s, img in enumerate(scenes):
        h, w, hwc = scene_layout(img, layout_hwc)
        org = split_origins(h, w, patch, overlap)
        origins.append(org)
        tiles.extend((s, left, up, h, w, hwc) for left, up in org)
    nh, nw = inference_resize_shape(cfg, patch, patch)
    table = tta_view_table(tta.tta_mapper, nh, nw, (patch, patch))
    k_cap = outs.packed_k_cap()
    if k_cap * len(table) > 65536:
        raise NotImplementedError("scene TTA: %d views x %d rows per view exceed the rotated NMS's 65536 candidates"
                                  % (len(table), k_cap))
    # the per-image path's chunks (_batch_inference_packed: `batch_size` consecutive views per detector call, a chunk of
    # several sizes zero-padded to its largest view): a view's rows depend on its chunk's padded shape, so chunk j of every
    # tile of a batch goes through one detector call.  With 3 views per size (the released AUG) a chunk is one size.
    bs = max(1, int(tta.batch_size))
    chunks = [(a, min(a + bs, len(table))) for a in range(0, len(table), bs)]
    return patch, origins, tiles, (nh, nw), table, chunks


def tta_tile_rows(tta, scenes, patch_size=1024, overlap=200, batch=8, layout_hwc=None):
    """Every tile's merged TTA rows: (rows [T, k_cap, 18] f32, counts [T] int32, overflow [1] int32 -- all on the device --,
    tile_info [(left, up, scene)], origins per scene).  Tile t's rows[t, :counts[t]] are OneStageRCNNWithTTA's merged
    Instances of that tile (corners, scores, centerness, classes in keep order).  The host does not wait for the result.

    Batch b + 1's views and detector calls are enqueued before batch b's merge: the merge's descriptor upload (a pageable
    copy) returns once the caller's stream has reached it, i.e. after batch b's detections, and by then batch b + 1 keeps the
    GPU busy.  (A stream of its own for the views measured far slower, 0.24x the per-tile route.)"""
    from . import postprocess as pp
    from .data.loader import _to_chw_resized
    m = tta.model
    dev = m.device
    outs = m.proposal_generator.dafne_outputs
    with torch.cuda.device(dev):
        main = torch.cuda.current_stream()
        scenes = [x.to(dev).contiguous() for x in scenes]
        patch, origins, tiles, (nh, nw), table, chunks = _tta_scene_plan(tta, scenes, patch_size, overlap, layout_hwc)
        pre = (nh, nw) != (patch, patch)
        k_out = outs.packed_k_cap()

        def enqueue(bt):
            n = len(bt)
            if pre:
                # the test loader's resize of a tile file (data.loader.DAFNeTestMapper.finish); the views resample that image
                org = [[] for _ in scenes]
                for s, left, up, _, _, _ in bt:
                    org[s].append((left, up))
                hwc = gather_tiles(scenes, org, patch, layout_hwc)
                order = sorted(range(n), key=lambda i: bt[i][0])          # gather_tiles returns the tiles scene by scene
                srcs = [None] * n
                for j, i in enumerate(order):
                    srcs[i] = (_to_chw_resized(hwc[j], nh, nw), False, 0, 0, nh, nw)
            else:
                srcs = [(scenes[s], hwc, left, up, patch, patch) for s, left, up, _, _, hwc in bt]
            # detector calls of at most _TTA_VIEWS_PER_CALL views (whole tiles' chunks); they rotate over the compute streams as
            # in _views_packed: two for calls of 6 views or more, else three
            tpc = [max(1, min(n, _TTA_VIEWS_PER_CALL // (e - a))) for a, e in chunks]
            nstreams = 2 if max((e - a) * t for (a, e), t in zip(chunks, tpc)) >= 6 else 3
            pending = []
            ncall = 0
            for j, (a, e) in enumerate(chunks):
                shapes = [table[k][:2] for k in range(a, e)]
                hw = [shapes[k - a] for src in srcs for k in range(a, e)]          # tile-major: tile i's views of the chunk
                if len(set(shapes)) == 1:
                    vh, vw = shapes[0]
                    x = scene_views([src + (table[k][2], table[k][3]) for src in srcs for k in range(a, e)], vh, vw)
                else:                        # one views launch per size of the chunk, zero-padded into the chunk's batch
                    x = torch.zeros(len(hw), 3, max(h for h, _ in hw), max(w for _, w in hw), dtype=torch.uint8, device=dev)
                    for vh, vw in sorted(set(shapes)):
                        ks = [k for k in range(a, e) if shapes[k - a] == (vh, vw)]
                        y = scene_views([src + (table[k][2], table[k][3]) for src in srcs for k in ks], vh, vw)
                        q = 0
                        for i in range(n):
                            for k in ks:
                                x[i * (e - a) + k - a, :, :vh, :vw] = y[q]
                                q += 1
                # the arguments of OneStageRCNNWithTTA._views_packed: every view's rows are the per-image path's rows
                for t0 in range(0, n, tpc[j]):
                    t1 = min(n, t0 + tpc[j])
                    v0, v1 = t0 * (e - a), t1 * (e - a)
                    rows, counts = m.detect_packed(x[v0:v1], valid_hw=hw[v0:v1], out_hw=[(patch, patch)] * (v1 - v0),
                                                   do_postprocess=False, graphs=False, pipelined=True, splits=1,
                                                   stream_offset=ncall % nstreams)
                    ncall += 1
                    pending.append((a, e, t0, t1, rows, counts))
            done = torch.cuda.Event()
            done.record(m.side_stream)
            return n, pending, done

        def finish(state):
            n, pending, done = state
            main.wait_event(done)
            views = []
            for a, e, t0, t1, rows, counts in pending:
                rows.record_stream(main)
                counts.record_stream(main)
                q = 0
                for i in range(t0, t1):
                    for k in range(a, e):
                        views.append((rows[q], counts[q:q + 1], i, k, table[k]))
                        q += 1
            cand, ovf = tta_candidates(views, n, int(pending[0][4].shape[1]))
            keep, nk = tta_select(cand, outs.nms_thresh, max(outs.post_nms_topk, 0))
            r, c = pp.gather(cand, keep, nk, sizes=None, k_cap=k_out)
            return r, c, torch.maximum(ovf.max(), (c > k_out).to(torch.int32).max())

        done_parts, prev = [], None
        for b0 in range(0, len(tiles), max(1, int(batch))):
            cur = enqueue(tiles[b0:b0 + batch])
            if prev is not None:
                done_parts.append(finish(prev))
            prev = cur
        done_parts.append(finish(prev))
        rows = torch.cat([r for r, _, _ in done_parts])
        counts = torch.cat([c for _, c, _ in done_parts])
        overflow = torch.stack([f for _, _, f in done_parts]).max().reshape(1)
    info = [(left, up, s) for s, left, up, _, _, _ in tiles]
    return rows, counts, overflow, info, origins


def detect_scenes_tta(tta, scenes, patch_size=1024, overlap=200, batch=8, layout_hwc=None, tasks=("task1",), scales=(1,)):
    """OneStageRCNNWithTTA.detect_scenes: device uint8 BGR scenes -> merge_scenes' dicts per scene (plus "origins"); "tile" /
    "row" index the tiles' merged TTA rows.  The host reads what merge_scenes reads (and the overflow flag with it).
    scales: only (1,) -- the TTA views are cut from the scene itself, not from a resampled scene."""
    tasks = _check_tasks(tasks)
    if _check_scales(scales, "bicubic") != (1.0,):
        raise NotImplementedError("scene TTA with scales %r: the TTA views are cut from the scene itself; only scales=(1,) is "
                                  "built (detect_scenes takes scales)" % (tuple(scales),))
    if not scenes:
        return []
    m = tta.model
    cfg = m.cfg
    rows, counts, overflow, info, origins = tta_tile_rows(tta, scenes, patch_size, overlap, batch, layout_hwc)
    with torch.cuda.device(m.device):
        res = merge_scenes(rows, counts, info, len(scenes), int(cfg.MODEL.DAFNE.NUM_CLASSES), skip_mask(cfg),
                           task1_score_mode(cfg), overflow=overflow, tasks=tasks)
    for r, org in zip(res, origins):
        r["origins"] = org
    return res


def write_task1_merged(results, scene_names, classnames, dst):
    """Task1_<class>.txt per class, as ResultMerge_multi_process.mergesingle writes them: scenes in call order, each scene's
    detections in keep order, `name + " " + str(score) + " " + " ".join(map(str, coords))`."""
    os.makedirs(dst, exist_ok=True)
    host = []
    for r in results:
        host.append((r["corners"].cpu().numpy().astype(np.float64), r["scores"].cpu().numpy().astype(np.float64),
                     r["labels"].cpu().numpy()))
    for c, cname in enumerate(classnames):
        with open(os.path.join(dst, "Task1_%s.txt" % cname), "w") as f:
            for name, (corners, scores, labels) in zip(scene_names, host):
                for i in np.nonzero(labels == c)[0]:
                    f.write(name + " " + str(float(scores[i])) + " " + " ".join(map(str, corners[i].tolist())) + "\n")


def write_task2_merged(results, scene_names, classnames, dst):
    """Task2_<class>.txt per class, as ResultMerge_multi_process.mergesingle writes them for mergebyrec: scenes in call order,
    each scene's boxes in keep order, `name + " " + str(score) + " " + " ".join(map(str, [xmin, ymin, xmax, ymax]))`.
    results: detect_scenes(..., tasks=("task1", "task2"))."""
    if any("task2" not in r for r in results):
        raise ValueError("write_task2_merged: the results hold no \"task2\" entry (detect_scenes(..., tasks=(\"task1\", \"task2\")))")
    os.makedirs(dst, exist_ok=True)
    host = []
    for r in results:
        t = r["task2"]
        host.append((t["boxes"].cpu().numpy().astype(np.float64), t["scores"].cpu().numpy().astype(np.float64),
                     t["labels"].cpu().numpy()))
    for c, cname in enumerate(classnames):
        with open(os.path.join(dst, "Task2_%s.txt" % cname), "w") as f:
            for name, (boxes, scores, labels) in zip(scene_names, host):
                for i in np.nonzero(labels == c)[0]:
                    f.write(name + " " + str(float(scores[i])) + " " + " ".join(map(str, boxes[i].tolist())) + "\n")
