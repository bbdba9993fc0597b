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
  merge_tile_rows(...)                          tile rows -> per-(scene, class) f64 merge rows + back-index
  merge_scenes(...)                             the above + NMS + the kept rows per scene
  detect_scenes(model, scenes, ...)             OneStageDetector.detect_scenes
  write_task1_merged(results, names, classes, dst)
"""
import os

import numpy as np
import torch

from . import _lib

NMS_THRESH = 0.1          # ResultMerge_multi_process.py:22
# NMS workspace per launch: the buckets of a call are cut into launches of at most this many bytes
_NMS_WS_LIMIT = 1 << 31


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


def task1_score_mode(cfg):
    """1 where evaluation.task1.task1_scores writes score^2 / centerness (CENTERNESS != none, not CENTERNESS_USE_IN_SCORE)."""
    d = cfg.MODEL.DAFNE
    return 1 if (d.CENTERNESS != "none" and not d.CENTERNESS_USE_IN_SCORE) else 0


def skip_mask(cfg):
    """Labels _generate_task_1_files leaves out: DOTA-1.5's container-crane (15) with DATASETS.DOTA_REMOVE_CONTAINER_CRANE."""
    return (1 << 15) if bool(cfg.DATASETS.DOTA_REMOVE_CONTAINER_CRANE) else 0


def merge_tile_rows(rows, counts, tile_info, n_scenes, n_classes, skip=0, score_mode=0, m_cap=None):
    """rows [T,k_cap,18] f32 + counts [T] (device) + tile_info [T,3] int32 (left, up, scene) -> (dets [B,m_cap,9] f64,
    bucket counts [B] int32, src [B,m_cap] int32, m_cap) with B = n_scenes * n_classes.  m_cap None: sized from the bucket
    counts (a host read of B integers)."""
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

        def call(cap, dets, src):
            _lib.check(L.dafne_scene_merge_rows_hip(_lib.ptr(rows), _lib.ptr(counts), T, k_cap, _lib.ptr(info), int(n_scenes),
                                                    int(n_classes), int(skip), int(score_mode), int(cap), _lib.ptr(dets),
                                                    _lib.ptr(bcount), _lib.ptr(src), _lib.ptr(ws), nbytes, _lib.current_stream()),
                       "dafne_scene_merge_rows_hip")
        if m_cap is None:
            call(0, None, None)
            m_cap = max(int(bcount.max().item()), 1)
        dets = torch.empty((nb, m_cap, 9), dtype=torch.float64, device=dev)
        src = torch.empty((nb, m_cap), dtype=torch.int32, device=dev)
        call(m_cap, dets, src)
    return dets, bcount, src, m_cap


def nms_buckets(dets, bcount, m_cap, thresh=NMS_THRESH):
    """The tile merge's NMS (strict hull test) on every bucket, on the device: -> keep [B,m_cap] int64, num_keep [B]."""
    L = _lib.load()
    dev = dets.device
    nb = int(dets.shape[0])
    keep = torch.empty((nb, m_cap), dtype=torch.int64, device=dev)
    nk = torch.zeros(nb, dtype=torch.int32, device=dev)
    per = max(L.dafne_poly_nms_f64_workspace_bytes(1, m_cap), 1)
    step = max(1, min(nb, _NMS_WS_LIMIT // per))
    with torch.cuda.device(dev):
        nbytes = L.dafne_poly_nms_f64_workspace_bytes(step, m_cap)
        if nbytes == 0:
            raise _lib.DafneHipError("poly_nms_f64: bad size %d x %d" % (step, m_cap))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        for b0 in range(0, nb, step):
            n = min(step, nb - b0)
            _lib.check(L.dafne_poly_nms_f64_batched_hip(_lib.ptr(dets[b0:b0 + n]), _lib.ptr(bcount[b0:b0 + n]), n, m_cap,
                                                        float(thresh), 1, _lib.ptr(keep[b0:b0 + n]), _lib.ptr(nk[b0:b0 + n]),
                                                        _lib.ptr(ws), nbytes, 0, _lib.current_stream()),
                       "dafne_poly_nms_f64_batched_hip")
    return keep, nk


def merge_scenes(rows, counts, tile_info, n_scenes, n_classes, skip=0, score_mode=0):
    """Tile rows -> per scene {"corners" [K,8] f64, "scores" [K] f64, "labels" [K] int64, "tile" [K], "row" [K]}: class by
    class, each class in the NMS keep order (descending score) -- what mergebypoly writes for that scene."""
    k_cap = int(rows.shape[1])
    dets, bcount, src, m_cap = merge_tile_rows(rows, counts, tile_info, n_scenes, n_classes, skip, score_mode)
    keep, nk = nms_buckets(dets, bcount, m_cap)
    dev = dets.device
    nb = dets.shape[0]
    # the kept rows of every bucket, bucket-major (scene, then class): one host read, the kept counts
    valid = torch.arange(m_cap, device=dev)[None, :] < nk[:, None].to(torch.int64)
    flat = (torch.arange(nb, device=dev, dtype=torch.int64)[:, None] * m_cap + keep.clamp(0, m_cap - 1))[valid]
    d = dets.reshape(-1, 9)[flat]
    s = src.reshape(-1)[flat].to(torch.int64)
    lab = (torch.arange(nb, device=dev, dtype=torch.int64)[:, None].expand(nb, m_cap) % n_classes)[valid]
    per_scene = nk.reshape(n_scenes, n_classes).sum(1).cpu().tolist()
    out = []
    o = 0
    for k in per_scene:
        out.append({"corners": d[o:o + k, :8], "scores": d[o:o + k, 8], "labels": lab[o:o + k],
                    "tile": s[o:o + k] // k_cap, "row": s[o:o + k] % k_cap})
        o += k
    return out


def detect_scenes(model, scenes, patch_size=1024, overlap=200, batch=8, layout_hwc=None):
    """OneStageDetector.detect_scenes: device uint8 BGR scenes (HWC or CHW) -> one result per scene (merge_scenes' dicts,
    plus "origins": the scene's tile origins in split order).  Tiles of all scenes go through detect_packed(pipelined=True)
    in batches of `batch` (the engine is batch-invariant: a tile's detections do not depend on its batch)."""
    from .data.loader import _to_chw_resized, inference_resize_shape
    if not scenes:
        return []
    cfg = model.cfg
    dev = model.device
    patch = int(patch_size)
    origins = []
    info = []
    for s, img in enumerate(scenes):
        h, w, _ = scene_layout(img, layout_hwc)
        org = split_origins(h, w, patch, overlap)
        origins.append(org)
        info.extend((left, up, s) for left, up in org)
    with torch.cuda.device(dev):
        tiles = gather_tiles([x.to(dev) for x in scenes], origins, patch, layout_hwc)
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
        rows = torch.cat([r for r, _ in parts])
        counts = torch.cat([c for _, c in parts])
        res = merge_scenes(rows, counts, info, len(scenes), int(cfg.MODEL.DAFNE.NUM_CLASSES), skip_mask(cfg), task1_score_mode(cfg))
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
