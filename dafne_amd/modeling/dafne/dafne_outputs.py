"""The reference's DAFNeOutputs (dafne/modeling/dafne/dafne_outputs.py) with the same method names and argument meaning,
backed by HIP kernels: the inference half (:123-190 config, :733-925) on the post-process kernels, and the forward VALUES of
the training half (:44-731) -- location-to-ground-truth assignment, centerness targets and the four loss terms -- on
csrc/targets_kernels.h.

Gradients with respect to the head outputs are built (loss_function.py: losses() on inputs that require grad returns
losses with a grad_fn, backed by dafne_losses_backward_hip), and so is the backward of the head's prediction layers (pred_backward.py:
OneStageDetector.backward_prediction_layers); the backward of the towers, the FPN and the backbone is not, so DAFNe.forward /
OneStageDetector.forward keep raising under ``self.training``.  One process: an
initialised process group with more than one rank raises NotImplementedError (the reference all-reduces num_pos and the
centerness sum, :44-50, 629, 665).
"""
import ctypes

import torch
from torch import nn

from ... import _lib
from ... import postprocess as pp
from ...structures import Instances
from ..nms.nms import ml_nms  # noqa: F401  (re-exported: the reference module imports it here)

INF = 100000000


def compute_ctrness_targets(reg_targets, alpha):
    """:79-93 on [n, 4] targets (abcd or ltrb): (min / max of left-right)(min / max of top-bottom) in the targets' dtype,
    raised to 1 / alpha, NaN -> 0.  Plain torch on whatever device the targets live on (a handful of elementwise launches: the
    loss kernel computes its own, this is the reference's module function for callers that want the values)."""
    if len(reg_targets) == 0:
        return reg_targets.new_zeros(len(reg_targets))
    left_right = reg_targets[:, [0, 2]]
    top_bottom = reg_targets[:, [1, 3]]
    ctrness = (left_right.min(dim=-1)[0] / left_right.max(dim=-1)[0]) * (top_bottom.min(dim=-1)[0] / top_bottom.max(dim=-1)[0])
    ctrness = ctrness ** (1 / alpha)
    ctrness[torch.isnan(ctrness)] = 0.0
    return ctrness


class Targets:
    """dafne_assign_targets_hip's outputs on the device, LEVEL first, then image, then location (the order of the
    reference's losses(), :527): labels / target_inds [P] int32, corners [P, 8], ltrb / abcd [P, 4] float32."""

    def __init__(self, n_images, shapes, strides, device):
        self.n_images, self.shapes, self.strides = int(n_images), [tuple(int(v) for v in s) for s in shapes], list(strides)
        P = self.n_images * sum(h * w for h, w in self.shapes)
        self.P = P
        self.labels = torch.empty(P, dtype=torch.int32, device=device)
        self.target_inds = torch.empty(P, dtype=torch.int32, device=device)
        self.corners = torch.empty(P, 8, dtype=torch.float32, device=device)
        self.ltrb = torch.empty(P, 4, dtype=torch.float32, device=device)
        self.abcd = torch.empty(P, 4, dtype=torch.float32, device=device)

    def level_slices(self):
        out, off = [], 0
        for h, w in self.shapes:
            out.append(slice(off, off + self.n_images * h * w))
            off += self.n_images * h * w
        return out


class DAFNeOutputs(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        d = cfg.MODEL.DAFNE
        self.pre_nms_thresh_test = d.INFERENCE_TH_TEST
        self.pre_nms_topk_test = d.PRE_NMS_TOPK_TEST
        self.post_nms_topk_test = d.POST_NMS_TOPK_TEST
        self.pre_nms_thresh = self.pre_nms_thresh_test
        self.pre_nms_topk = self.pre_nms_topk_test
        self.post_nms_topk = self.post_nms_topk_test
        self.nms_thresh = d.NMS_TH
        self.thresh_with_ctr = d.THRESH_WITH_CTR
        self.sort_corners = d.SORT_CORNERS
        self.centerness_mode = d.CENTERNESS
        self.has_centerness = self.centerness_mode != "none"
        assert self.centerness_mode in ["none", "plain", "oriented"]
        self.corner_prediction_strategy = d.CORNER_PREDICTION
        self.num_classes = d.NUM_CLASSES
        self.strides = d.FPN_STRIDES
        self.stride_norm = d.ENABLE_FPN_STRIDE_NORM
        # ---- target assignment and losses (:127-190)
        self.focal_loss_alpha = d.LOSS_ALPHA
        self.focal_loss_gamma = d.LOSS_GAMMA
        self.center_sample = d.CENTER_SAMPLE
        self.center_sample_only = d.CENTER_SAMPLE_ONLY
        self.combine_center_sample = d.COMBINE_CENTER_SAMPLE
        self.radius = d.POS_RADIUS
        self.in_box_check = d.ENABLE_IN_BOX_CHECK
        self.level_size_filtering = d.ENABLE_LEVEL_SIZE_FILTERING
        self.pre_nms_thresh_train = d.INFERENCE_TH_TRAIN
        self.pre_nms_topk_train = d.PRE_NMS_TOPK_TRAIN
        self.post_nms_topk_train = d.POST_NMS_TOPK_TRAIN
        self.loss_logspace = d.ENABLE_LOSS_LOG
        self.loss_beta = d.LOSS_SMOOTH_L1_BETA
        self.loss_modulation = d.ENABLE_LOSS_MODULATION
        self.centerness_alpha = d.CENTERNESS_ALPHA
        self.has_center_reg = self.corner_prediction_strategy == "center-to-corner"
        self.lambda_cls = d.LOSS_LAMBDA.CLS
        self.lambda_ctr = d.LOSS_LAMBDA.CTR
        self.lambda_corners = d.LOSS_LAMBDA.CORNERS
        self.lambda_center = d.LOSS_LAMBDA.CENTER
        self.lambda_ltrb = d.LOSS_LAMBDA.LTRB
        if d.LOSS_LAMBDA_NORM:
            self.normalize_lambdas()
        soi, prev_size = [], -1
        for sz in d.SIZES_OF_INTEREST:
            soi.append([prev_size, sz])
            prev_size = sz
        soi.append([prev_size, INF])
        self.sizes_of_interest = soi

    # ---- lambdas (:192-237)
    def normalize_lambdas(self):
        lambda_sum = self.lambda_cls + self.lambda_corners
        if self.has_centerness:
            lambda_sum += self.lambda_ctr
        if self.has_center_reg:
            lambda_sum += self.lambda_center
        self.lambda_cls = self.lambda_cls / lambda_sum
        self.lambda_ctr = self.lambda_ctr / lambda_sum
        self.lambda_corners = self.lambda_corners / lambda_sum
        self.lambda_center = self.lambda_center / lambda_sum
        self.lambda_ltrb = self.lambda_ltrb / lambda_sum

    def update_lambdas(self, lambda_cls=None, lambda_ctr=None, lambda_corners=None, lambda_center=None, normalize=False):
        lam = self.cfg.MODEL.DAFNE.LOSS_LAMBDA
        self.lambda_cls = lambda_cls if lambda_cls is not None else lam.CLS
        self.lambda_ctr = lambda_ctr if lambda_ctr is not None else lam.CTR
        self.lambda_corners = lambda_corners if lambda_corners is not None else lam.CORNERS
        self.lambda_center = lambda_center if lambda_center is not None else lam.CENTER
        if normalize:
            self.normalize_lambdas()

    # ---- target assignment (:252-503)
    def assign_targets(self, shapes, gt_instances, device):
        """shapes: (H, W) of every level; gt_instances: one Instances per image with gt_corners [G, 8], gt_boxes, gt_corners_area
        [G], gt_classes [G] (data.targets.make_gt_instances; host or device tensors) -- or the packed device arrays with device
        offsets (data.train_views.PackedGT), which are handed to the kernel as they are.  -> Targets.  The boxes of Instances
        go up in five copies; nothing is read back."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.DafneHipError("target assignment: the MI355X engine has no CPU path")
        if len(shapes) != len(self.strides) or len(shapes) != len(self.sizes_of_interest):
            raise ValueError("target assignment: %d levels, %d strides, %d sizes of interest"
                             % (len(shapes), len(self.strides), len(self.sizes_of_interest)))
        L = _lib.load()
        packed_gt = gt_instances if hasattr(gt_instances, "offsets") and hasattr(gt_instances, "corners") else None
        if packed_gt is not None:
            # the packed device arrays of dafne_train_gt_hip / dafne_scene_pack_tile_gt_hip (data.train_views.PackedGT): corners
            # [G, 8], hbox [G, 4], area [G] f32, classes [G] int32, offsets [n + 1] int32, all on the device.  Nothing is copied
            # or read: the offsets stay where they are, G (the allocation) bounds the rows.
            n = int(packed_gt.offsets.shape[0]) - 1
            n_gt = int(packed_gt.corners.shape[0])
            for t, dt in ((packed_gt.corners, torch.float32), (packed_gt.hbox, torch.float32), (packed_gt.area, torch.float32),
                          (packed_gt.classes, torch.int32), (packed_gt.offsets, torch.int32)):
                if t.device != dev or t.dtype != dt or not t.is_contiguous():
                    raise ValueError("target assignment: the packed ground truth must be contiguous fp32 / int32 tensors on %s" % (dev,))
            if packed_gt.hbox.shape[0] != n_gt or packed_gt.area.shape[0] != n_gt or packed_gt.classes.shape[0] != n_gt:
                raise ValueError("target assignment: the packed arrays hold different row counts")
        else:
            n = len(gt_instances)
            counts = [len(g.gt_classes) for g in gt_instances]
            offsets = [0]
            for c in counts:
                offsets.append(offsets[-1] + c)
            n_gt = offsets[-1]

        def packed(get, width, dtype):
            parts = [get(g).detach().reshape(-1, width).to(dtype) for g in gt_instances]
            t = torch.cat(parts, 0) if parts else torch.zeros(0, width, dtype=dtype)
            return t.to(dev, non_blocking=True).contiguous()
        tg = Targets(n, shapes, self.strides, dev)
        prm = _lib.TargetParams()
        prm.n_images, prm.n_levels, prm.n_classes = n, len(shapes), self.num_classes
        prm.flags = ((_lib.TGT_CENTER_SAMPLE if self.center_sample else 0)
                     | (_lib.TGT_CENTER_SAMPLE_ONLY if self.center_sample_only else 0)
                     | (_lib.TGT_COMBINE_CENTER_SAMPLE if self.combine_center_sample else 0)
                     | (_lib.TGT_IN_BOX_CHECK if self.in_box_check else 0)
                     | (_lib.TGT_LEVEL_SIZE_FILTERING if self.level_size_filtering else 0)
                     | (_lib.TGT_FPN_STRIDE_NORM if self.stride_norm else 0))
        for l, ((h, w), s) in enumerate(zip(tg.shapes, self.strides)):
            prm.H[l], prm.W[l], prm.stride[l] = h, w, int(s)
            prm.size_lo[l], prm.size_hi[l] = float(self.sizes_of_interest[l][0]), float(self.sizes_of_interest[l][1])
            prm.radius[l] = float(s * self.radius)       # get_sample_region: strides[level] * radius (:327)
        with torch.cuda.device(dev):
            if packed_gt is not None:
                corners, hbox, area, cls, off = packed_gt.corners, packed_gt.hbox, packed_gt.area, packed_gt.classes, packed_gt.offsets
            else:
                corners = packed(lambda g: g.gt_corners, 8, torch.float32)
                hbox = packed(lambda g: g.gt_boxes.tensor, 4, torch.float32)
                area = packed(lambda g: g.gt_corners_area, 1, torch.float32)
                cls = packed(lambda g: g.gt_classes, 1, torch.int32)
                off = torch.tensor(offsets, dtype=torch.int32).to(dev, non_blocking=True)
            _lib.check(L.dafne_assign_targets_hip(
                ctypes.byref(prm), _lib.ptr(corners), _lib.ptr(hbox), _lib.ptr(area), _lib.ptr(cls), _lib.ptr(off), n_gt,
                _lib.ptr(tg.labels), _lib.ptr(tg.target_inds), _lib.ptr(tg.corners), _lib.ptr(tg.ltrb), _lib.ptr(tg.abcd),
                _lib.current_stream()), "dafne_assign_targets_hip")
            for t in (corners, hbox, area, cls, off):
                t.record_stream(torch.cuda.current_stream())
        return tg

    def _get_ground_truth(self, locations, gt_instances):
        """:252-295: the reference's dict -- labels, target_inds, reg_targets_corners / ltrb / abcd, locations, im_inds,
        fpn_levels -- as level-first lists in (image, location) order; the first five are views into the kernel's buffers
        (int32 where the reference has int64).  ``locations``: DAFNe.compute_locations' per-level [H W, 2] tensors, from
        which the level shapes are read (one host read per level); the kernel regenerates the locations themselves."""
        locations = list(locations)
        if not locations or not locations[0].is_cuda:
            raise _lib.DafneHipError("_get_ground_truth: the MI355X engine has no CPU path (got CPU locations)")
        shapes = []
        for loc, s in zip(locations, self.strides):
            w = (int(loc[-1, 0].item()) - s // 2) // s + 1
            shapes.append((loc.shape[0] // w, w))
        tg = self.assign_targets(shapes, gt_instances, locations[0].device)
        return self._targets_dict(tg, locations)

    @staticmethod
    def _targets_dict(tg, locations):
        n = tg.n_images
        sl = tg.level_slices()
        return {
            "labels": [tg.labels[s] for s in sl],
            "target_inds": [tg.target_inds[s] for s in sl],
            "reg_targets_corners": [tg.corners[s] for s in sl],
            "reg_targets_ltrb": [tg.ltrb[s] for s in sl],
            "reg_targets_abcd": [tg.abcd[s] for s in sl],
            "locations": [loc.repeat(n, 1) for loc in locations],
            "im_inds": [torch.arange(n, device=loc.device).repeat_interleave(loc.shape[0]) for loc in locations],
            "fpn_levels": [torch.full((n * loc.shape[0],), l, dtype=torch.long, device=loc.device)
                           for l, loc in enumerate(locations)],
        }

    # ---- losses (:505-731)
    @staticmethod
    def _require_device(tensors):
        if not all(t.is_cuda for t in tensors):
            raise _lib.DafneHipError("losses: the MI355X engine has no CPU path (got CPU tensors)")

    def losses(self, logits_pred, corners_reg_pred, center_reg_pred, ltrb_reg_pred, ctrness_pred, locations, gt_instances,
               top_feats=None):
        """The reference's eight arguments: per-level NCHW tensors as DAFNeHead.forward returns them (``locations`` is accepted
        and ignored: the kernel regenerates them; ltrb_reg_pred / top_feats are unused there too).  -> (extras, losses):
        losses {"loss/cls", "loss/corners", "loss/center" with a center regression, "loss/ctr" with centerness} as 0-dim fp32
        device tensors, extras {"loss_denorm", "num_pos"} likewise (plus "values_f64", the kernel's fp64 row).  No host read.
        With grad mode on and any of logits_pred / corners_reg_pred / center_reg_pred / ctrness_pred requiring grad, the four
        losses come from loss_function.DafneLossFunction and carry a grad_fn (same values, same extras)."""
        self._require_device(list(logits_pred) + list(corners_reg_pred))
        heads = list(logits_pred) + list(corners_reg_pred)
        heads += list(center_reg_pred) if self.has_center_reg else []
        heads += list(ctrness_pred) if self.has_centerness else []
        if torch.is_grad_enabled() and any(t.requires_grad for t in heads):
            from .loss_function import losses_with_grad
            return losses_with_grad(self, logits_pred, corners_reg_pred, center_reg_pred, ctrness_pred, gt_instances)

        def nhwc(t):
            return t.detach().float().permute(0, 2, 3, 1).contiguous()
        levels = []
        for l, s in enumerate(self.strides):
            ce = nhwc(center_reg_pred[l]) if self.has_center_reg else None
            ct = nhwc(ctrness_pred[l]) if self.has_centerness else None
            levels.append(pp.LevelInput(nhwc(logits_pred[l]), nhwc(corners_reg_pred[l]), ce, ct, s, 1.0))
        tg = self.assign_targets([(lv.H, lv.W) for lv in levels], gt_instances, levels[0].logits.device)
        return self.dafne_losses_packed(levels, tg, cooked=True)

    def dafne_losses_packed(self, levels, targets, cooked=False, want_ctr_targets=False, _call=None):
        """dafne_losses (:620-731) on the head's raw per-level outputs (postprocess.LevelInput, NHWC, no copies: what
        head_levels gives) and assign_targets' Targets.  cooked: the levels hold the finished regressions (losses()).
        _call: a dict that receives what a following dafne_losses_backward_hip needs (loss_function.py)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("the loss kernel is single-process: the reference all-reduces num_pos and the centerness "
                                      "sum over the ranks (dafne_outputs.py:629, 665)")
        L = _lib.load()
        dev = levels[0].logits.device
        if dev.type != "cuda":
            raise _lib.DafneHipError("losses: the MI355X engine has no CPU path (got CPU tensors)")
        n = levels[0].N
        if n != targets.n_images or [(lv.H, lv.W) for lv in levels] != targets.shapes:
            raise ValueError("losses: the targets were assigned for another batch / pyramid")
        if self.has_center_reg and any(lv.center is None for lv in levels):
            raise ValueError("losses: CORNER_PREDICTION center-to-corner needs the center regression")
        if self.has_centerness and any(lv.ctrness is None for lv in levels):
            raise ValueError("losses: CENTERNESS %r needs the centerness logits" % self.centerness_mode)
        prm = _lib.LossParams()
        prm.n_images, prm.n_levels, prm.n_classes = n, len(levels), self.num_classes
        prm.flags = ((_lib.LOSS_LOGSPACE if self.loss_logspace else 0) | (_lib.LOSS_MODULATION if self.loss_modulation else 0)
                     | (_lib.LOSS_SORT_CORNERS if self.sort_corners else 0) | (_lib.LOSS_HAS_CENTER_REG if self.has_center_reg else 0)
                     | (_lib.LOSS_COOKED if cooked else 0)
                     | {"plain": _lib.LOSS_CTR_PLAIN, "oriented": _lib.LOSS_CTR_ORIENTED, "none": 0}[self.centerness_mode])
        prm.alpha, prm.gamma, prm.beta = float(self.focal_loss_alpha), float(self.focal_loss_gamma), float(self.loss_beta)
        prm.ctr_alpha = float(self.centerness_alpha)
        prm.lambda_cls, prm.lambda_corners = float(self.lambda_cls), float(self.lambda_corners)
        prm.lambda_center, prm.lambda_ctr = float(self.lambda_center), float(self.lambda_ctr)
        descs = (_lib.LevelDesc * len(levels))()
        for i, lv in enumerate(levels):
            for t in (lv.logits, lv.delta, lv.center, lv.ctrness):
                assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous())
            descs[i] = _lib.LevelDesc(lv.logits.data_ptr(), lv.delta.data_ptr(), _lib.ptr(lv.center), _lib.ptr(lv.ctrness),
                                      lv.logits_ps, lv.delta_ps, lv.center_ps, lv.ctrness_ps, lv.H, lv.W, lv.stride, lv.scale)
        with torch.cuda.device(dev):
            nbytes = L.dafne_losses_workspace_bytes(ctypes.byref(prm), descs)
            if nbytes == 0:
                raise _lib.DafneHipError("dafne_losses_workspace_bytes: bad parameters / level table")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            row = torch.empty(6, dtype=torch.float64, device=dev)
            ctr_t = torch.empty(targets.P, dtype=torch.float32, device=dev) if want_ctr_targets else None
            _lib.check(L.dafne_losses_hip(ctypes.byref(prm), descs, _lib.ptr(targets.labels), _lib.ptr(targets.corners),
                                          _lib.ptr(targets.ltrb), _lib.ptr(targets.abcd), _lib.ptr(row), _lib.ptr(ctr_t),
                                          _lib.ptr(ws), nbytes, _lib.current_stream()), "dafne_losses_hip")
            r32 = row.to(torch.float32)
        if _call is not None:
            _call.update(prm=prm, descs=descs, ws=ws, ws_bytes=nbytes)
        losses = {"loss/cls": r32[0], "loss/corners": r32[1]}
        if self.has_center_reg:
            losses["loss/center"] = r32[2]
        if self.has_centerness:
            losses["loss/ctr"] = r32[3]
        extras = {"loss_denorm": r32[5], "num_pos": r32[4], "values_f64": row}
        if want_ctr_targets:
            extras["ctr_targets"] = ctr_t
        return extras, losses

    # ---- fused device path used by the engine ---------------------------------
    def predict_packed(self, levels, sizes=None, k_cap=None, scale_corners=True):
        """levels: list[postprocess.LevelInput] (NHWC fp32).  Returns (rows, counts):
        [N,k_cap,18] float32 detections and their per-image counts, on the GPU."""
        cand = self.decode_packed(levels)
        return self.select_packed(cand, sizes=sizes, k_cap=k_cap, scale_corners=scale_corners)

    def decode_packed(self, levels, out=None):
        if not self.stride_norm:
            # ENABLE_FPN_STRIDE_NORM false (dafne_outputs.py:771-774): the regression is already in pixels.  The decode kernel
            # computes (reg * scale) * stride; with scale / stride for a power-of-two stride both products only shift the
            # exponent, so the result has the bits of reg * scale (no other rounding: tests/test_gpu_decode.py)
            adj = []
            for lv in levels:
                if lv.stride <= 0 or lv.stride & (lv.stride - 1):
                    raise NotImplementedError("ENABLE_FPN_STRIDE_NORM=False with an FPN stride that is not a power of two (%d)" % lv.stride)
                adj.append(pp.LevelInput(lv.logits, lv.delta, lv.center, lv.ctrness, lv.stride, lv.scale / lv.stride,
                                         delta_ps=lv.delta_ps, center_ps=lv.center_ps, ctrness_ps=lv.ctrness_ps,
                                         logits_ps=lv.logits_ps))
            levels = adj
        return pp.decode_levels(levels, num_classes=self.num_classes, pre_nms_thresh=self.pre_nms_thresh_test,
                                pre_nms_topk=self.pre_nms_topk_test, thresh_with_ctr=self.thresh_with_ctr,
                                sort_corners=self.sort_corners, out=out)

    def packed_k_cap(self, n_levels=5):
        """Row capacity of the packed detections select_packed returns by default -- what a caller sizing a gather
        buffer must use (tools/eval_net.py, evaluation/driver.py) instead of restating the rule."""
        m_cap = n_levels * self.pre_nms_topk_test
        return min(m_cap, max(self.post_nms_topk_test, 1) + 256) if self.post_nms_topk_test > 0 else m_cap

    def select_packed(self, cand, sizes=None, k_cap=None, scale_corners=True):
        if self.nms_thresh > 0:
            keep, nk = pp.select(cand, self.nms_thresh, self.post_nms_topk_test)
        else:   # ml_nms returns its input unchanged (nms.py:22-23); only the cap applies
            keep, nk = _identity_keep_with_cap(cand, self.post_nms_topk_test)
        if k_cap is None:
            k_cap = self.packed_k_cap(cand.m_cap // max(self.pre_nms_topk_test, 1))
        return pp.gather(cand, keep, nk, sizes=sizes, k_cap=k_cap, scale_corners=scale_corners)

    # ---- reference-signature path ----------------------------------------------
    def predict_proposals(self, logits_pred, corners_reg_pred, ctrness_pred, locations, image_sizes,
                          top_feats=None):
        """Same arguments as the reference (:733-741): per-level NCHW tensors, with
        corners_reg_pred already (center.repeat + delta) * scale.  ``locations`` is
        accepted for signature parity; the kernel regenerates them (dafne.py:37-44)."""
        levels = []
        for lg, rc, ct, s in zip(logits_pred, corners_reg_pred, ctrness_pred, self.strides):
            lg_n = lg.detach().float().permute(0, 2, 3, 1).contiguous()
            rc_n = rc.detach().float().permute(0, 2, 3, 1).contiguous()
            # CENTERNESS none: the head's dummy ones are not read (dafne_outputs.py:810-830, score = sigmoid(cls))
            ct_n = ct.detach().float().permute(0, 2, 3, 1).contiguous() if self.has_centerness else None
            levels.append(pp.LevelInput(lg_n, rc_n, None, ct_n, s, 1.0))
        rows, counts = self.predict_packed(levels)
        sizes = [tuple(int(v) for v in (s.tolist() if isinstance(s, torch.Tensor) else s)) for s in image_sizes]
        return pp.rows_to_instances(rows, counts, sizes)

    def select_over_all_levels(self, boxlists):
        """:907-925, Instances in / Instances out (used by the TTA merge, tta.py:265): ml_nms, then the kthvalue cap
        with ties.  Both steps are one device call (dafne_select_over_all_levels_hip) and one host wait per image."""
        results = []
        for bl in boxlists:
            n = len(bl)
            if self.nms_thresh <= 0 or n == 0:          # ml_nms returns its input unchanged (nms.py:22-25)
                result = bl
                if n > self.post_nms_topk > 0:
                    s = result.scores
                    thr = torch.kthvalue(s, n - self.post_nms_topk + 1).values
                    result = result[torch.nonzero(s >= thr).squeeze(1)]
                results.append(result)
                continue
            if not bl.pred_corners.is_cuda:
                raise _lib.DafneHipError("select_over_all_levels: the MI355X engine has no CPU path (got CPU tensors)")
            L = _lib.load()
            dev = bl.pred_corners.device
            with torch.cuda.device(dev):
                b = bl.pred_corners.detach().to(torch.float32).contiguous()
                sc = bl.scores.detach().to(torch.float32).contiguous()
                c = bl.pred_classes.detach().to(torch.int32).contiguous()
                keep = torch.empty(n, dtype=torch.int64, device=dev)
                nk = torch.zeros(1, dtype=torch.int32, device=dev)
                nbytes = L.dafne_poly_nms_workspace_bytes(1, n)
                ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
                _lib.check(L.dafne_select_over_all_levels_hip(
                    _lib.ptr(b), _lib.ptr(sc), _lib.ptr(c), None, 1, n, float(self.nms_thresh),
                    int(max(self.post_nms_topk, 0)), _lib.ptr(keep), _lib.ptr(nk), _lib.ptr(ws), nbytes, 0,
                    _lib.current_stream()), "dafne_select_over_all_levels_hip")
                results.append(bl[keep[: int(nk.item())]])
        return results


def _identity_keep_with_cap(cand, post_topk):
    n, m = cand.n, cand.m_cap
    dev = cand.scores.device
    keep = torch.arange(m, device=dev, dtype=torch.int64).repeat(n, 1)
    nk = cand.counts.clone()
    if post_topk > 0:
        raise NotImplementedError("NMS_TH <= 0 with a post-NMS cap is not used by any released config")
    return keep, nk
