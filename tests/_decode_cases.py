"""Shared inputs of tests/test_decode_cases_cpu.py and tests/test_gpu_decode_edges.py: one table of decode / top-k cases, every
case and its oracle result made once.

Inputs are quantised so that the comparison with the oracle is exact instead of "within a few candidates":
  scores   class and centerness logits are integers in [-8, 8] (fp32).  The oracle's distinct values of sqrt(sigmoid(a) *
           sigmoid(b)) then lie at least 2.9e-4 apart (relative), about 2 400 fp32 ulps, while the device's expf may differ from
           numpy's exp by a few ulps: which candidates are selected, and in which order, is fully determined, and equal inputs give
           equal scores on either side.  Hand-placed values outside the grid: 30 (sigmoid exactly 1.0) only.
  corners  delta and center are integers in [-8, 8], scale is 1.0 or 0.5, strides are powers of two: every fp32 operation of the
           box decode is exact, so corners, hbox and locations must equal the oracle's bit for bit (the corner sort included: it
           compares exact values).  The grid is coarse enough to give collinear and coincident quads, where the sort leaves zeros.
tests/test_decode_cases_cpu.py checks on the oracle alone that every case reaches the regime its `why` names."""
import types

import numpy as np

from oracle import postprocess as opp

F32 = np.float32
K_CHUNK, K_BINS, K_MAX_TOPK, K_MAX_LEVELS, K_FIN_THREADS = 4096, 2048, 4096, 8, 1024     # dafne_amd/csrc/decode.hip
NO_CENTER, NO_CTRNESS = 1, 2                                                             # dafne_decode_params.flags
RAGGED = [(40, 56, 8, 1.0), (20, 28, 16, 0.5), (5, 7, 64, 1.0)]
LOGITS_PAD = 20      # logits_ps of the fused9 layout: C real channels, the rest +30 (a read of one becomes a top candidate)

CASES = {}


def _add(name, why, levels, C, topk, edit=None, *, N=2, thresh=0.05, twc=True, sortc=True, flags=0, layout="packed", seed=0,
         same_as=None, **claims):
    """claims (checked on the oracle by test_decode_cases_cpu.py):
      count     {(image, level): ">" | "<" | "==" | "+1" | "0"}: the candidate count against topk (+1: topk + 1; 0: none)
      cut_tie   [(image, level)]: the cut score is held by at least one taken and at least one rejected candidate
      taken     [(image, level, flat index)]: selected elements
      lowest    [(image, level)]: the selection is exactly the topk lowest flat indices
      zero_quad the corner sort leaves p2..p4 of some quads zero (no vertex qualifies), and at least one quad all zero
      at_thresh [(image, level)]: elements whose thresholded value equals the threshold exist (and are no candidates)"""
    assert name not in CASES and len(levels) <= K_MAX_LEVELS and N <= 3
    assert all(h * w * C <= 40 * 56 * 15 and (s & (s - 1)) == 0 and sc in (1.0, 0.5) for h, w, s, sc in levels)
    CASES[name] = types.SimpleNamespace(name=name, why=why, N=N, C=C, levels=levels, topk=topk, thresh=thresh, twc=twc, sortc=sortc,
                                        flags=flags, layout=layout, seed=seed, edit=edit, same_as=same_as, claims=claims)


def _grid(rng, shape, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, shape).astype(F32)


_ARRAYS, _REFS = {}, {}


def arrays(case):
    """-> per level dict(lg [N,H,W,C], dl [N,H,W,8], ce [N,H,W,2], ct [N,H,W,1]) fp32 on the host: the logical inputs, whatever
    the layout they reach the device in.  ce is None with NO_CENTER, ct None with NO_CTRNESS."""
    key = case.same_as or case.name
    if key not in _ARRAYS:
        src = CASES[key]
        rng = np.random.default_rng(src.seed)
        lv = []
        for h, w, _, _ in src.levels:
            lv.append(dict(lg=_grid(rng, (src.N, h, w, src.C)), dl=_grid(rng, (src.N, h, w, 8)), ce=_grid(rng, (src.N, h, w, 2)),
                           ct=_grid(rng, (src.N, h, w, 1))))
        if src.edit is not None:
            src.edit(src, lv, rng)
        for a in lv:
            if src.flags & NO_CENTER:
                a["ce"] = None
            if src.flags & NO_CTRNESS:
                a["ct"] = None
            for v in a.values():
                if v is not None:
                    v.setflags(write=False)
        _ARRAYS[key] = lv
    return _ARRAYS[key]


def thresholded_and_score(case, im, l):
    """([HW,C] value the threshold is applied to, [HW,C] ranked score) of one image and level, with the oracle's sigmoid32."""
    a = arrays(case)[l]
    cls = opp.sigmoid32(a["lg"][im].reshape(-1, case.C))
    if case.flags & NO_CTRNESS:
        return cls, cls
    ctr = opp.sigmoid32(a["ct"][im].reshape(-1))
    sc = np.sqrt(cls * ctr[:, None], dtype=F32)
    return (sc if case.twc else cls), sc


def _decode_level_no_ctrness(logits, reg, stride, *, thresh, topk, sort_corners, level):
    """dafne_outputs.py:792-905 for CENTERNESS none: oracle.postprocess.decode_level without the centerness factor and the square
    root (:810-829), built from the oracle's own parts (the restatement tests/test_gpu_ablation_head.py checks against the
    reference's goldens)."""
    C, H, W = logits.shape
    loc = opp.compute_locations(H, W, stride)
    rcf = np.transpose((reg.astype(F32) * F32(stride)).astype(F32), (1, 2, 0)).reshape(-1, 8)
    cls = opp.sigmoid32(np.transpose(logits, (1, 2, 0)).reshape(-1, C))
    li, ci = np.nonzero(cls > F32(thresh))
    sc = cls[li, ci]
    if li.shape[0] > topk:
        order = np.lexsort((li.astype(np.int64) * C + ci, -sc.astype(np.float64)))
        sel = np.sort(order[:topk])
        li, ci, sc = li[sel], ci[sel], sc[sel]
    poly = np.empty((li.shape[0], 8), F32)
    for j in range(8):
        poly[:, j] = (loc[li, j % 2] + rcf[li, j]).astype(F32)
    if sort_corners:
        poly = opp.sort_quadrilateral(poly)
    hb = (np.stack((poly[:, 0::2].min(1), poly[:, 1::2].min(1), poly[:, 0::2].max(1), poly[:, 1::2].max(1)), axis=1)
          if poly.shape[0] else np.zeros((0, 4), F32))
    return {"pred_boxes": hb.astype(F32), "pred_corners": poly, "scores": sc.astype(F32),
            "centerness": np.ones(li.shape[0], F32), "pred_classes": ci.astype(np.int64),
            "locations": loc[li].astype(F32), "fpn_levels": np.full(li.shape[0], level, np.int64)}


def reference(case):
    """-> per image (list of the oracle's per-level results, their concatenation); computed once, never written to."""
    key = case.same_as or case.name
    if key not in _REFS:
        src, lv, out = CASES[key], arrays(case), []
        for im in range(src.N):
            per = []
            for l, (h, w, s, scale) in enumerate(src.levels):
                a = lv[l]
                reg = a["dl"][im] if src.flags & NO_CENTER else (np.tile(a["ce"][im], (1, 1, 4)) + a["dl"][im]).astype(F32)
                reg = np.transpose((reg * F32(scale)).astype(F32), (2, 0, 1))
                lg = np.transpose(a["lg"][im], (2, 0, 1))
                if src.flags & NO_CTRNESS:
                    per.append(_decode_level_no_ctrness(lg, reg, s, thresh=src.thresh, topk=src.topk, sort_corners=src.sortc,
                                                        level=l))
                else:
                    per.append(opp.decode_level(lg, reg, np.transpose(a["ct"][im], (2, 0, 1)), s, thresh=src.thresh,
                                                topk=src.topk, thresh_with_ctr=src.twc, sort_corners=src.sortc, level=l))
            tot = opp.cat(per)
            for v in tot.values():
                v.setflags(write=False)
            out.append((per, tot))
        _REFS[key] = out
    return _REFS[key]


def flat_index(case, l, det):
    """Flat element index (location major, class minor) of the oracle's rows of level l."""
    h, w, s, _ = case.levels[l]
    x = ((det["locations"][:, 0] - F32(s // 2)) / F32(s)).astype(np.int64)
    y = ((det["locations"][:, 1] - F32(s // 2)) / F32(s)).astype(np.int64)
    return (y * w + x) * case.C + det["pred_classes"]


# ------------------------------------------------------------------------------------------------------------------ the cases
_EVERY = [(im, l) for im in range(2) for l in range(2)]

def _edit_ragged(case, lv, rng):
    """Level 1's first pixel decodes to four corners at (0, 0) (location 8 + 8 * (center -1 + delta 0) at stride 16, scale 0.5)
    and is every image's best candidate there: coincident points, the sort leaves p2..p4 zero and p1 is the origin."""
    a = lv[1]
    a["dl"][:, 0, 0] = 0
    a["ce"][:, 0, 0] = -1
    a["lg"][:, 0, 0, 0] = 8
    a["ct"][:, 0, 0] = 8


for _twc in (True, False):
    _add("cut-ragged-twc" if _twc else "cut-ragged-notwc",
         "several chunks with a ragged last one (33600 = 8 x 4096 + 832, 8400 = 2 x 4096 + 208), a topk that is no power of two "
         "(kp 1024 holds 24 padding entries), ties at the cut only partly taken, a level below topk; quads the sort zeroes",
         RAGGED, 15, 1000, _edit_ragged, twc=_twc, seed=101 + _twc,
         count={(0, 0): ">", (1, 0): ">", (0, 1): ">", (1, 1): ">", (0, 2): "<", (1, 2): "<"}, cut_tie=_EVERY, zero_quad=True)

_add("chunk-exact", "a level of exactly kChunk elements, a power of two (ibits 12 at its boundary); topk a power of two (no padding)",
     [(16, 16, 8, 1.0)], 16, 1024, seed=103, count={(0, 0): ">", (1, 0): ">"}, cut_tie=[(0, 0), (1, 0)])


def _edit_chunk_plus_one(case, lv, rng):
    lv[0]["lg"][0, -1, -1, 0] = 8       # the one element of the second chunk is image 0's best candidate
    lv[0]["ct"][0, -1, -1, 0] = 8


_add("chunk-plus-one", "a level of kChunk + 1 elements: the second chunk holds one element, which must be selected; C = 1",
     [(17, 241, 8, 1.0)], 1, 100, _edit_chunk_plus_one, seed=104, count={(0, 0): ">", (1, 0): ">"},
     taken=[(0, 0, K_CHUNK)])


def _edit_topk_one(case, lv, rng):
    lg, ct = lv[0]["lg"], lv[0]["ct"]
    np.minimum(lg[0], 7, out=lg[0])     # image 0: the best score (8, 8) at exactly two elements, the lower flat index wins
    ct[0].reshape(-1)[[10, 20]] = 8
    lg[0].reshape(-1, case.C)[10, 3] = 8
    lg[0].reshape(-1, case.C)[20, 1] = 8


_add("topk-one", "topk 1 (kp 2); image 0 has its best score twice", [(5, 7, 16, 0.5)], 15, 1, _edit_topk_one, seed=105,
     count={(0, 0): ">", (1, 0): ">"}, cut_tie=[(0, 0)], taken=[(0, 0, 10 * 15 + 3)])

_add("topk-max", "topk 4096 = kMaxTopk: kp fills the whole sort array; corner sort off",
     [(40, 56, 8, 0.5)], 15, 4096, sortc=False, seed=106, count={(0, 0): ">", (1, 0): ">"}, cut_tie=[(0, 0), (1, 0)])

_add("one-index-step", "levels of at most 2048 elements (2048 and 560) with more candidates than topk: the index select takes a "
     "single radix step", [(8, 16, 8, 1.0), (5, 7, 16, 0.5)], 16, 50, seed=107,
     count={k: ">" for k in _EVERY}, cut_tie=_EVERY)


def _edit_placed(extra):
    def edit(case, lv, rng):
        """Nothing is a candidate (logit -8), then topk + extra elements per image and level are set to logits in [1, 8], every
        chunk of the level among them.  extra 1: three of the placed elements get logit 0 on pixels of centerness 0, the lowest
        score there is, so the cut falls among those three."""
        for a in lv:
            n, c = a["lg"].shape[0], a["lg"].shape[-1]
            a["lg"][:] = -8
            a["ct"][:] = _grid(rng, a["ct"].shape, 0, 8)
            n_elem = a["lg"][0].size
            for im in range(n):
                first = np.arange(0, n_elem, K_CHUNK) + rng.integers(0, min(K_CHUNK, n_elem - (n_elem - 1) // K_CHUNK * K_CHUNK))
                rest = np.setdiff1d(rng.permutation(n_elem), first, assume_unique=True)
                idx = np.concatenate((first, rest[:case.topk + extra - first.size]))
                a["lg"][im].reshape(-1)[idx] = _grid(rng, idx.shape, 1, 8)
                if extra:
                    low = idx[-3:]
                    a["lg"][im].reshape(-1)[low] = 0
                    a["ct"][im].reshape(-1)[low // c] = 0
    return edit


_PLACED = [(40, 56, 8, 1.0), (5, 7, 64, 0.5)]
_add("exactly-topk", "a candidate count equal to topk on every level: decode_pick's total <= topk branch at its boundary",
     _PLACED, 15, 300, _edit_placed(0), twc=False, seed=108, count={k: "==" for k in _EVERY})
_add("topk-plus-one", "a candidate count of topk + 1: exactly one candidate is cut, the highest flat index of the lowest score",
     _PLACED, 15, 300, _edit_placed(1), twc=True, seed=109, count={k: "+1" for k in _EVERY}, cut_tie=_EVERY)


def _edit_all_tied(case, lv, rng):
    lv[0]["lg"][:] = 2
    lv[0]["ct"][:] = 1


_add("all-tied", "every element tied at one score: the select is made by index alone, over two index radix steps",
     [(40, 56, 8, 1.0)], 15, 1000, _edit_all_tied, seed=110, count={(0, 0): ">", (1, 0): ">"}, cut_tie=[(0, 0), (1, 0)],
     lowest=[(0, 0), (1, 0)])
_add("all-tied-4096", "every element tied, over a level of exactly 4096 elements", [(16, 16, 8, 0.5)], 16, 1000, _edit_all_tied,
     seed=111, count={(0, 0): ">", (1, 0): ">"}, cut_tie=[(0, 0), (1, 0)], lowest=[(0, 0), (1, 0)])


def _edit_saturated(case, lv, rng):
    lg, ct = lv[0]["lg"], lv[0]["ct"]
    for im, npix in ((0, 10), (1, 5)):            # 150 elements > topk in image 0, 75 < topk in image 1
        px = rng.permutation(lg[im].shape[0] * lg[im].shape[1])[:npix]
        lg[im].reshape(-1, case.C)[px] = 30
        ct[im].reshape(-1)[px] = 30


_add("saturated", "scores of exactly 1.0 (logit 30, centerness 30) in the top histogram bin: more of them than topk in image 0 "
     "(the cut is made inside the top bin by index), fewer in image 1", [(20, 28, 8, 1.0)], 15, 100, _edit_saturated, seed=112,
     count={(0, 0): ">", (1, 0): ">"}, cut_tie=[(0, 0), (1, 0)])


def _edit_at_threshold(case, lv, rng):
    for a in lv:
        a["ct"][:, ::3] = 0
        a["lg"][:, ::3, ::2, :5] = 0              # sigmoid 0.5, and with centerness 0 a score of sqrt(0.25) = 0.5 exactly


_AT = [(20, 28, 8, 1.0), (5, 7, 32, 0.5)]
for _name, _twc, _flags in (("at-threshold-twc", True, 0), ("at-threshold-notwc", False, 0), ("at-threshold-noctr", False, NO_CTRNESS)):
    _add(_name, "thresh 0.5 with elements whose thresholded value is exactly 0.5: the test is a strict >", _AT, 15, 200,
         _edit_at_threshold, thresh=0.5, twc=_twc, flags=_flags, seed=113, count={(0, 0): ">", (1, 0): ">"}, at_thresh=_EVERY)

for _name, _thr in (("thresh-zero-twc", 0.0), ("thresh-negative-twc", -1.0)):
    _add(_name, "pre_nms_thresh <= 0 with thresh_with_ctr: setup's key_lo = 0 branch; every element is a candidate", _AT, 15, 300,
         thresh=_thr, twc=True, seed=114, count={k: ">" for k in _EVERY}, cut_tie=_EVERY)


def _edit_empty_first(case, lv, rng):
    lv[0]["lg"][:] = -8
    for a in lv:
        a["lg"][1] = -8


_add("empty-level-first", "level 0 without a candidate before a full and a partly filled level (the off sum of decode_finalize); "
     "image 1 without any candidate (count 0)", [(5, 7, 8, 1.0), (20, 28, 16, 0.5), (3, 4, 32, 1.0)], 15, 150, _edit_empty_first,
     seed=115, count={(0, 0): "0", (0, 1): ">", (0, 2): "<", (1, 0): "0", (1, 1): "0", (1, 2): "0"})

_add("eight-levels", "kMaxLevels levels, some above and some below topk",
     [(3, 4, 8, 1.0), (3, 3, 16, 0.5), (2, 4, 32, 1.0), (2, 3, 64, 0.5), (2, 2, 128, 1.0), (1, 3, 256, 0.5), (1, 2, 512, 1.0),
      (1, 1, 1024, 0.5)], 15, 12, twc=False, seed=116, count={(0, 0): ">", (1, 0): ">", (0, 7): "<", (1, 7): "<"})

_add("one-class", "C = 1 on two levels", [(20, 28, 8, 1.0), (5, 7, 16, 0.5)], 1, 50, seed=117,
     count={(0, 0): ">", (1, 0): ">", (0, 1): "<", (1, 1): "<"}, cut_tie=[(0, 0), (1, 0)])

_add("fused9", "cut-ragged-twc in the engine's layout (modeling/dafne/dafne.py head_levels): delta | centerness in one [N,H,W,9] "
     "buffer (delta_ps 9, centerness a flat view from offset 8 with ctrness_ps 9), logits_ps 20 with +30 in the padding channels",
     RAGGED, 15, 1000, twc=True, layout="fused9", same_as="cut-ragged-twc")
_add("fused9-no-center", "the fused layout of a head without center regression (NO_CENTER): delta is the whole regression",
     [(20, 28, 16, 0.5), (5, 7, 64, 1.0)], 15, 400, twc=True, flags=NO_CENTER, layout="fused9", seed=118,
     count={(0, 0): ">", (1, 0): ">", (0, 1): "<", (1, 1): "<"}, cut_tie=[(0, 0), (1, 0)])

NAMES = list(CASES)
