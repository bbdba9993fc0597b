#!/usr/bin/env python3
"""tests/golden/scene_split.npz: the tile origins of the reference's own DOTA split, SplitOnlyImage_multi_process.splitbase
.SplitSingle at rate 1 (tools/prepare_dota), for a list of (h, w, patch, overlap) cases.  cv2 is stubbed: imread returns a
zero image of the case's shape, imwrite records the tile file names <scene>__1__<left>___<up>.png in call order.

    python tests/golden/make_golden_scene.py        (build container only: imports the reference's split module)
"""
import os
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

# (h, w, patch, overlap): smaller than, equal to, patch + slide (1848 at 1024 / 200) and +- 1, a large scene, a one-row
# strip, another patch / overlap and ImgSplit's default gap of 100
CASES = [(500, 700, 1024, 200), (1024, 1024, 1024, 200), (1024, 300, 1024, 200), (1848, 1848, 1024, 200), (1847, 1849, 1024, 200),
         (1849, 1847, 1024, 200), (700, 900, 1024, 200), (1848, 1100, 1024, 200), (4000, 3000, 1024, 200), (3000, 4000, 1024, 200),
         (1, 5000, 1024, 200), (5000, 1, 1024, 200), (1333, 2011, 600, 150), (600, 601, 600, 150), (2048, 2049, 1024, 100),
         (1025, 924, 1024, 100), (4000, 4000, 1024, 200)]


def main():
    assert os.path.isdir(REF), "reference tree not present: fixtures can only be made in the build container"
    state = {"shape": None, "names": []}
    cv2 = types.ModuleType("cv2")
    cv2.imread = lambda path, *a: np.zeros(state["shape"], dtype=np.uint8)
    cv2.imwrite = lambda path, img: state["names"].append(os.path.basename(path)) or True
    cv2.INTER_CUBIC = 2
    sys.modules["cv2"] = cv2
    sys.modules["dota_utils"] = types.ModuleType("dota_utils")     # (file listing only; needs shapely, unused by SplitSingle)
    sys.path.insert(0, os.path.join(REF, "tools", "prepare_dota"))
    import SplitOnlyImage_multi_process as sp
    out = {"cases": np.array(CASES, dtype=np.int64)}
    for i, (h, w, patch, overlap) in enumerate(CASES):
        s = sp.splitbase.__new__(sp.splitbase)         # (no worker pool: SplitSingle runs in this process)
        s.srcpath, s.dstpath, s.outpath = "src", "dst", "dst"
        s.gap, s.subsize, s.slide, s.ext, s.padding = overlap, patch, patch - overlap, ".png", True
        state["shape"], state["names"] = (h, w, 3), []
        s.SplitSingle("P%04d" % i, 1, ".png")
        origins = []
        for n in state["names"]:
            m = re.fullmatch(r"P%04d__1__(\d+)___(\d+)\.png" % i, n)
            assert m, n
            origins.append((int(m.group(1)), int(m.group(2))))
        out["origins_%d" % i] = np.array(origins, dtype=np.int64).reshape(-1, 2)
    np.savez_compressed(os.path.join(HERE, "scene_split.npz"), **out)
    print("wrote scene_split.npz,", len(CASES), "cases")


if __name__ == "__main__":
    main()
