#!/usr/bin/env python3
"""Record the reference implementation's NIQE answers for the NIQE tests: tests/golden/niqe_cases.npz, and a copy of its pristine model next to it.

    python tools/make_niqe_golden.py --upstream /path/to/the/upstream/checkout

It runs only where the upstream tree is (BasicSR's ``basicsr/metrics/niqe.py`` and ``niqe_pris_params.npz``); no test and nothing on a GPU machine
needs that tree, they read the two files written here.  Upstream's module is loaded BY PATH and none of its text is kept.

Two of its imports are replaced:
  * ``cv2``.  ``niqe()`` calls ``cv2.resize(img, (w // 2, h // 2), interpolation=cv2.INTER_LINEAR)`` once, to halve the picture for the second
    scale.  The module below stands in for it: its ``resize`` is the mean of every 2 x 2 block and it ASSERTS that the size asked for is exactly half.
    That is what bilinear interpolation computes there: OpenCV samples output pixel i at input position 2 i + 0.5 (pixel centres aligned, scale
    exactly 2), halfway between the input pixels 2 i and 2 i + 1 in both directions, so the four weights are 1/4 each and there is no border case --
    ``niqe()`` crops to a multiple of 96 first, so both sides are even.  Differences are those of float rounding.  INTER_LINEAR without anti-aliasing
    is the reference's own simplification (its comment says so); the device kernel follows the reference, not the MATLAB original.
  * ``basicsr.metrics.metric_util``.  ``niqe()`` itself uses nothing of it (``calculate_niqe`` does, to convert colour); a stub with the two names
    lets the module import.

What is recorded (float64):
  score/<case>      : ``niqe()`` on every frame of every case of ``niqe_cases.CASES``, fed with the luma on the 16 .. 235 scale in float64 (the whole
                      pictures of one code, ``niqe_cases.FLAT_CASES``, are not recorded: upstream fits the residue its own sums leave there, and
                      the answer says nothing -- DESIGN.md 3.33);
  feature/<block>   : ``compute_feature()`` on every block of ``niqe_cases.feature_blocks()`` (float32 blocks).
"""
import argparse
import importlib.util
import os
import shutil
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _cv2_stand_in() -> types.ModuleType:
    m = types.ModuleType("cv2")
    m.INTER_LINEAR = 1

    def resize(img, dsize, interpolation=None):
        h, w = img.shape
        assert interpolation == m.INTER_LINEAR and h % 2 == 0 and w % 2 == 0 and tuple(dsize) == (w // 2, h // 2), (img.shape, dsize, interpolation)
        return 0.25 * ((img[0::2, 0::2] + img[0::2, 1::2]) + (img[1::2, 0::2] + img[1::2, 1::2]))
    m.resize = resize
    return m


def load_upstream(path: str) -> types.ModuleType:
    """Upstream's niqe.py as a module, with the two stand-ins in place while it imports; sys.modules is put back afterwards."""
    util = types.ModuleType("basicsr.metrics.metric_util")
    util.reorder_image = util.to_y_channel = None
    pkg = types.ModuleType("basicsr.metrics")
    pkg.metric_util = util
    fake = {"cv2": _cv2_stand_in(), "basicsr.metrics": pkg, "basicsr.metrics.metric_util": util}
    if "basicsr" not in sys.modules:
        fake["basicsr"] = types.ModuleType("basicsr")
    saved = {k: sys.modules.get(k) for k in fake}
    sys.modules.update(fake)
    try:
        spec = importlib.util.spec_from_file_location("upstream_niqe", path)
        mod = importlib.util.module_from_spec(spec)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)      # scipy.ndimage.filters
            spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--upstream", required=True, help="the upstream checkout (the directory that holds basicsr/metrics/niqe.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    import niqe_cases as K
    metrics = os.path.join(a.upstream, "basicsr", "metrics")
    up = load_upstream(os.path.join(metrics, "niqe.py"))
    with np.load(os.path.join(metrics, "niqe_pris_params.npz")) as z:
        mu, cov, win = z["mu_pris_param"], z["cov_pris_param"], z["gaussian_window"]
    rec = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # the mean of an empty slice: the NaN the cases are there for
        for c in K.CASES:
            rec["score/" + c.name] = np.array([up.niqe(K.values(K.picture(c, Y), c.fmt), mu, cov, win) for Y in K.frames(c)], np.float64).reshape(-1)
            print(c.name, rec["score/" + c.name])
        for name, b in K.feature_blocks():
            rec["feature/" + name] = np.array(up.compute_feature(b), np.float64)
    os.makedirs(a.out, exist_ok=True)
    np.savez(os.path.join(a.out, "niqe_cases.npz"), **rec)
    shutil.copyfile(os.path.join(metrics, "niqe_pris_params.npz"), os.path.join(a.out, "niqe_pris_params.npz"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
