#!/usr/bin/env python3
"""Record the reference implementation's SSIM and PSNR answers for the full-reference tests: tests/golden/ssim_cases.npz.

    python tools/make_ssim_golden.py --upstream /path/to/the/upstream/checkout

It runs only where the upstream tree is (``basicsr/metrics/psnr_ssim.py``); no test and nothing on a GPU machine needs that tree, they read the file
written here.  Upstream's module is loaded BY PATH and none of its text is kept.

Three of its imports are replaced, because neither ``cv2`` nor ``skimage`` need be installed:
  * ``cv2``.  ``_ssim_cly`` calls ``getGaussianKernel(11, 1.5)`` and ``filter2D(img, -1, window, borderType=BORDER_REPLICATE)``.  The module below stands in:
    its kernel is OpenCV's formula for a given sigma, ``exp(-(i - (n - 1) / 2)^2 / (2 sigma^2))`` normalised to sum 1, as an n x 1 float64 column; its
    ``filter2D`` is the plain float64 correlation of the picture, padded by replicating its border, with the window, anchored at the window's centre --
    what OpenCV computes for a float64 picture up to the order of its sums -- and it ASSERTS that the depth is -1 and the border the replicated one.
  * ``skimage.metrics``: imported by the module, used by nothing that runs here; an empty stub.
  * ``basicsr.metrics.metric_util``: ``reorder_image`` gives a 2-d picture a channel axis, as upstream's does for 'HWC'; ``to_y_channel`` is not reached
    (``test_y_channel`` stays False: the planes fed ARE the stream's luma and chroma).

What is recorded (float64), per case of tests/ssim_cases.py:
  ssim/<case>   : [T] ``_ssim_cly`` of the two luma planes of every frame pair, fed on the reference's 0 .. 255 scale (the codes at 8 bit, codes * 255 /
                  1023 at 10 bit);
  psnr/<case>   : [T, 3] ``calculate_psnr(crop_border=0)`` of the Y, U and V planes on the same scale (``inf`` where they are equal).
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "shift-net_amd"))


def _cv2_stand_in() -> types.ModuleType:
    m = types.ModuleType("cv2")
    m.BORDER_REPLICATE = 1

    def getGaussianKernel(ksize, sigma):
        assert ksize % 2 == 1 and sigma > 0
        i = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
        g = np.exp(-(i * i) / (2.0 * sigma * sigma))
        return (g / g.sum()).reshape(ksize, 1)

    def filter2D(src, ddepth, kernel, borderType=None):
        assert ddepth == -1 and borderType == m.BORDER_REPLICATE and src.ndim == 2 and src.dtype == np.float64, (ddepth, borderType, src.shape, src.dtype)
        kh, kw = kernel.shape
        assert kh % 2 == 1 and kw % 2 == 1
        h, w = src.shape
        pad = np.pad(src, ((kh // 2, kh // 2), (kw // 2, kw // 2)), mode="edge")
        out = np.zeros((h, w), np.float64)
        for i in range(kh):
            for j in range(kw):
                out += kernel[i, j] * pad[i:i + h, j:j + w]
        return out
    m.getGaussianKernel, m.filter2D = getGaussianKernel, filter2D
    return m


def load_upstream(path: str) -> types.ModuleType:
    """Upstream's psnr_ssim.py as a module, with the stand-ins in place while it imports; sys.modules is put back afterwards."""
    util = types.ModuleType("basicsr.metrics.metric_util")
    util.reorder_image = lambda img, input_order="HWC": img[..., None] if img.ndim == 2 else img
    util.to_y_channel = None
    pkg = types.ModuleType("basicsr.metrics")
    pkg.metric_util = util
    sk, skm = types.ModuleType("skimage"), types.ModuleType("skimage.metrics")
    sk.metrics = skm
    fake = {"cv2": _cv2_stand_in(), "basicsr.metrics": pkg, "basicsr.metrics.metric_util": util, "skimage": sk, "skimage.metrics": skm}
    if "basicsr" not in sys.modules:
        fake["basicsr"] = types.ModuleType("basicsr")
    saved = {k: sys.modules.get(k) for k in fake}
    sys.modules.update(fake)
    try:
        spec = importlib.util.spec_from_file_location("upstream_psnr_ssim", path)
        mod = importlib.util.module_from_spec(spec)
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
    ap.add_argument("--upstream", required=True, help="the upstream checkout (the directory that holds basicsr/metrics/psnr_ssim.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    import ssim_cases as K
    up = load_upstream(os.path.join(a.upstream, "basicsr", "metrics", "psnr_ssim.py"))
    rec = {}
    for c in K.CASES:
        ssim, psnr = [], []
        for pa, pb in K.pictures(c):
            fa, fb = ([K.upstream_scale(p, c.fmt) for p in planes] for planes in (pa, pb))
            ssim.append(up._ssim_cly(fa[0], fb[0]))
            psnr.append([up.calculate_psnr(x, y, crop_border=0) for x, y in zip(fa, fb)])
        rec["ssim/" + c.name], rec["psnr/" + c.name] = np.array(ssim, np.float64), np.array(psnr, np.float64)
        print(c.name, rec["ssim/" + c.name], rec["psnr/" + c.name].reshape(-1))
    os.makedirs(a.out, exist_ok=True)
    np.savez(os.path.join(a.out, "ssim_cases.npz"), **rec)
    return 0


if __name__ == "__main__":
    sys.exit(main())
