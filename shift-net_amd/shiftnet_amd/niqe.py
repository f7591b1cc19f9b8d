"""NIQE, the no-reference quality score of Mittal, Soundararajan and Bovik ("Making a 'Completely Blind' Image Quality Analyzer", IEEE SPL 2013):
the part that is not per pixel, on the host in float64.

NIQE cuts a picture into 96 x 96 blocks at two scales.  Per block and scale it looks at five maps: the locally normalised luma n (mean and
deviation under a 7 x 7 Gaussian window) and the products of n with its left, upper, upper-left and upper-right neighbour.  To each map it fits an
asymmetric generalised Gaussian (AGGD): a shape alpha and a scale to the left and to the right of zero, beta_l and beta_r.  That gives 2 features for
n (alpha and the mean of the two scales) and 4 for each product (alpha, the distribution's mean, beta_l, beta_r): 18 per scale, 36 per block.  The
score is the Mahalanobis-like distance between the mean and covariance of the picture's 36-vectors and those of a corpus of pristine natural pictures
(the "pristine model": mu, cov and the window, in a small .npz file).  Smaller reads as "more like a natural picture"; it is no verdict.

The moment-matching fit of an AGGD needs five sums of a map with N values m:
    N-, S- : the count and the sum of m^2 over m < 0        N+, S+ : the same over m > 0        A : the sum of |m|
    sigma_l = sqrt(S- / N-)    sigma_r = sqrt(S+ / N+)    g = sigma_l / sigma_r
    r = (A / N)^2 / ((S- + S+) / N)                R = r (g^3 + 1) (g + 1) / (g^2 + 1)^2
    alpha = the grid point a at which rho(a) = Gamma(2/a)^2 / (Gamma(1/a) Gamma(3/a)) is nearest to R
    beta_l = sigma_l sqrt(Gamma(1/alpha) / Gamma(3/alpha)), beta_r likewise; mean = (beta_r - beta_l) Gamma(2/alpha) / Gamma(1/alpha)
``sn_yuv_niqe_sums`` (csrc/sn_niqe.hip, include/shiftnet_hip.h) makes those sums on the device, ``block_features`` the 18 numbers from a block's 5 x 5
sums, ``score`` the distance.  The reference implementation this is checked against (tests/golden/niqe_cases.npz, made by tools/make_niqe_golden.py) is
BasicSR's; its grid for alpha, 0.2 to 10 in steps of 0.001, and its rule for blocks it cannot fit (NaN, dropped from the covariance) are kept.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
from scipy.special import gamma

BLOCK = 96            # SN_NIQE_BLOCK
MAPS, SUMS = 5, 5     # SN_NIQE_MAPS, SN_NIQE_SUMS
FEATURES = 18         # per block and scale

_table: Optional[Tuple[np.ndarray, np.ndarray]] = None


def default_params_path() -> str:
    """tests/golden/niqe_pris_params.npz of the checkout: the one place the pristine model's file lives in this repository."""
    import basicsr._paths as P
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(P.__file__))), "tests", "golden", "niqe_pris_params.npz")


def load_params(path: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The pristine model -> (mu[36], cov[36, 36], win7[7]), float64.  win7 holds the row sums of the 7 x 7 window, its separable factor: the window
    adds up to 1, so outer(win7, win7) is the window if it is separable at all.  Raises ValueError if it is not, to 1e-12."""
    with np.load(path) as z:
        mu = np.asarray(z["mu_pris_param"], dtype=np.float64).reshape(-1)
        cov = np.asarray(z["cov_pris_param"], dtype=np.float64)
        win = np.asarray(z["gaussian_window"], dtype=np.float64)
    if mu.shape != (2 * FEATURES,) or cov.shape != (2 * FEATURES, 2 * FEATURES) or win.shape != (7, 7):
        raise ValueError(f"{path}: not a NIQE model of {2 * FEATURES} features and a 7 x 7 window: {mu.shape}, {cov.shape}, {win.shape}")
    win7 = win.sum(axis=1)
    if not np.abs(np.outer(win7, win7) - win).max() <= 1e-12:
        raise ValueError(f"{path}: the 7 x 7 window is not the outer product of its row sums (the kernel filters rows, then columns)")
    return mu, cov, win7


def gamma_table() -> Tuple[np.ndarray, np.ndarray]:
    """(a, rho(a)) on the grid 0.2, 0.201, ..., 10.0 (9801 points); rho is strictly increasing."""
    global _table
    if _table is None:
        a = np.arange(0.2, 10.001, 0.001)
        inv = np.reciprocal(a)
        _table = (a, np.square(gamma(inv * 2)) / (gamma(inv) * gamma(inv * 3)))
    return _table


def nearest_shape(R):
    """The index of the grid point whose rho is nearest to R (a number or an array): what an argmin over (rho - R)^2 of the whole table finds (the
    first of equals; 0 for NaN, where every square is NaN), by bisection on the increasing table and one comparison of the same two squares."""
    _, rho = gamma_table()
    R = np.asarray(R, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        hi = np.clip(np.searchsorted(rho, R), 1, len(rho) - 1)      # beyond either end the nearer of the two end points is the end point
        idx = np.where((rho[hi - 1] - R) ** 2 <= (rho[hi] - R) ** 2, hi - 1, hi)
    idx = np.where(np.isnan(R), 0, idx)
    return int(idx) if idx.ndim == 0 else idx


def _aggd(s: np.ndarray, N: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The five sums of maps, [..., 5] -> (alpha, beta_l, beta_r), [...] each.  The deviation of an empty side is NaN (the mean of no values) and so is
    that side's beta; R is NaN then, and alpha is the FIRST grid point, 0.2: what the reference's argmin over an all-NaN array returns.  The block's
    row of features then holds NaN and ``score`` drops it from the covariance, but its finite entries still count in the mean -- kept as the
    reference has it."""
    n_neg, s_neg, n_pos, s_pos, s_abs = np.moveaxis(s, -1, 0)
    with np.errstate(all="ignore"):
        sl, sr = np.sqrt(s_neg / n_neg), np.sqrt(s_pos / n_pos)
        g = sl / sr
        r = (s_abs / N) ** 2 / ((s_neg + s_pos) / N)
        R = (r * (g ** 3 + 1) * (g + 1)) / ((g ** 2 + 1) ** 2)
        alpha = gamma_table()[0][nearest_shape(R)]
        k = np.sqrt(gamma(1 / alpha) / gamma(3 / alpha))
        return alpha, sl * k, sr * k


def block_features(sums: np.ndarray, B: int) -> np.ndarray:
    """sums: [..., 5, 5], the five sums of the five maps of blocks of side ``B`` (96 at scale 1, 48 at scale 2) -> their 18 features, [..., 18] float64;
    NaN where a side of a map is empty (``_aggd``).  All blocks are fitted at once: a 720p frame has 91 of them at each scale."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.shape[-2:] != (MAPS, SUMS):
        raise ValueError(f"a block has {MAPS} x {SUMS} sums, got {sums.shape}")
    alpha, bl, br = _aggd(sums, B * B)                              # [..., 5] each
    with np.errstate(all="ignore"):
        mean = (br - bl) * (gamma(2 / alpha) / gamma(1 / alpha))
    feat = [alpha[..., 0], (bl[..., 0] + br[..., 0]) / 2]
    for k in range(1, MAPS):
        feat += [alpha[..., k], mean[..., k], bl[..., k], br[..., k]]
    return np.stack(feat, axis=-1)


def frame_features(sums: np.ndarray) -> np.ndarray:
    """sums: [2, nbh, nbw, 5, 5], one frame of ``niqe_sums_yuv`` -> [nbh * nbw, 36]: per block the 18 features of scale 1, then those of scale 2.
    The blocks come column by column, the order the reference implementation adds them in."""
    sums = np.asarray(sums, dtype=np.float64)
    feat = np.concatenate([block_features(sums[s], BLOCK >> s) for s in range(2)], axis=-1)      # [nbh, nbw, 36]
    return np.ascontiguousarray(feat.transpose(1, 0, 2)).reshape(-1, 2 * FEATURES)


def score(feat: np.ndarray, mu: np.ndarray, cov: np.ndarray) -> float:
    """feat: [nblocks, 36] -> the distance sqrt(d^T pinv((cov + cov_feat) / 2) d), d = mu - nanmean(feat): the mean ignores NaN entries, the covariance
    is that of the rows without any NaN.  nan when fewer than two rows are NaN-free: there is no covariance then."""
    feat = np.asarray(feat, dtype=np.float64).reshape(-1, 2 * FEATURES)
    clean = feat[~np.isnan(feat).any(axis=1)]
    if clean.shape[0] < 2:
        return float("nan")
    d = mu - np.nanmean(feat, axis=0)
    inv = np.linalg.pinv((cov + np.cov(clean, rowvar=False)) / 2)
    return float(np.sqrt(d @ inv @ d))


def frame_score(sums: np.ndarray, mu: np.ndarray, cov: np.ndarray) -> float:
    """One frame of ``niqe_sums_yuv`` -> its score."""
    return score(frame_features(sums), mu, cov)
