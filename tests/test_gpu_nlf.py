"""-m gpu: the noise-level function.  ``sn_yuv_noise_hist_bands`` and ``sn_noise_map_level`` against the numpy restatements of tests/nlf_ref.py bit for
bit, the band histograms against ``sn_yuv_noise_hist``, and the video restorer with ``noise_model=`` against windows composed by hand from the
restatements, against itself with the pipeline off, with the curves fed back as a list, on the cropped stream, and through the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nlf_ref as F
import noise_ref as N
import picture_ref as P
import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import noise, restore, y4m
from shiftnet_amd.io_edges import egress_yuv, ingest_yuv, noise_hist_bands_yuv, noise_hist_yuv, noise_map_level, yuv_fmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F420_8 = R.Fmt(8, R.C420_CENTER, R.BT709, R.LIMITED)
F444_8 = R.Fmt(8, R.C444, R.BT601, R.FULL)
F444_10 = R.Fmt(10, R.C444, R.BT709, R.LIMITED)
F420_10 = R.Fmt(10, R.C420_LEFT, R.BT709, R.LIMITED)
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def pack(codes: np.ndarray, fmt: R.Fmt) -> np.ndarray:
    """int [T, samples] -> uint8 [T, frame_bytes]."""
    return codes.astype(np.uint8) if fmt.bits == 8 else codes.astype("<u2").view(np.uint8).reshape(len(codes), -1)


def payloads(fmt: R.Fmt, T: int, H: int, W: int, seed: int, kind: str = "ramp") -> np.ndarray:
    """ramp: a diagonal luma ramp over the whole code range plus noise whose level differs from frame to frame (many bands, many bins, clipped codes);
    random: every code equally likely (v reaches 2 (2^bits - 1): the saturating bin fills); edges: only the codes lo, lo + 1, hi - 1 and hi of the
    limited range (blocks with a code equal to lo or hi do not count, the others do)."""
    rng = np.random.default_rng(seed)
    top = (1 << fmt.bits) - 1
    n = R.frame_bytes(fmt, H, W) // (1 if fmt.bits == 8 else 2)
    p = rng.integers(0, top + 1, (T, n))
    y, x = np.mgrid[0:H, 0:W]
    for t in range(T):
        if kind == "ramp":
            s = (2.0, 9.0, 30.0)[t % 3] * (top / 255.0)
            Y = np.clip(np.rint(top * (x + y) / max(H + W - 2, 1) + rng.normal(0.0, 1.0, (H, W)) * s), 0, top)
        elif kind == "edges":
            sc = 1 << (fmt.bits - 8)
            Y = np.array([16 * sc, 16 * sc + 1, 235 * sc - 1, 235 * sc])[rng.integers(0, 4, (H, W))]
            Y[0:2, 0:2] = [[16 * sc + 1, 235 * sc - 1], [235 * sc - 1, 16 * sc + 1]]            # three blocks that count for certain: a mixed one,
            Y[0:2, 2:4], Y[0:2, 4:6] = 16 * sc + 1, 235 * sc - 1                                  # one in the first band and one in the last
        else:
            Y = p[t, :H * W].reshape(H, W)
        p[t, :H * W] = Y.reshape(-1)
    return pack(p, fmt)


# (format, H, W, T, rect, kind, lo / hi or None for the format's own)
HIST_CASES = {
    "8-bit 420 38x52 T3": (F420_8, 38, 52, 3, None, "ramp", None),                         # odd block counts, a right edge of one block, unaligned rows
    "10-bit 444 34x70": (F444_10, 34, 70, 2, None, "ramp", None),
    "444 rect odd origin": (F444_8, 40, 48, 2, (5, 3, 30, 25), "ramp", None),
    "420 rect to the far edge, odd w": (F420_8, 37, 71, 2, (8, 4, 63, 33), "ramp", None),
    "codes equal to lo and hi": (F420_8, 20, 36, 2, None, "edges", None),
    "codes equal to lo and hi, 10 bit": (F420_10, 20, 36, 1, None, "edges", None),
    "v >= NBV": (F444_8, 34, 66, 2, None, "random", None),
    "v >= NBV, 10 bit": (F420_10, 34, 66, 1, None, "random", (-1, 1024)),
    "smaller than one block": (F420_8, 1, 9, 2, None, "random", None),
    "two workgroups per frame": (F420_8, 200, 340, 2, None, "ramp", None),                   # 100 block rows x 43 units = 4300 > the 4096 of a workgroup
    "two workgroups per frame, 10 bit": (F420_10, 200, 340, 2, None, "ramp", None),         # the same for the 10-bit instance, with its 8 copies
}


@pytest.mark.parametrize("case", list(HIST_CASES), ids=list(HIST_CASES))
def test_noise_hist_bands_equals_the_restatement_exactly_overwrites_and_sums_to_the_flat_histogram(case):
    fmt, H, W, T, rect, kind, lohi = HIST_CASES[case]
    f = yuv_fmt(*fmt)
    nb = F.nbv(fmt.bits)
    assert nb == noise.nlf_bins(fmt.bits)
    lo, hi = lohi or N.clip_codes(fmt)
    p = payloads(fmt, T, H, W, seed=H * 1000 + W + T, kind=kind)
    want = F.hist_bands_ref(p, fmt, H, W, lo, hi, rect)
    h, w = (H, W) if rect is None else (rect[3], rect[2])
    assert want.shape == (T, 16, nb) and int(want.sum(dtype=np.int64)) <= T * (h // 2) * (w // 2)
    if kind == "ramp":
        assert (want.sum(axis=(0, 2)) > 0).sum() >= 8 and (want.sum(axis=(0, 1)) > 0).sum() > 16             # many bands, many bins
    if kind == "random":
        assert (want.sum() == 0) if h < 2 else (want[:, :, nb - 1].sum() > 0)                                 # the saturating bin fills
    if kind == "edges":
        assert 0 < want.sum() < T * (h // 2) * (w // 2) and (want.sum(axis=(0, 2)) > 0).sum() >= 3               # some blocks are excluded, both end bands fill
        assert want[:, 0].sum() > 0 and want[:, 15].sum() > 0
    GUARD = 64
    dev = torch.from_numpy(p).cuda()
    g = torch.from_numpy(np.full(T * 16 * nb + 2 * GUARD, 0xA5A5A5A5, np.uint32)).cuda()      # dst starts as garbage: overwritten, not added to
    out = g[GUARD:GUARD + T * 16 * nb].view(T, 16, nb)
    for call in (1, 2):
        got = noise_hist_bands_yuv(dev, f, H, W, lo, hi, out=out, rect=rect)
        assert got is out
        b = g.cpu().numpy()
        assert np.array_equal(b[GUARD:-GUARD].reshape(T, 16, nb), want), (case, call)
        assert (b[:GUARD] == 0xA5A5A5A5).all() and (b[-GUARD:] == 0xA5A5A5A5).all()
    if lohi is None:
        alloc = noise_hist_bands_yuv(dev, f, H, W, rect=rect)                               # allocating form, the format's own lo / hi
        assert alloc.dtype == torch.uint32 and np.array_equal(alloc.cpu().numpy(), want)
    # against the existing kernel: the same blocks, only split by band and saturated
    flat = noise_hist_yuv(dev, f, H, W, lo, hi, rect=rect).cpu().numpy().astype(np.int64)
    bands = want.astype(np.int64).sum(axis=1)
    assert np.array_equal(bands[:, :nb - 1], flat[:, :nb - 1]) and np.array_equal(bands[:, nb - 1], flat[:, nb - 1:].sum(axis=1))


def test_noise_hist_bands_refuses_what_noise_hist_rect_refuses():
    lib = L.load()
    f = yuv_fmt(8, L.SN_YUV_420_CENTER, 0, 0)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(2 * 16 * 512 + 8, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    src, d = buf.data_ptr(), dst.data_ptr()
    call = lib.sn_yuv_noise_hist_bands
    assert call(src, f, None, d, 16, 235, 1, 8, 8, s) == 0
    assert call(src, f, L.YuvRect(2, 2, 4, 4), d, 16, 235, 1, 8, 8, s) == 0
    for bad in (L.YuvRect(1, 2, 4, 4), L.YuvRect(2, 2, 3, 4), L.YuvRect(2, 2, 8, 4), L.YuvRect(-2, 0, 4, 4), L.YuvRect(0, 0, 0, 4)):
        assert call(src, f, bad, d, 16, 235, 1, 8, 8, s) == -22                              # 4:2:0: odd origin, odd w inside, outside the frame, empty
    assert call(src, yuv_fmt(8, 0, 0, 0), L.YuvRect(1, 3, 3, 5), d, 16, 235, 1, 8, 8, s) == 0   # 4:4:4: any integers
    assert call(src, yuv_fmt(9, 0, 0, 0), None, d, 16, 235, 1, 8, 8, s) == -22
    assert call(src, yuv_fmt(8, 3, 0, 0), None, d, 16, 235, 1, 8, 8, s) == -22
    for T, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        assert call(src, f, None, d, 16, 235, T, H, W, s) == -22
    for k in (1, 2, 3):
        assert call(src, f, None, d + k, 16, 235, 1, 8, 8, s) == -22                         # dst is uint32
    assert call(src + 1, yuv_fmt(10, 0, 0, 0), None, d, 64, 940, 1, 8, 8, s) == -22           # 16-bit samples at an odd address
    assert call(src + 1, f, None, d, 16, 235, 1, 8, 8, s) == 0
    assert call(None, f, None, d, 16, 235, 1, 8, 8, s) == -22 and call(src, f, None, None, 16, 235, 1, 8, 8, s) == -22
    assert call(src, None, None, d, 16, 235, 1, 8, 8, s) == -22
    assert call(src, f, None, d, 236, 235, 1, 8, 8, s) == -22                                 # lo > hi
    assert call(src, f, None, d, 235, 235, 1, 8, 8, s) == 0                                   # lo == hi: legal, nothing counts
    assert call(src, f, None, d, 16, 235, 1, 1, 9, s) == 0
    torch.cuda.synchronize()
    assert int(dst.abs().sum()) == 0                                                          # every legal call above counted nothing (codes 0) ...
    assert call(src, f, None, d, -1, 235, 2, 8, 8, s) == 0
    torch.cuda.synchronize()
    h = dst.cpu().numpy()
    assert h[0] == 16 and h[16 * 128] == 16 and int(np.abs(h).sum()) == 32                     # ... with lo = -1: S - 4 lo = 4 -> band 0, bin 0, two frames


# ---- the map ----------------------------------------------------------------------------------------------------------------------------------
# (format, H, W, rect, Hp, Wp)
MAP_CASES = {
    "21x27 padded to 24x32": (F420_8, 21, 27, None, 24, 32),
    "8x8 exactly": (F444_8, 8, 8, None, 8, 8),
    "5x5": (F420_8, 5, 5, None, 8, 8),
    "rect inside 40x48": (F420_8, 40, 48, (6, 4, 26, 22), 24, 32),                          # 4:2:0: even origin and size; partial blocks on both far edges
    "rect inside 40x48, odd origin, 10 bit": (F444_10, 40, 48, (5, 3, 30, 25), 28, 32),
    "10 bit 21x27": (F420_10, 21, 27, None, 24, 28),
    "several tiles 70x300": (F420_8, 70, 300, None, 72, 304),                               # a tile is 128 x 32 pixels: 3 x 3 of them, partial blocks on both edges
    "a tile of padding only": (F444_8, 20, 20, None, 40, 136),
}
CURVE = [9.0, 8.5, 8.25, 7.0, 7.5, 6.0, 5.5, 5.75, 4.0, 3.5, 3.0, 2.0, 2.5, 1.0, 0.5, 0.0]      # not monotonic, ends at zero


def bits_of(t: torch.Tensor, name: str) -> np.ndarray:
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if name != "fp32" else t.numpy().view(np.uint32)


def want_bits(a: np.ndarray, name: str) -> np.ndarray:
    return a.view(np.uint16) if name != "fp32" else a.view(np.uint32)


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("case", list(MAP_CASES), ids=list(MAP_CASES))
def test_noise_map_level_equals_the_float32_restatement_bit_for_bit(case, name):
    fmt, H, W, rect, Hp, Wp = MAP_CASES[case]
    f, dt, T = yuv_fmt(*fmt), DTYPES[name], 2
    lo, hi = N.clip_codes(fmt)
    p = payloads(fmt, T, H, W, seed=H * 1000 + W, kind="ramp")
    dev = torch.from_numpy(p).cuda()
    k32 = F.knots32(CURVE)
    want = F.map_ref(p, fmt, H, W, Hp, Wp, k32, lo, hi, name, rect)
    if min(H, W) > 16:
        assert len(np.unique(want)) > 8                                                        # the plane does vary
    got = noise_map_level(dev, f, H, W, Hp, Wp, [c / 255.0 for c in CURVE], dt, rect=rect)
    assert got.shape == (1, T, 1, Hp, Wp) and got.dtype == dt
    assert np.array_equal(bits_of(got[0], name), want_bits(want, name)), (case, name)
    if rect is not None:                                                                       # ... which is the cropped stream's plane
        crop = P.crop_payloads(p, fmt, H, W, rect)
        assert torch.equal(got, noise_map_level(torch.from_numpy(crop).cuda(), f, rect[3], rect[2], Hp, Wp, [c / 255.0 for c in CURVE], dt))
    GUARD = 64                                                                                 # the filling form, at an address that is not 16 B aligned
    g = torch.full((T * Hp * Wp + 2 * GUARD + 1,), 7.0, dtype=dt, device="cuda")
    out = g[GUARD + 1:GUARD + 1 + T * Hp * Wp].view(1, T, 1, Hp, Wp)
    assert noise_map_level(dev, f, H, W, Hp, Wp, [c / 255.0 for c in CURVE], dt, lo, hi, out=out, rect=rect) is out and torch.equal(out, got)
    assert bool((g[:GUARD + 1] == 7.0).all()) and bool((g[GUARD + 1 + T * Hp * Wp:] == 7.0).all())
    for s in (0.0, 7.3, 50.0):                                                                 # a flat curve: float32(s / 255) in the dtype at every pixel
        flat = noise_map_level(dev, f, H, W, Hp, Wp, [s / 255.0] * 16, dt, rect=rect)
        one = R.to_dtype_bits(np.array([np.float32(s / 255.0)], np.float32), name)
        assert (bits_of(flat, name) == want_bits(one, name)[0]).all(), (case, name, s)
    lo2, hi2 = lo + 7, hi - 30                                                                 # another lo / hi: u is clamped at both ends
    assert np.array_equal(bits_of(noise_map_level(dev, f, H, W, Hp, Wp, [c / 255.0 for c in CURVE], dt, lo2, hi2, rect=rect)[0], name),
                          want_bits(F.map_ref(p, fmt, H, W, Hp, Wp, k32, lo2, hi2, name, rect), name))


def test_noise_map_level_refuses_bad_arguments():
    import ctypes as C
    lib = L.load()
    f = yuv_fmt(8, L.SN_YUV_420_CENTER, 0, 0)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(4096, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    src, d = buf.data_ptr(), dst.data_ptr()
    kn = (C.c_float * 16)(*([0.02] * 16))
    call = lib.sn_noise_map_level
    assert call(src, f, None, kn, 16, 235, d, 0, 1, 8, 8, 8, 8, s) == 0
    assert call(src, f, L.YuvRect(2, 2, 4, 4), kn, 16, 235, d, 0, 1, 8, 8, 4, 4, s) == 0
    assert call(src, f, L.YuvRect(1, 2, 4, 4), kn, 16, 235, d, 0, 1, 8, 8, 4, 4, s) == -22
    assert call(src, f, None, kn, 16, 235, d, 0, 1, 8, 8, 7, 8, s) == -22 and call(src, f, None, kn, 16, 235, d, 0, 1, 8, 8, 8, 7, s) == -22
    assert call(src, f, None, kn, 235, 235, d, 0, 1, 8, 8, 8, 8, s) == -22 and call(src, f, None, kn, 236, 235, d, 0, 1, 8, 8, 8, 8, s) == -22
    assert call(src, f, None, kn, 16, 235, d, 3, 1, 8, 8, 8, 8, s) == -22 and call(src, f, None, kn, 16, 235, d, -1, 1, 8, 8, 8, 8, s) == -22
    assert call(src, yuv_fmt(9, 0, 0, 0), None, kn, 16, 235, d, 0, 1, 8, 8, 8, 8, s) == -22
    assert call(src + 1, yuv_fmt(10, 0, 0, 0), None, kn, 64, 940, d, 0, 1, 8, 8, 8, 8, s) == -22
    for T, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert call(src, f, None, kn, 16, 235, d, 0, T, H, W, 8, 8, s) == -22
    assert call(None, f, None, kn, 16, 235, d, 0, 1, 8, 8, 8, 8, s) == -22 and call(src, f, None, kn, 16, 235, None, 0, 1, 8, 8, 8, 8, s) == -22
    assert call(src, None, None, kn, 16, 235, d, 0, 1, 8, 8, 8, 8, s) == -22 and call(src, f, None, None, 16, 235, d, 0, 1, 8, 8, 8, 8, s) == -22
    for bad in (float("nan"), float("inf")):
        assert call(src, f, None, (C.c_float * 16)(*([0.02] * 15 + [bad])), 16, 235, d, 0, 1, 8, 8, 8, 8, s) == -22
    torch.cuda.synchronize()
    assert bool((dst[:64] == float(np.float32(0.02))).all()) and int((dst != 0).sum()) == 64           # the two legal calls wrote 8 x 8 and 4 x 4, nothing else did
    with pytest.raises(ValueError, match="knots"):
        noise_map_level(buf[:96].view(1, 96), f, 8, 8, 8, 8, [0.02] * 15, torch.float32)


# ---- the restorer -----------------------------------------------------------------------------------------------------------------------------
H, W, ONE_LEN, FRAMES = 36, 44, 3, 8
FMT = R.Fmt(8, R.C420_CENTER, R.BT601, R.LIMITED)                                              # what the command line assumes below 720 rows


def two_band_clip(split=22, seed=11):
    """8 frames of 36 x 44: the left part at the centre code of band 3 with noise of sigma 5 luma codes, the right part at band 12's with sigma 2,
    noisy chroma.  18 x 11 blocks a side and frame: a window of 7 (6) input frames has 1386 (1188) blocks in each of the two bands."""
    rng = np.random.default_rng(seed)
    ch, cw = R.chroma_shape(FMT, H, W)
    x = np.arange(W)[None, :]
    out = []
    for _ in range(FRAMES):
        Y = np.where(x < split, 64.0 + rng.normal(0.0, 5.0, (H, W)), 187.0 + rng.normal(0.0, 2.0, (H, W)))
        U, V = (np.clip(np.rint(128 + rng.normal(0.0, 3.0, (ch, cw))), 16, 240).astype(np.int64) for _ in range(2))
        out.append(R.join_planes(np.clip(np.rint(Y), 0, 255).astype(np.int64), U, V, FMT))
    return out


def run(net, pay, h, w, **kw):
    kw.setdefault("sigma", "auto")
    vr = restore.VideoRestorer(net, ONE_LEN, **kw)
    out = list(vr.restore(iter(pay), yuv_fmt(*FMT), h, w))
    return out, vr.stats


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def by_hand(net, pay, h, w, clamp=(0.0, 50.0)):
    """reference curve -> reference map -> forward_fp32_out(x, map, shortcut) -> egress_yuv, window by window; returns (payloads, curves)."""
    f = yuv_fmt(*FMT)
    dt = next(net.parameters()).dtype
    name = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}[dt]
    hp, wp = restore.padded_size(h, w, net.V.topo)
    lo, hi = N.clip_codes(FMT)
    out, curves = [], []
    for first, cnt, idx in restore.plan_windows(len(pay), ONE_LEN):
        stack = np.stack([pay[i] for i in idx])
        curve = F.curve_ref(F.hist_bands_ref(stack, FMT, h, w, lo, hi), FMT, clamp)
        curves.append(curve)
        bits = F.map_ref(stack, FMT, h, w, hp, wp, F.knots32(curve), lo, hi, name)
        nm = torch.from_numpy(bits.view(np.int16) if name != "fp32" else bits).cuda()
        nm = (nm.view(dt) if name != "fp32" else nm).view(1, len(idx), 1, hp, wp)
        dev = torch.from_numpy(stack).cuda()
        x = ingest_yuv(dev, f, h, w, hp, wp, dt)
        kw = {} if dt == torch.float32 else {"shortcut": ingest_yuv(dev, f, h, w, hp, wp, torch.float32)}
        with torch.no_grad():
            y = net.forward_fp32_out(x, nm, **kw)
        assert tuple(y.shape) == (cnt, 3, hp, wp)
        out += list(egress_yuv(y, f, h, w).cpu().numpy())
    return out, curves


@pytest.fixture(scope="module")
def net():
    return restore.load_net("denoise_small", "synthetic", "bf16")


@pytest.fixture(scope="module")
def level(net):
    """The clip restored with noise_model="level", pipelined: shared by the tests below and left unchanged."""
    pay = two_band_clip()
    out, stats = run(net, pay, H, W, noise_model="level")
    return pay, out, stats


def test_level_writes_the_bytes_of_the_manual_composition(net, level):
    pay, out, stats = level
    want, curves = by_hand(net, pay, H, W)
    assert len(curves) == 3 and all(c[3] > 2.0 * c[12] > 0.0 for c in curves)                   # two bands with an estimate of their own, the rest filled
    assert all(c[0] == c[3] and c[15] == c[12] and c[3] > c[7] > c[12] for c in curves)
    assert stats["window_nlf"] == curves                                                       # floats compared with ==
    assert len(out) == FRAMES and same(out, want)
    assert stats["nlf_launches"] == stats["nlf_map_launches"] == stats["noise_launches"] == stats["windows"] == 3
    assert len(stats["window_sigma"]) == 3 and "window_frame_sigma" in stats                   # the flat estimate still runs and is still reported
    flat, fstats = run(net, pay, H, W)
    assert not same(flat, out) and "window_nlf" not in fstats and "nlf_launches" not in fstats  # the plane does reach the network; None is today's path
    assert fstats["window_sigma"] == stats["window_sigma"]


def test_level_is_the_same_with_the_pipeline_off_and_with_the_curves_fed_back(net, level):
    pay, out, stats = level
    off, ostats = run(net, pay, H, W, noise_model="level", pipeline=False)
    assert same(off, out) and ostats["window_nlf"] == stats["window_nlf"]
    listed, lstats = run(net, pay, H, W, sigma=10.0, noise_model=stats["window_nlf"])
    assert same(listed, out)
    assert lstats["window_nlf"] == stats["window_nlf"] and lstats["nlf_launches"] == 0 and lstats["noise_launches"] == 0 and lstats["nlf_map_launches"] == 3
    with pytest.raises(ValueError, match="window 2"):
        run(net, pay, H, W, noise_model=stats["window_nlf"][:2])
    clamped, cstats = run(net, pay, H, W, noise_model="level", sigma_clamp=(4.0, 6.0))          # the curve is clamped to sigma_clamp
    assert cstats["window_nlf"] == [[min(max(k, 4.0), 6.0) for k in c] for c in stats["window_nlf"]]
    assert not same(clamped, out)


def test_level_inside_a_picture_writes_the_bytes_of_the_cropped_stream(net):
    """One dark band over the whole frame: the rectangle's 12 x 14 blocks x 7 input frames reach NLF_MIN_BLOCKS in the windows of 7 frames."""
    rect = (4, 6, 28, 24)
    pay = two_band_clip(split=W)
    whole, stats = run(net, pay, H, W, noise_model="level", picture=rect)
    crop = list(P.crop_payloads(np.stack(pay), FMT, H, W, rect))
    want, cstats = run(net, crop, rect[3], rect[2], noise_model="level")
    assert stats["window_nlf"] == cstats["window_nlf"] and any(max(c) > 0.0 for c in stats["window_nlf"])
    assert np.array_equal(P.crop_payloads(np.stack(whole), FMT, H, W, rect), np.stack(want))
    assert np.array_equal(P.paste_payloads(np.stack(whole), np.stack(crop), FMT, H, W, rect), np.stack(pay))      # outside: as it came in


def test_restore_video_cli_round_trip_through_noise_model_out(tmp_path, level):
    pay, api, stats = level
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, dst2, nlf = tmp_path / "in.y4m", tmp_path / "out.y4m", tmp_path / "out2.y4m", tmp_path / "nlf.txt"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    base = [sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "denoise_small", "--checkpoint", "synthetic",
            "--dtype", "bf16", "--one_len", str(ONE_LEN), "--sigma", "auto"]
    r = subprocess.run(base + ["--noise_model", "level", "--noise_model_out", str(nlf), str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "done: 8 frames" in r.stderr and "noise model (level)" in r.stderr
    assert noise.parse_curves(nlf.read_text()) == stats["window_nlf"]

    def read(path):
        with open(path, "rb") as fh:
            return list(y4m.Y4MReader(fh))
    got = read(dst)
    assert same(got, api)
    r = subprocess.run(base + ["--noise_model", str(nlf), str(src), str(dst2)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "noise model (listed)" in r.stderr and same(read(dst2), got)
