"""-m gpu: the tiled restorer.  ``sn_tile_accumulate`` (csrc/sn_tile.hip) against the numpy restatement of tests/tile_ref.py bit for bit, its argument
checks, and ``VideoRestorer(tile=...)`` against a composition written out here: the network on each contiguous crop, tile_ref's blend, the existing
egress -- byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import picture_ref as P
import tile_ref as TR
import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import noise, restore, synth, windows, y4m
from shiftnet_amd.io_edges import egress_yuv, ingest_u8, ingest_yuv, noise_map_level, tile_accumulate, yuv_fmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HC, WC, GUARD = 40, 56, 64              # the canvas of the kernel tests, and the floats kept on either side of it (64 floats keep its 16-byte alignment)


def values(rng, shape):
    """float32 of both signs: most of magnitude about 1, one in eight up to 1e4, a few exact zeros."""
    v = rng.standard_normal(shape)
    big = rng.random(shape) < 0.125
    v = np.where(big, rng.uniform(-1e4, 1e4, shape), v)
    v = np.where(rng.random(shape) < 0.02, 0.0, v)
    return v.astype(np.float32)


def weights(rng, n):
    """float32 in [0, 1] with exact 0 and exact 1 among them."""
    w = rng.random(n).astype(np.float32)
    w[rng.integers(0, n)] = 0.0
    w[(np.flatnonzero(w)[0])] = 1.0
    return w


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Canvas:
    """A [T, 3, HC, WC] canvas inside a larger device buffer, ``shift`` floats off 16-byte alignment, with its host twin."""

    def __init__(self, rng, T, shift=0):
        self.n = T * 3 * HC * WC
        self.lo = GUARD + shift
        self.host = values(rng, self.n + 2 * GUARD + 4)
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        self.view = self.dev[self.lo:self.lo + self.n].view(T, 3, HC, WC)
        self.want = self.host[self.lo:self.lo + self.n].reshape(T, 3, HC, WC)      # a view: the reference changes the host twin in place

    def check(self, what):
        got = self.dev.cpu().numpy()
        assert np.array_equal(bits(got[self.lo:self.lo + self.n]), bits(self.host[self.lo:self.lo + self.n])), what
        assert np.array_equal(bits(got[:self.lo]), bits(self.host[:self.lo])) and np.array_equal(bits(got[self.lo + self.n:]), bits(self.host[self.lo + self.n:])), what


TILES = [(8, 8), (16, 24), (12, 20), (5, 7)]      # (5, 7): a row that ends inside a thread's four samples, rows at every alignment


@pytest.mark.parametrize("T", [1, 3])
def test_the_kernel_equals_the_restatement_bit_for_bit_and_touches_nothing_else(T):
    rng = np.random.default_rng(100 + T)
    for th, tw in TILES:
        places = [(y0, x0) for y0 in (0, 5) for x0 in (0, 1, 3, 4)] + [(HC - th, WC - tw)]
        for shift, tile_shift in ((0, 0), (1, 0), (0, 1)):                           # canvas / tile off 16-byte alignment: the element-wise path at x0 = 0 too
            c = Canvas(rng, T, shift)
            for y0, x0 in places:                                                    # accumulated in order into one canvas: the places overlap
                tile = values(rng, (T, 3, th, tw))
                wy, wx = weights(rng, th), weights(rng, tw)
                store = torch.zeros(tile.size + 4, dtype=torch.float32, device="cuda")
                tdev = store[tile_shift:tile_shift + tile.size].view(T, 3, th, tw)
                tdev.copy_(torch.from_numpy(tile))
                assert tile_accumulate(tdev, c.view, torch.from_numpy(wy).cuda(), torch.from_numpy(wx).cuda(), y0, x0) is c.view
                TR.accumulate(c.want, tile, wy, wx, y0, x0)
                c.check((T, th, tw, y0, x0, shift, tile_shift))


def test_three_overlapping_tiles_accumulated_in_order_equal_the_restatement():
    rng = np.random.default_rng(7)
    plan = windows.plan_tiles(HC, WC, 16, 24, 4)                                     # 3 x 3 tiles: rows at 0, 12, 24, columns at 0, 20, 32 (the last shifted)
    assert len(plan.ys) == 3 and len(plan.xs) == 3
    c = Canvas(rng, 3)
    c.dev[c.lo:c.lo + c.n] = 0
    c.host[c.lo:c.lo + c.n] = 0
    results = [values(rng, (3, 3, 16, 24)) for _ in plan.tiles]
    wy, wx = torch.from_numpy(plan.wy).cuda(), torch.from_numpy(plan.wx).cuda()
    for i, ((y0, x0, _, _), r) in enumerate(zip(plan.tiles, results)):
        tile_accumulate(torch.from_numpy(r).cuda(), c.view, wy[i // 3], wx[i % 3], y0, x0)
    c.want[...] = TR.blend(results, plan, (3, 3, HC, WC))
    c.check("3 x 3")
    same = [np.full((3, 3, 16, 24), 0.625, np.float32)] * 9                          # the blend of a constant is the constant, to the weights' rounding
    c.dev[c.lo:c.lo + c.n] = 0
    for i, (y0, x0, _, _) in enumerate(plan.tiles):
        tile_accumulate(torch.from_numpy(same[i]).cuda(), c.view, wy[i // 3], wx[i % 3], y0, x0)
    # the weights of an axis sum to 1 within 4 ulp (tests/test_host_tiles.py), so their products within 8; up to four terms of three roundings of half
    # an ulp each add 6: 14 ulp of 1.0 at most, times the constant
    assert float((c.view.double() - 0.625).abs().max()) <= 0.625 * 16 * 2.0 ** -23


def test_illegal_arguments_are_refused_before_anything_is_launched():
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    GARBAGE = 1234.5
    canvas = torch.full((1, 3, HC, WC), GARBAGE, device="cuda")
    tile = torch.ones((1, 3, 8, 8), device="cuda")
    w = torch.ones(8, device="cuda")
    t, c, y, x = tile.data_ptr(), canvas.data_ptr(), w.data_ptr(), w.data_ptr()

    def call(tp=t, cp=c, yp=y, xp=x, T=1, C=3, th=8, tw=8, Hc=HC, Wc=WC, y0=0, x0=0):
        return lib.sn_tile_accumulate(tp, cp, yp, xp, T, C, th, tw, Hc, Wc, y0, x0, s)
    for kw in ({"tp": None}, {"cp": None}, {"yp": None}, {"xp": None},                                   # a null pointer
               {"tp": t + 2}, {"cp": c + 1}, {"yp": y + 2}, {"xp": x + 3},                               # a pointer that is not 4-byte aligned
               {"T": 0}, {"C": 0}, {"th": 0}, {"tw": 0}, {"Hc": 0}, {"Wc": 0}, {"T": -1}, {"th": -8},     # a size below 1
               {"y0": -1}, {"x0": -1}, {"y0": HC - 7}, {"x0": WC - 7}, {"th": HC + 1, "y0": 0}, {"y0": 2 ** 31 - 1}, {"x0": 2 ** 31 - 1},
               {"T": 21846, "C": 3}, {"T": 65536, "C": 1}, {"T": 2 ** 16, "C": 2 ** 16}):                # T * C > 65535 (the last: a product past 2^31)
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()
    assert bool((canvas == GARBAGE).all())                                           # nothing was launched
    assert call(y0=HC - 8, x0=WC - 8) == 0 and call(tp=t + 4, th=7, tw=8, cp=c + 4, Wc=WC - 1, xp=x, yp=y + 4) == 0      # legal: the far corner; 4-byte alignment
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="inside"):
        tile_accumulate(tile, canvas, w, w, HC - 7, 0)
    with pytest.raises(ValueError, match="float32"):
        tile_accumulate(tile.half(), canvas, w, w, 0, 0)
    with pytest.raises(ValueError, match="wy"):
        tile_accumulate(tile, canvas, w[:7], w, 0, 0)
    with pytest.raises(ValueError, match="contiguous"):
        tile_accumulate(tile[..., ::2], canvas, w, w[:4], 0, 0)


# ---- the restorer -------------------------------------------------------------------------------------------------------------------------
FMT = R.Fmt(8, R.C420_CENTER, R.BT601, R.LIMITED)
H, W, FRAMES, ONE_LEN = 40, 56, 7, 3
TILE, OVERLAP = (24, 32), 8
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
NEW_KEYS = {"tile", "tile_overlap", "window_tiles", "tile_launches"}


def clip(sigma=0.0, h=H, w=W, seed=3):
    """FRAMES payloads of the synthetic sharp clip, 4:2:0 8 bit, made by the existing egress."""
    rgb = synth.sharp_clip(FRAMES, h, w, seed)
    if sigma:
        rgb = np.clip(np.rint(rgb.astype(np.float64) + np.random.default_rng(seed).normal(0.0, sigma, rgb.shape)), 0, 255).astype(np.uint8)
    x = ingest_u8(torch.from_numpy(rgb).cuda(), torch.float32)[0]
    return list(egress_yuv(x, yuv_fmt(*FMT), h, w).cpu().numpy())


def run(net, pay, h=H, w=W, **kw):
    vr = restore.VideoRestorer(net, ONE_LEN, **kw)
    out = list(vr.restore(iter(pay), yuv_fmt(*FMT), h, w))
    return out, vr.stats, vr


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def composed(net, pay, tile, overlap, sigma=None, curves=None, blend=TR.blend):
    """What the tiled restorer must write, window by window: the existing ingest on the whole frames, ``net.forward_fp32_out`` on each contiguous crop
    (of the float32 twin and of the noise plane as well), ``blend`` of the results on the host, the existing egress on the blended canvas."""
    f = yuv_fmt(*FMT)
    dt = next(net.parameters()).dtype
    hp, wp = windows.padded_size(H, W, net.V.topo)
    plan = windows.plan_tiles(hp, wp, tile[0], tile[1], overlap)
    lo, hi = noise.clip_codes(FMT.bits, FMT.range)
    out, tiles = [], []
    for k, (_, n, idx) in enumerate(windows.plan_windows(FRAMES, ONE_LEN)):
        dev = torch.from_numpy(np.stack([pay[i] for i in idx])).cuda()
        t = len(idx)
        x = ingest_yuv(dev, f, H, W, hp, wp, dt)
        x32 = ingest_yuv(dev, f, H, W, hp, wp, torch.float32) if dt != torch.float32 else None
        plane = None
        if curves is not None:
            plane = noise_map_level(dev, f, H, W, hp, wp, [c / 255.0 for c in curves[k]], dt, lo, hi)
        results = []
        for y0, x0, th, tw in plan.tiles:
            crop = (slice(None), slice(None), slice(None), slice(y0, y0 + th), slice(x0, x0 + tw))
            kw = {"shortcut": x32[crop].contiguous()} if x32 is not None else {}
            if plane is not None:
                o = net.forward_fp32_out(x[crop].contiguous(), plane[crop].contiguous(), **kw)
            elif sigma is not None:
                o = net.forward_fp32_out(x[crop].contiguous(), torch.full((1, 1, 1, 1, 1), sigma / 255.0, dtype=dt, device="cuda").expand(1, t, 1, th, tw), **kw)
            else:
                o = net.forward_fp32_out(x[crop].contiguous(), **kw)
            assert o.dtype == torch.float32 and tuple(o.shape) == (n, 3, th, tw)
            results.append(o.cpu().numpy())
        canvas = blend(results, plan, (n, 3, hp, wp))
        out += list(egress_yuv(torch.from_numpy(canvas).cuda(), f, H, W).cpu().numpy())
        tiles.append(list(plan.tiles))
    return out, tiles


@pytest.fixture(scope="module")
def deblur():
    """Per dtype: the net, the clip, the untiled run."""
    pay = clip()
    made = {}
    for name in DTYPES:
        net = restore.load_net("deblur_small", "synthetic", name)
        full, stats, vr = run(net, pay)
        assert not (NEW_KEYS & set(stats)) and vr.run.launches["tile"] == 0 and not same(full, pay)
        made[name] = (net, full, stats)
    return pay, made


@pytest.mark.parametrize("name", list(DTYPES))
def test_the_tiled_deblurrer_writes_the_bytes_of_the_composition(deblur, name):
    pay, made = deblur
    net, full, _ = made[name]
    want, tiles = composed(net, pay, TILE, OVERLAP)
    got, stats, _ = run(net, pay, tile=TILE, tile_overlap=OVERLAP)
    assert same(got, want)
    assert stats["tile"] == TILE and stats["tile_overlap"] == OVERLAP and stats["window_tiles"] == tiles and stats["frames"] == FRAMES
    assert tiles[0] == [(0, 0, 24, 32), (0, 24, 24, 32), (16, 0, 24, 32), (16, 24, 24, 32)] and stats["tile_launches"] == 12 and stats["windows"] == 3
    assert not same(got, full)                                                       # a tiled result is not the full-frame result
    serial, stats2, _ = run(net, pay, tile=TILE, tile_overlap=OVERLAP, pipeline=False)
    assert same(serial, got) and stats2["window_tiles"] == tiles and stats2["tile_launches"] == 12
    assert same(run(net, pay, tile=24, tile_overlap=OVERLAP)[0], composed(net, pay, (24, 24), OVERLAP)[0])      # an int is a square; 2 x 3 tiles


def test_overlap_zero_is_plain_crop_assembly(deblur):
    pay, made = deblur
    net = made["bf16"][0]

    def assemble(results, plan, shape):
        canvas = np.zeros(shape, dtype=np.float32)
        for (y0, x0, th, tw), r in zip(plan.tiles, results):
            canvas[:, :, y0:y0 + th, x0:x0 + tw] = r
        return canvas
    want, tiles = composed(net, pay, (20, 28), 0, blend=assemble)                    # 40 = 2 x 20, 56 = 2 x 28: the tiles abut
    assert tiles[0] == [(0, 0, 20, 28), (0, 28, 20, 28), (20, 0, 20, 28), (20, 28, 20, 28)]
    got, stats, _ = run(net, pay, tile=(20, 28), tile_overlap=0)
    assert same(got, want) and stats["window_tiles"] == tiles and stats["tile_overlap"] == 0


@pytest.mark.parametrize("tile", [(40, 56), (48, 64), 64])
def test_a_tile_that_covers_the_picture_takes_the_untiled_path(deblur, tile):
    pay, made = deblur
    net, full, stats_full = made["bf16"]
    got, stats, vr = run(net, pay, tile=tile, tile_overlap=4)
    assert same(got, full)
    assert set(stats) - set(stats_full) == NEW_KEYS and set(stats_full) <= set(stats)
    assert stats["tile_launches"] == 0 and vr.run.launches["tile"] == 0 and stats["window_tiles"] == [[(0, 0, 40, 56)]] * 3
    assert {k: v for k, v in stats.items() if k.endswith("_launches") and k not in NEW_KEYS} == {k: v for k, v in stats_full.items() if k.endswith("_launches")}
    assert stats["windows"] == stats_full["windows"] and stats["frames"] == stats_full["frames"]


@pytest.fixture(scope="module")
def denoise():
    return restore.load_net("denoise_small", "synthetic", "bf16"), clip(sigma=10.0)


def test_the_tiled_denoiser_broadcasts_a_fixed_sigma_to_the_tiles_shape(denoise):
    net, pay = denoise
    want, tiles = composed(net, pay, TILE, OVERLAP, sigma=10.0)
    got, stats, _ = run(net, pay, sigma=10.0, tile=TILE, tile_overlap=OVERLAP)
    assert same(got, want) and stats["window_tiles"] == tiles and stats["window_sigma"] == [10.0] * 3
    assert not same(got, run(net, pay, sigma=10.0)[0])
    assert same(run(net, pay, sigma=10.0, tile=TILE, tile_overlap=OVERLAP, pipeline=False)[0], got)


def test_the_tiled_denoiser_slices_the_noise_plane_of_the_whole_picture(denoise):
    net, pay = denoise
    curves = [[14.0 - 0.5 * b - k for b in range(16)] for k in range(3)]             # one curve per window, falling from the shadows to the highlights
    want, tiles = composed(net, pay, TILE, OVERLAP, curves=curves)
    got, stats, _ = run(net, pay, sigma=10.0, noise_model=curves, tile=TILE, tile_overlap=OVERLAP)
    assert same(got, want) and stats["window_tiles"] == tiles and stats["nlf_map_launches"] == 3 and stats["tile_launches"] == 12
    assert not same(got, composed(net, pay, TILE, OVERLAP, sigma=10.0)[0])           # the plane reaches the tiles


RECT = (8, 4, 40, 32)                                                                # x0, y0, w, h: 32 x 40 samples are 2 x 2 tiles of 24 x 32
OFMT = R.Fmt(10, R.C444, FMT.matrix, FMT.range)


def boxed_and_cropped(net, pay, ofmt, **kw):
    """The restorer with ``picture=RECT`` on the stream and the same restorer on the cropped stream: (written, its rectangle cut out, the cropped
    stream's frames, the two stats)."""
    crop = list(P.crop_payloads(np.stack(pay), FMT, H, W, RECT))
    inner, stats_in, _ = run(net, crop, h=RECT[3], w=RECT[2], **kw)
    got, stats, _ = run(net, pay, picture=RECT, **kw)
    want_tiles = [[(0, 0, 24, 32), (0, 8, 24, 32), (8, 0, 24, 32), (8, 8, 24, 32)]] * 3 if kw.get("tile") is not None else None
    assert stats.get("window_tiles") == want_tiles == stats_in.get("window_tiles")
    assert len(got) == FRAMES and len(got[0]) == R.frame_bytes(ofmt, H, W)
    return got, list(P.crop_payloads(np.stack(got), ofmt, H, W, RECT)), inner, stats, stats_in


def test_picture_format_amount_and_report_together_equal_the_cropped_stream_inside_the_rectangle(denoise):
    """picture + out_format="444p10" + amount=0.5 + report=True with a tile equals, inside the rectangle, the same restorer on the cropped stream: the
    bytes and the report's sums.  The input side of the blend and of the report is, inside the rectangle of a tiled window, the rectangle converted as
    the cropped stream's frames are."""
    net, pay = denoise
    kw = dict(sigma=10.0, out_format="444p10", amount=0.5, report=True, tile=TILE, tile_overlap=OVERLAP)
    got, inside, inner, stats, stats_in = boxed_and_cropped(net, pay, OFMT, **kw)
    differ = sum(int((a.view("<u2") != b.view("<u2")).sum()) for a, b in zip(inside, inner))
    print(f"samples inside the rectangle that differ from the cropped stream: {differ} of {sum(a.size // 2 for a in inside)}")
    assert same(inside, inner)
    assert stats["frame_sums"] == stats_in["frame_sums"] and stats["tile_launches"] == stats_in["tile_launches"] == 12
    assert same(run(net, pay, picture=RECT, pipeline=False, **kw)[0], got)
    zero = dict(kw, amount=0.0)                                                      # amount 0: the converted input -- the rectangle's own conversion inside
    _, inside0, inner0, _, _ = boxed_and_cropped(net, pay, OFMT, **zero)
    assert same(inside0, inner0)


def test_picture_with_tiles_and_each_pair_of_the_other_options_and_the_untiled_restorer_beside_it(denoise):
    """picture + tile with the other options of the combined case two at a time: another format out with the report, and amount + report in the format
    read, equal the cropped stream inside the rectangle byte for byte and sum for sum.  All of them together WITHOUT a tile stay what they were: equal to
    the cropped stream away from the rectangle's edges -- 2 samples, the reach of the 4:2:0 chroma filters of the whole frame's conversion that the
    blend's input side goes through there.  Outside the rectangle the tiles change nothing."""
    net, pay = denoise
    tiled = dict(sigma=10.0, tile=TILE, tile_overlap=OVERLAP)
    _, inside, inner, stats, stats_in = boxed_and_cropped(net, pay, OFMT, out_format="444p10", report=True, **tiled)
    assert same(inside, inner) and stats["frame_sums"] == stats_in["frame_sums"] and stats["tile_launches"] == 12
    _, inside, inner, stats, stats_in = boxed_and_cropped(net, pay, FMT, amount=0.5, report=True, **tiled)
    assert same(inside, inner) and stats["frame_sums"] == stats_in["frame_sums"] and stats["tile_launches"] == 12
    kw = dict(out_format="444p10", amount=0.5, report=True)
    planes = lambda frames: np.stack(frames).view("<u2").reshape(FRAMES, 3, RECT[3], RECT[2])      # noqa: E731
    untiled, inside, inner, stats, _ = boxed_and_cropped(net, pay, OFMT, sigma=10.0, **kw)
    assert np.array_equal(planes(inside)[:, :, 2:-2, 2:-2], planes(inner)[:, :, 2:-2, 2:-2])
    assert len(stats["frame_sums"]) == FRAMES and all(r[0] == RECT[2] * RECT[3] for r in stats["frame_sums"])
    with_tiles, _, _ = run(net, pay, picture=RECT, **kw, **tiled)
    assert not same(untiled, with_tiles)
    outside = P.paste_payloads(np.stack(with_tiles), P.crop_payloads(np.stack(untiled), OFMT, H, W, RECT), OFMT, H, W, RECT)
    assert same(list(outside), untiled)                                              # outside the rectangle the tiles change nothing


def test_illegal_tiles_are_refused_at_construction(deblur):
    net = deblur[1]["bf16"][0]
    for tile, overlap in (((24, 30), 8), ((4, 32), 0), ((24, 32), 13), ((24, 32), -1), ("24x32", 8), ((24, 32, 8), 8), (True, 0), ((24, 32), 4.0)):
        with pytest.raises(ValueError, match="tile"):
            restore.VideoRestorer(net, ONE_LEN, tile=tile, tile_overlap=overlap)
    with pytest.raises(ValueError, match="tile_overlap"):
        restore.VideoRestorer(net, ONE_LEN, tile_overlap=-1)
    assert restore.VideoRestorer(net, ONE_LEN).tile is None and restore.VideoRestorer(net, ONE_LEN, tile=512).tile == (512, 512, 32)


# ---- the command line -------------------------------------------------------------------------------------------------------------------------
def test_restore_video_cli_with_a_tile_writes_the_restorers_bytes(tmp_path, deblur):
    pay, made = deblur
    want, _, _ = run(made["bf16"][0], pay, tile=TILE, tile_overlap=OVERLAP)
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "deblur_small", "--checkpoint", "synthetic", "--dtype", "bf16",
                        "--one_len", str(ONE_LEN), "--tile", "24x32", "--tile_overlap", str(OVERLAP), str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "tile: 24 x 32, overlap 8" in r.stderr and "tiles: 4 to 4 per window, 12 blended over 3 windows" in r.stderr
    with open(dst, "rb") as fh:
        assert same(list(y4m.Y4MReader(fh)), want)                                  # 40 < 720: the CLI's default matrix is BT.601, as FMT
