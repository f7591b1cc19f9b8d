"""-m gpu: the active picture.  The three ``_rect`` entry points of csrc/sn_yuv.hip and csrc/sn_yuv_stats.hip against the restatements of tests/yuv_ref.py and
tests/noise_ref.py on the CROPPED stream (tests/picture_ref.py), bit for bit; ``sn_yuv_rowcol_sums`` against numpy exactly; and the video
restorer with ``picture=`` against itself on the cropped stream, byte for byte inside the rectangle, and against its input outside."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import noise_ref as N
import picture_ref as P
import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import picture, restore, synth, y4m
from shiftnet_amd.io_edges import egress_yuv, ingest_yuv, noise_hist_yuv, rowcol_sums_yuv, yuv_fmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"420jpeg": (8, R.C420_CENTER), "420mpeg2": (8, R.C420_LEFT), "444": (8, R.C444), "420p10": (10, R.C420_LEFT), "444p10": (10, R.C444)}
COLOURS = {"601lim": (R.BT601, R.LIMITED), "709full": (R.BT709, R.FULL)}
FORMATS = {f"{m}-{c}": R.Fmt(*MODES[m], *COLOURS[c]) for m in MODES for c in COLOURS}
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
# (H, W) of the stream -> rectangles (x0, y0, w, h).  70 x 37: odd sizes, one workgroup; the whole frame, rows at addresses of no alignment, odd w and
# h reaching both far edges, hardly more than a lane's 8 x 2 unit.  304 x 40: W % 16 == 0 and two workgroups along x; the whole frame and a
# rectangle whose rows keep the wide loads.
STREAMS = {(37, 70): [(0, 0, 70, 37), (2, 4, 40, 22), (8, 0, 62, 37), (16, 2, 10, 4)],
           (40, 304): [(0, 0, 304, 40), (16, 2, 272, 32)]}
CASES = [(H, W, rect, T) for (H, W), rects in STREAMS.items() for rect in rects for T in (1, 3)]


def pads(rect):
    """The padded sizes of the two topologies: the next multiple of 4 and of 8."""
    return [((rect[3] + m - 1) // m * m, (rect[2] + m - 1) // m * m) for m in (4, 8)]


def random_payloads(fmt, T, H, W, seed):
    rng = np.random.default_rng(seed)
    n = R.frame_bytes(fmt, H, W)
    if fmt.bits == 8:
        return rng.integers(0, 256, (T, n), dtype=np.uint8)
    return rng.integers(0, 1024, (T, n // 2)).astype("<u2").view(np.uint8).reshape(T, n)


def bits_of(t: torch.Tensor, name: str) -> np.ndarray:
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if name != "fp32" else t.numpy().view(np.uint32)


def want_bits(a: np.ndarray, name: str) -> np.ndarray:
    return a.view(np.uint16) if name != "fp32" else a.view(np.uint32)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FORMATS.values()), ids=list(FORMATS))
def test_ingest_rect_equals_the_restatement_on_the_cropped_stream_bit_for_bit(fmt):
    f = yuv_fmt(*fmt)
    for H, W, rect, T in CASES:
        p = random_payloads(fmt, T, H, W, seed=H * 1000 + W + T)
        dev = torch.from_numpy(p).cuda()
        crop = P.crop_payloads(p, fmt, H, W, rect)
        for Hp, Wp in pads(rect):
            for name, dt in DTYPES.items():
                got = ingest_yuv(dev, f, H, W, Hp, Wp, dt, rect=rect)
                assert got.shape == (1, T, 3, Hp, Wp) and got.dtype == dt
                want = R.ingest_emu(crop, fmt, rect[3], rect[2], Hp, Wp, name)
                assert np.array_equal(bits_of(got[0], name), want_bits(want, name)), (fmt, H, W, rect, Hp, Wp, T, name)
                if rect == (0, 0, W, H):                                            # the whole frame: the entry point without a rectangle
                    assert torch.equal(got, ingest_yuv(dev, f, H, W, Hp, Wp, dt))
                out = torch.full((1, T, 3, Hp, Wp), 7.0, dtype=dt, device="cuda")     # the filling form writes the same
                assert ingest_yuv(dev, f, H, W, Hp, Wp, dt, out=out, rect=rect) is out and torch.equal(out, got)


@pytest.mark.parametrize("fmt", list(FORMATS.values()), ids=list(FORMATS))
def test_egress_rect_writes_the_cropped_streams_samples_into_the_rectangle_and_nothing_else(fmt):
    f = yuv_fmt(*fmt)
    GUARD = 64
    for H, W, rect, T in CASES:
        fb = R.frame_bytes(fmt, H, W)
        rng = np.random.default_rng(H * 1000 + W + T + 5)
        pre = rng.integers(0, 256, T * fb + 2 * GUARD, dtype=np.uint8)               # what the payloads and the guards hold before
        for Hp, Wp in pads(rect):
            g = torch.Generator().manual_seed(H * 1000 + W + T + Hp)
            x32 = torch.rand(T, 3, Hp, Wp, generator=g) * 1.4 - 0.2                  # values below 0 and above 1: the clamp matters
            for name, dt in DTYPES.items():
                x = x32.to(dt)
                buf = torch.from_numpy(pre).cuda()
                dst = buf[GUARD:GUARD + T * fb].view(T, fb)
                got = egress_yuv(x.cuda(), f, H, W, dst=dst, rect=rect)
                assert got is dst
                inner = R.egress_emu(x.float().numpy(), fmt, rect[3], rect[2])
                want = P.paste_payloads(pre[GUARD:GUARD + T * fb].reshape(T, fb), inner, fmt, H, W, rect)
                b = buf.cpu().numpy()
                assert np.array_equal(b[GUARD:GUARD + T * fb].reshape(T, fb), want), (fmt, H, W, rect, Hp, Wp, T, name)
                assert np.array_equal(b[:GUARD], pre[:GUARD]) and np.array_equal(b[GUARD + T * fb:], pre[GUARD + T * fb:])
                if rect == (0, 0, W, H):
                    assert np.array_equal(egress_yuv(x.cuda(), f, H, W).cpu().numpy(), want)
    got = egress_yuv(torch.rand(2, 3, 8, 16).cuda(), f, 37, 70, rect=(16, 2, 10, 4))  # allocating form: zeros outside the rectangle
    assert got.shape == (2, R.frame_bytes(fmt, 37, 70))
    z = np.zeros_like(got.cpu().numpy())
    assert np.array_equal(P.paste_payloads(got.cpu().numpy(), P.crop_payloads(z, fmt, 37, 70, (16, 2, 10, 4)), fmt, 37, 70, (16, 2, 10, 4)), z)


@pytest.mark.parametrize("bits", [8, 10])
def test_rowcol_sums_equal_numpy_exactly_overwrite_and_write_nothing_else(bits):
    fmt = R.Fmt(bits, R.C420_CENTER, R.BT709, R.LIMITED)
    f = yuv_fmt(*fmt)
    GUARD = 64
    # the two streams, and one with two workgroups along both axes (a wave covers 512 pixels, a workgroup 64 rows)
    for (H, W), T in [(s, t) for s in [(37, 70), (40, 304), (70, 520)] for t in (1, 3)]:
        p = random_payloads(fmt, T, H, W, seed=H * 1000 + W + T)
        if T == 3:                                                                   # one frame of the top code: the largest sums
            p[1, :H * W * (1 if bits == 8 else 2)] = 0xFF if bits == 8 else np.tile(np.array([0xFF, 0x03], np.uint8), H * W)
        wr, wc = P.rowcol_ref(p, fmt, H, W)
        fb = R.frame_bytes(fmt, H, W)
        for off in ((0, 1) if bits == 8 else (0, 2)):                                # 8 bit: payloads at odd addresses as well (element-wise loads)
            buf = torch.zeros(T * fb + 16, dtype=torch.uint8, device="cuda")
            src = buf[off:off + T * fb].view(T, fb)
            src.copy_(torch.from_numpy(p))
            g = torch.from_numpy(np.full(T * (H + W) + 3 * GUARD, 0xA5A5A5A5, np.uint32)).cuda()       # garbage: overwritten, not added to
            rows = g[GUARD:GUARD + T * H].view(T, H)
            cols = g[2 * GUARD + T * H:2 * GUARD + T * (H + W)].view(T, W)
            for call in (1, 2):                                                      # a second call into the same buffers: the same values
                r, c = rowcol_sums_yuv(src, f, H, W, out_rows=rows, out_cols=cols)
                assert r is rows and c is cols
                b = g.cpu().numpy()
                assert np.array_equal(b[GUARD:GUARD + T * H].reshape(T, H), wr), (bits, H, W, T, off, call)
                assert np.array_equal(b[2 * GUARD + T * H:2 * GUARD + T * (H + W)].reshape(T, W), wc), (bits, H, W, T, off, call)
                for guard in (b[:GUARD], b[GUARD + T * H:2 * GUARD + T * H], b[2 * GUARD + T * (H + W):]):
                    assert (guard == 0xA5A5A5A5).all()
    r, c = rowcol_sums_yuv(torch.from_numpy(p).cuda(), f, H, W)                      # allocating form
    assert r.dtype == c.dtype == torch.uint32 and np.array_equal(r.cpu().numpy(), wr) and np.array_equal(c.cpu().numpy(), wc)
    top = (1 << bits) - 1
    assert int(wr.max()) == top * W and int(wc.max()) == top * H                     # the frame of the top code


@pytest.mark.parametrize("fmt", list(FORMATS.values()), ids=list(FORMATS))
def test_noise_hist_rect_equals_the_restatement_on_the_cropped_luma(fmt):
    f = yuv_fmt(*fmt)
    lo, hi = N.clip_codes(fmt)
    for H, W, rect, T in CASES:
        p = random_payloads(fmt, T, H, W, seed=H * 1000 + W + T + 11)
        want = N.hist_ref(P.crop_payloads(p, fmt, H, W, rect), fmt, rect[3], rect[2], lo, hi)
        assert want.sum() > 0
        out = torch.from_numpy(np.full((T, N.nbins(fmt.bits)), 0xA5A5A5A5, np.uint32)).cuda()
        got = noise_hist_yuv(torch.from_numpy(p).cuda(), f, H, W, lo, hi, out=out, rect=rect)
        assert np.array_equal(got.cpu().numpy(), want), (fmt, H, W, rect, T)
        if rect == (0, 0, W, H):
            assert np.array_equal(noise_hist_yuv(torch.from_numpy(p).cuda(), f, H, W, lo, hi).cpu().numpy(), want)


def test_illegal_rectangles_and_sizes_are_refused_before_anything_is_launched():
    lib = L.load()
    f420, f444 = yuv_fmt(8, L.SN_YUV_420_CENTER, 0, 0), yuv_fmt(8, L.SN_YUV_444, 0, 0)
    buf = torch.zeros(3 * 40 * 70, dtype=torch.uint8, device="cuda")
    x = torch.zeros(1, 3, 40, 72, device="cuda")
    h32 = torch.zeros(2047, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    H, W = 37, 70
    ing = lambda fm, r, hp=40, wp=72: lib.sn_ingest_yuv_rect(buf.data_ptr(), fm, r, x.data_ptr(), L.SN_F32, 1, H, W, hp, wp, s)   # noqa: E731
    egr = lambda fm, r, hp=40, wp=72: lib.sn_egress_yuv_rect(x.data_ptr(), L.SN_F32, fm, r, buf.data_ptr(), 1, H, W, hp, wp, s)   # noqa: E731
    hst = lambda fm, r: lib.sn_yuv_noise_hist_rect(buf.data_ptr(), fm, r, h32.data_ptr(), 16, 235, 1, H, W, s)                     # noqa: E731
    ok = L.YuvRect(2, 4, 40, 22)
    for call in (ing, egr, hst):
        assert call(f420, ok) == 0
        assert call(f420, None) == -22
        for bad in [(1, 4, 40, 22), (2, 3, 40, 22), (2, 4, 39, 22), (2, 4, 40, 21), (-2, 4, 40, 22), (2, 4, 70, 22), (2, 4, 40, 34), (0, 0, 0, 8), (0, 0, 8, 0),
                    (2, 4, 2 ** 31 - 1, 22)]:
            assert call(f420, L.YuvRect(*bad)) == -22, bad
        for fine in [(1, 3, 39, 21), (69, 36, 1, 1)]:                                # 4:4:4 takes any integers inside the frame
            assert call(f444, L.YuvRect(*fine)) == 0, fine
        assert call(f420, L.YuvRect(8, 0, 62, 37)) == 0                             # odd w and h that reach the far edges
    assert ing(f420, ok, 20, 72) == -22 and ing(f420, ok, 40, 36) == -22 and ing(f420, ok, 22, 40) == 0      # Hp, Wp against the rectangle
    assert egr(f420, ok, 20, 72) == -22 and egr(f420, ok, 40, 36) == -22
    r32 = torch.zeros(256, dtype=torch.int32, device="cuda")
    sums = lambda fm, rows, cols, T=1, h=H, w=W: lib.sn_yuv_rowcol_sums(buf.data_ptr(), fm, rows, cols, T, h, w, s)               # noqa: E731
    rp, cp = r32.data_ptr(), r32.data_ptr() + 4 * 64
    assert sums(f420, rp, cp) == 0
    assert sums(f420, None, cp) == -22 and sums(f420, rp, None) == -22 and sums(None, rp, cp) == -22
    assert sums(f420, rp + 2, cp) == -22 and sums(f420, rp, cp + 1) == -22
    assert sums(yuv_fmt(12, 0, 0, 0), rp, cp) == -22 and sums(yuv_fmt(8, 3, 0, 0), rp, cp) == -22
    for T, h, w in ((0, H, W), (1, 0, W), (1, H, 0), (1, 65536, 1), (1, 1, 65536)):
        assert sums(f420, rp, cp, T, h, w) == -22
    assert lib.sn_yuv_rowcol_sums(buf.data_ptr() + 1, yuv_fmt(10, 0, 0, 0), rp, cp, 1, 8, 8, s) == -22        # 16-bit samples at an odd address
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="even"):
        ingest_yuv(buf[:R.frame_bytes(R.Fmt(8, 1, 0, 0), H, W)].view(1, -1), f420, H, W, 40, 72, torch.float32, rect=(1, 4, 40, 22))


# ---- the restorer ---------------------------------------------------------------------------------------------------------------------------
FMT420 = R.Fmt(8, R.C420_CENTER, R.BT601, R.LIMITED)
B = P.BOXED
RECT, H, W, ONE_LEN = B["rect"], B["h"], B["w"], B["one_len"]


def boxed_clip(n=B["n"], sigma=0.0, seed=3, edges=False):
    """n frames of the synthetic sharp clip at 72 x 128 inside RECT of a 96 x 128 stream, bars at the black code (16, chroma 128).  edges: the
    picture's first and last two rows and columns are random saturated colours, a new draw per frame: the strongest contrast against the bars right
    where a bar sample would leak in (the chroma filters of both edges, the 3 x 3 stacks)."""
    rgb = synth.sharp_clip(n, RECT[3], RECT[2], seed).copy()
    if edges:
        rng = np.random.default_rng(seed + 100)
        for sl in (np.s_[:, :2], np.s_[:, -2:], np.s_[:, :, :2], np.s_[:, :, -2:]):
            rgb[sl] = rng.integers(0, 2, rgb[sl].shape, dtype=np.uint8) * 255
    if sigma:
        rgb = np.clip(np.rint(rgb.astype(np.float64) + np.random.default_rng(seed).normal(0.0, sigma, rgb.shape)), 0, 255).astype(np.uint8)
    return list(P.boxed_payloads(FMT420, rgb))


def run(net, pay, h, w, **kw):
    vr = restore.VideoRestorer(net, ONE_LEN, **kw)
    out = list(vr.restore(iter(pay), yuv_fmt(*FMT420), h, w))
    return out, vr.stats


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def deblur():
    """The net, the boxed clip, and the reference computed once: the restorer on the cropped stream, pasted over the input."""
    net = restore.load_net("deblur_small", "synthetic", "bf16")
    pay = boxed_clip(edges=True)
    r, c = P.rowcol_ref(np.stack(pay), FMT420, H, W)
    assert picture.decide_picture(r, c, FMT420, H, W, 1.0) == RECT               # the clip: no row or column of the picture is dark in every frame
    crop = list(P.crop_payloads(np.stack(pay), FMT420, H, W, RECT))
    inner, stats = run(net, crop, RECT[3], RECT[2])
    assert stats["window_picture"] == [None] * 3 and stats["picture_launches"] == 0
    want = list(P.paste_payloads(np.stack(pay), np.stack(inner), FMT420, H, W, RECT))
    assert not same(want, pay)
    return net, pay, want


def test_a_fixed_picture_gives_the_cropped_streams_bytes_inside_and_the_inputs_outside(deblur):
    net, pay, want = deblur
    got, stats = run(net, pay, H, W, picture=RECT)
    assert same(got, want)                                                         # inside: the cropped stream's restoration; outside: the input
    assert stats["window_picture"] == [RECT] * 3 and stats["picture_launches"] == 0 and stats["frames"] == B["n"]
    serial, _ = run(net, pay, H, W, picture=RECT, pipeline=False)
    assert same(serial, got)
    full, stats = run(net, pay, H, W)                                              # the default restores the bars as well
    assert stats["window_picture"] == [None] * 3 and not same(full, got)


def test_auto_finds_the_rectangle_of_every_window_and_a_list_of_it_gives_the_same_bytes(deblur):
    net, pay, want = deblur
    for pipe in (True, False):
        got, stats = run(net, pay, H, W, picture="auto", pipeline=pipe)
        assert stats["window_picture"] == [RECT] * 3 and stats["picture_launches"] == stats["windows"] == 3
        assert same(got, want), pipe
    listed, stats = run(net, pay, H, W, picture=[RECT] * 3)
    assert same(listed, want) and stats["window_picture"] == [RECT] * 3 and stats["picture_launches"] == 0
    with pytest.raises(ValueError, match="window 2"):
        run(net, pay, H, W, picture=[RECT] * 2)
    with pytest.raises(ValueError, match="even"):
        run(net, pay, H, W, picture=(0, 11, 128, 72))
    with pytest.raises(ValueError, match="inside"):
        run(net, pay, H, W, picture=[(0, 12, 128, 96)])
    with pytest.raises(ValueError, match="smallest picture the restorer takes is 5 x 5"):        # deblur_small: the "small" topology
        run(net, pay, H, W, picture=(0, 12, 128, 4))
    with pytest.raises(ValueError, match="picture"):
        restore.VideoRestorer(net, ONE_LEN, picture="bars")


def test_a_leading_window_of_black_frames_is_restored_as_the_full_frame(deblur):
    net, pay, _ = deblur
    black = P.black_payload(FMT420, H, W)
    clip = [black] * 5 + pay[:6]                                                   # window 0 is fed frames 2 1 0 1 2 3 4: all black
    got, stats = run(net, clip, H, W, picture="auto")
    assert stats["window_picture"] == [None, RECT, RECT, RECT]
    full, _ = run(net, clip, H, W)
    assert same(got[:3], full[:3])                                                 # the bytes of picture=None for its frames
    listed, _ = run(net, clip, H, W, picture=[None, RECT, RECT, RECT])
    assert same(listed, got)
    for a, b in zip(got[3:], clip[3:]):                                            # the later windows leave the bars alone
        assert np.array_equal(P.paste_payloads(a[None], P.crop_payloads(b[None], FMT420, H, W, RECT), FMT420, H, W, RECT)[0], b)
    assert not same(got[5:], clip[5:])


def test_denoise_with_sigma_auto_estimates_on_the_rectangle():
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    pay = boxed_clip(sigma=10.0)
    crop = list(P.crop_payloads(np.stack(pay), FMT420, H, W, RECT))
    inner, want_stats = run(net, crop, RECT[3], RECT[2], sigma="auto")
    want = list(P.paste_payloads(np.stack(pay), np.stack(inner), FMT420, H, W, RECT))
    assert all(0.0 < s < 50.0 for s in want_stats["window_sigma"])
    for pic in (RECT, "auto"):
        got, stats = run(net, pay, H, W, sigma="auto", picture=pic)
        assert stats["window_sigma"] == want_stats["window_sigma"] and stats["window_frame_sigma"] == want_stats["window_frame_sigma"], pic
        assert stats["window_picture"] == [RECT] * 3 and same(got, want), pic
    got, stats = run(net, pay, H, W, sigma=list(want_stats["window_sigma"]), picture=RECT)           # sigma as a list
    assert same(got, want)
    got, _ = run(net, pay, H, W, sigma=10.0, picture=RECT)                         # and as a number
    inner10, _ = run(net, crop, RECT[3], RECT[2], sigma=10.0)
    assert same(got, list(P.paste_payloads(np.stack(pay), np.stack(inner10), FMT420, H, W, RECT)))


def test_listed_scene_cuts_are_honoured_inside_the_rectangle(deblur):
    net, pay, _ = deblur
    crop = list(P.crop_payloads(np.stack(pay), FMT420, H, W, RECT))
    inner, _ = run(net, crop, RECT[3], RECT[2], scene_cuts=[4])
    got, stats = run(net, pay, H, W, scene_cuts=[4], picture="auto")
    assert stats["cuts"] == [4] and stats["window_picture"] == [RECT] * len(stats["window_picture"])
    assert same(got, list(P.paste_payloads(np.stack(pay), np.stack(inner), FMT420, H, W, RECT)))


def test_the_smallest_picture_of_the_small_topology_is_restored_and_one_row_less_is_refused(deblur):
    net = deblur[0]
    h = w = 7                                                                      # (2, 2, 5, 5): odd w and h, legal because they reach the far edges
    rng = np.random.default_rng(9)
    pay = [rng.integers(16, 236, R.frame_bytes(FMT420, h, w), dtype=np.uint8) for _ in range(4)]
    rect = (2, 2, picture.smallest_picture(net.V.topo), picture.smallest_picture(net.V.topo))
    assert rect == (2, 2, 5, 5)
    inner, _ = run(net, list(P.crop_payloads(np.stack(pay), FMT420, h, w, rect)), 5, 5)
    got, stats = run(net, pay, h, w, picture=rect)
    assert stats["window_picture"] == [rect] * 2
    assert same(got, list(P.paste_payloads(np.stack(pay), np.stack(inner), FMT420, h, w, rect)))
    with pytest.raises(ValueError, match="smallest picture the restorer takes is 5 x 5"):
        run(net, pay, h, w, picture=(2, 2, 4, 5))


# ---- the command line -------------------------------------------------------------------------------------------------------------------------
def test_restore_video_cli_picture_auto_then_the_file_it_wrote_give_identical_files(tmp_path, deblur):
    _, pay, want = deblur
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, dst2, pic = tmp_path / "in.y4m", tmp_path / "out.y4m", tmp_path / "out2.y4m", tmp_path / "picture.txt"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    base = [sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "deblur_small", "--checkpoint", "synthetic",
            "--dtype", "bf16", "--one_len", str(ONE_LEN)]
    r = subprocess.run(base + ["--picture", "auto", "--picture_out", str(pic), str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "picture (auto)" in r.stderr and "0:12:128:72" in r.stderr
    assert picture.read_pictures(pic) == [RECT] * 3
    r = subprocess.run(base + ["--picture", str(pic), str(src), str(dst2)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "picture (listed)" in r.stderr
    assert dst.read_bytes() == dst2.read_bytes()
    with open(dst, "rb") as fh:
        assert same(list(y4m.Y4MReader(fh)), want)                                  # 96 < 720: the CLI's default matrix is BT.601, as FMT420
