"""-m gpu: the dithered egress (``sn_egress_yuv_dither``, csrc/sn_yuv.hip) against its numpy restatement (tests/dither_ref.py) bit for bit, and
the video restorer writing another format than it read, dithered or not, against windows assembled by hand."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dither_ref as D
import picture_ref as P
import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import restore, y4m
from shiftnet_amd.io_edges import egress_yuv, ingest_yuv, yuv_fmt
from test_gpu_yuv import FMT420, clip_payloads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {"8bit-444": (8, R.C444), "8bit-420c": (8, R.C420_CENTER), "8bit-420l": (8, R.C420_LEFT), "10bit-444": (10, R.C444), "10bit-420l": (10, R.C420_LEFT)}
FORMATS = {f"{k}-{'709' if m else '601'}-{'full' if r else 'lim'}": R.Fmt(*v, m, r) for k, v in LAYOUTS.items() for m in (R.BT601, R.BT709)
           for r in (R.LIMITED, R.FULL)}
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
# (H, W, Hp, Wp): a single sample; less than a lane's 8 x 2 unit; an odd size; all lanes on the wide path; a wide interior with an element-wise
# edge and odd sizes; two workgroups along x (a workgroup covers 256 columns)
SIZES = [(1, 1, 4, 4), (2, 7, 4, 8), (3, 9, 4, 12), (16, 64, 16, 64), (35, 67, 40, 72), (17, 264, 24, 264)]
RUNS = [(1, 0, 0), (3, 5, 0xDEADBEEF), (1, 5, 0xDEADBEEF), (3, 0, 0)]                 # (T, t0, seed): T in {1, 3} x t0 in {0, 5}, two seeds
GUARD = 64


def tensor(T, Hp, Wp, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(T, 3, Hp, Wp, generator=g) * 1.4 - 0.2                         # values below 0 and above 1: the clamp matters


def call(lib, x, fmt, rect, dither, dst, T, H, W):
    return lib.sn_egress_yuv_dither(x.data_ptr(), L.SN_F32 if x.dtype == torch.float32 else (L.SN_F16 if x.dtype == torch.float16 else L.SN_BF16), fmt, rect,
                                    dither, dst.data_ptr(), T, H, W, x.shape[2], x.shape[3], torch.cuda.current_stream().cuda_stream)


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FORMATS.values()), ids=list(FORMATS))
def test_dithered_egress_equals_the_restatement_bit_for_bit_and_writes_nothing_else(fmt):
    f = yuv_fmt(*fmt)
    for (H, W, Hp, Wp), (T, t0, seed) in [(s, r) for s in SIZES for r in RUNS]:
        x32 = tensor(T, Hp, Wp, H * 1000 + W + T)
        fb = R.frame_bytes(fmt, H, W)
        for name, dt in DTYPES.items():
            x = x32.to(dt)
            buf = torch.full((T * fb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            got = egress_yuv(x.cuda(), f, H, W, dst=buf[GUARD:GUARD + T * fb].view(T, fb), dither=(seed, t0))
            want = D.egress(x.float().numpy(), fmt, H, W, seed, t0)
            assert np.array_equal(got.cpu().numpy(), want), (fmt, H, W, Hp, Wp, T, t0, seed, name)
            b = buf.cpu().numpy()
            assert (b[:GUARD] == 0xA5).all() and (b[GUARD + T * fb:] == 0xA5).all()
    assert not np.array_equal(want, R.egress_emu(x.float().numpy(), fmt, H, W))       # the last case: the dither changes bytes
    got = egress_yuv(torch.rand(2, 3, 16, 24).cuda(), f, 15, 23, dither=(1, 0))       # allocating form
    assert got.shape == (2, R.frame_bytes(fmt, 15, 23)) and got.dtype == torch.uint8


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_mode_none_gives_the_bytes_of_the_entry_points_without_dither(layout):
    fmt = R.Fmt(*LAYOUTS[layout], R.BT709, R.LIMITED)
    f, lib = yuv_fmt(*fmt), L.load()
    H, W, Hp, Wp, T = 35, 67, 40, 72, 3
    x = tensor(T, Hp, Wp, 11).cuda()
    fb = R.frame_bytes(fmt, H, W)
    none = L.YuvDither(L.SN_DITHER_NONE, 123, 7)                                     # seed and t0 are not looked at
    dst = torch.full((T, fb), 0xA5, dtype=torch.uint8, device="cuda")
    assert call(lib, x, f, None, none, dst, T, H, W) == 0
    assert torch.equal(dst, egress_yuv(x, f, H, W))
    rect = (6, 4, 26, 16)
    pre = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (T, fb), dtype=np.uint8)).cuda()
    a, b = pre.clone(), pre.clone()
    assert call(lib, x, f, L.YuvRect(*rect), none, a, T, H, W) == 0
    assert torch.equal(a, egress_yuv(x, f, H, W, dst=b, rect=rect)) and not torch.equal(a, pre)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_one_launch_of_four_frames_equals_two_launches_of_two_at_their_frame_numbers(layout):
    fmt = R.Fmt(*LAYOUTS[layout], R.BT601, R.FULL)
    f = yuv_fmt(*fmt)
    H, W, Hp, Wp = 35, 67, 40, 72
    x = tensor(4, Hp, Wp, 12).cuda()
    one = egress_yuv(x, f, H, W, dither=(77, 0))
    two = torch.cat([egress_yuv(x[:2].contiguous(), f, H, W, dither=(77, 0)), egress_yuv(x[2:].contiguous(), f, H, W, dither=(77, 2))])
    assert torch.equal(one, two)
    assert not torch.equal(one[2:], egress_yuv(x[2:].contiguous(), f, H, W, dither=(77, 0)))      # the frame number matters
    assert not torch.equal(one, egress_yuv(x, f, H, W, dither=(78, 0)))                           # and the seed


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_with_a_rectangle_the_inside_is_the_dithered_egress_of_the_cropped_tensor_and_the_outside_stays(layout):
    fmt = R.Fmt(*LAYOUTS[layout], R.BT601, R.LIMITED)
    f = yuv_fmt(*fmt)
    H, W, T, seed, t0 = 24, 40, 3, 5, 2
    fb = R.frame_bytes(fmt, H, W)
    for rect in [(6, 4, 26, 16), (6, 4, 34, 20), (0, 0, 40, 24)]:                    # inside; odd-free and reaching both far edges; the whole frame
        for Hp, Wp in ((rect[3] + 3) // 4 * 4, (rect[2] + 3) // 4 * 4), ((rect[3] + 7) // 8 * 8, (rect[2] + 7) // 8 * 8):
            x32 = tensor(T, Hp, Wp, Hp * 100 + Wp)
            pre = np.random.default_rng(rect[2]).integers(0, 256, T * fb + 2 * GUARD, dtype=np.uint8)
            for name, dt in DTYPES.items():
                x = x32.to(dt)
                buf = torch.from_numpy(pre).cuda()
                dst = buf[GUARD:GUARD + T * fb].view(T, fb)
                assert egress_yuv(x.cuda(), f, H, W, dst=dst, rect=rect, dither=(seed, t0)) is dst
                inner = D.egress(x.float().numpy(), fmt, rect[3], rect[2], seed, t0)             # the cropped stream: positions count from the rectangle's origin
                want = P.paste_payloads(pre[GUARD:GUARD + T * fb].reshape(T, fb), inner, fmt, H, W, rect)
                b = buf.cpu().numpy()
                assert np.array_equal(b[GUARD:GUARD + T * fb].reshape(T, fb), want), (fmt, rect, Hp, Wp, name)
                assert np.array_equal(b[:GUARD], pre[:GUARD]) and np.array_equal(b[GUARD + T * fb:], pre[GUARD + T * fb:])


def test_bad_arguments_return_einval_and_launch_nothing():
    lib = L.load()
    f420, f10 = yuv_fmt(8, L.SN_YUV_420_CENTER, 0, 0), yuv_fmt(10, L.SN_YUV_444, 0, 0)
    H, W = 24, 40
    x = torch.full((1, 3, H, W), 0.5, device="cuda")
    dst = torch.full((4 * H * W * 2 + 2,), 0xA5, dtype=torch.uint8, device="cuda")
    ok, rect = L.YuvDither(L.SN_DITHER_TPDF, 1, 0), L.YuvRect(6, 4, 26, 16)
    s = torch.cuda.current_stream().cuda_stream

    def go(fmt=f420, r=None, d=ok, out=x, to=dst, T=1, h=H, w=W, hp=H, wp=W, dt=L.SN_F32):
        return lib.sn_egress_yuv_dither(out.data_ptr() if out is not None else None, dt, fmt, r, d, to if isinstance(to, (int, type(None))) else to.data_ptr(),
                                        T, h, w, hp, wp, s)
    bad = [go(d=None), go(d=L.YuvDither(2, 1, 0)), go(d=L.YuvDither(-1, 1, 0)), go(d=L.YuvDither(L.SN_DITHER_TPDF, 1, -1)),
           go(d=L.YuvDither(L.SN_DITHER_NONE, 1, -1)), go(r=rect, d=None),
           go(out=None), go(to=None), go(fmt=None), go(fmt=yuv_fmt(9, 0, 0, 0)), go(fmt=yuv_fmt(8, 3, 0, 0)), go(dt=3), go(T=0), go(h=0), go(w=0),
           go(hp=H - 1), go(wp=W - 1), go(fmt=f10, to=dst.data_ptr() + 1),                     # 16-bit samples at an odd address
           go(r=L.YuvRect(5, 4, 26, 16)), go(r=L.YuvRect(6, 4, 25, 16)), go(r=L.YuvRect(6, 4, 36, 16)), go(r=rect, hp=12)]
    torch.cuda.synchronize()
    assert bad == [-22] * len(bad), bad
    assert bool((dst == 0xA5).all())                                                 # nothing was launched
    assert go() == 0 and go(r=rect) == 0 and go(d=L.YuvDither(L.SN_DITHER_TPDF, 2 ** 32 - 1, 2 ** 31 - 2)) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="dither"):
        egress_yuv(x[0:1].view(1, 3, H, W), f420, H, W, dither=(2 ** 32, 0))
    with pytest.raises(ValueError, match="dither"):
        egress_yuv(x[0:1].view(1, 3, H, W), f420, H, W, dither=(0, -1))


# ---- the restorer ---------------------------------------------------------------------------------------------------------------------------
N, HH, WW, ONE_LEN, SEED = 12, 40, 48, 4, 3
OUT_TAGS = ("444p10", "420p10", "420jpeg")


def out_fmt(tag):
    return R.Fmt(*y4m.MODES[tag], FMT420.matrix, FMT420.range)


def run(net, pay, h=HH, w=WW, **kw):
    if net.V.denoise:
        kw.setdefault("sigma", 10.0)
    vr = restore.VideoRestorer(net, ONE_LEN, **kw)
    out = list(vr.restore(iter(pay), yuv_fmt(*FMT420), h, w))
    return out, vr.stats


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def forward_windows(net, payloads, h, w):
    """The float32 result of every window, assembled here as tests/test_gpu_yuv.py's by_hand does: (first frame, [n,3,hp,wp] on the device)."""
    f = yuv_fmt(*FMT420)
    dt = next(net.parameters()).dtype
    hp, wp = restore.padded_size(h, w, net.V.topo)
    n = len(payloads)
    refl = lambda i: -i if i < 0 else (2 * (n - 1) - i if i >= n else i)      # noqa: E731
    out = []
    for lo in range(0, n, ONE_LEN):
        hi = min(lo + ONE_LEN, n)
        idx = [refl(i) for i in range(lo - 2, hi + 2)]
        dev = torch.from_numpy(np.stack([payloads[i] for i in idx])).cuda()
        x = ingest_yuv(dev, f, h, w, hp, wp, dt)
        x32 = ingest_yuv(dev, f, h, w, hp, wp, torch.float32)
        with torch.no_grad():
            if net.V.denoise:
                nm = torch.full((1, 1, 1, 1, 1), 10.0 / 255.0, dtype=dt, device="cuda").expand(1, len(idx), 1, hp, wp)
                y = net.forward_fp32_out(x, nm, shortcut=x32)
            else:
                y = net.forward_fp32_out(x, shortcut=x32)
        assert tuple(y.shape) == (hi - lo, 3, hp, wp) and y.dtype == torch.float32
        out.append((lo, y.clone()))
    return out


@pytest.fixture(scope="module", params=["deblur_small", "denoise_small"])
def clip(request):
    """The net, the 12-frame 48 x 40 4:2:0 8-bit clip, and the float32 windows of the whole clip computed once."""
    net = restore.load_net(request.param, "synthetic", "bf16")
    pay = list(clip_payloads(N, HH, WW, seed=11))
    return request.param, net, pay, forward_windows(net, pay, HH, WW)


def test_every_output_format_equals_hand_assembled_windows_dithered_or_not_pipelined_or_not(clip):
    _, net, pay, wins = clip
    for tag in OUT_TAGS:
        ofmt = out_fmt(tag)
        plain = [p for _, y in wins for p in egress_yuv(y, yuv_fmt(*ofmt), HH, WW).cpu().numpy()]
        got, stats = run(net, pay, out_format=tag)
        assert all(p.shape == (R.frame_bytes(ofmt, HH, WW),) and p.dtype == np.uint8 for p in got)
        assert same(got, plain), tag
        assert stats["out_format"] == (None if tag == "420jpeg" else tag) and stats["dither"] is None and stats["frames"] == N
        assert same(run(net, pay, out_format=tag, pipeline=False)[0], plain), tag
        noisy = [p for lo, y in wins for p in D.egress(y.cpu().numpy(), ofmt, HH, WW, SEED, lo)]  # the frame number counts from the clip's first frame
        assert not same(noisy, plain)
        got, stats = run(net, pay, out_format=tag, dither="tpdf", dither_seed=SEED)
        assert same(got, noisy), tag
        assert stats["dither"] == "tpdf" and stats["dither_seed"] == SEED
        assert same(run(net, pay, out_format=tag, dither="tpdf", dither_seed=SEED, pipeline=False)[0], noisy), tag
    other, _ = run(net, pay, out_format="444p10", dither="tpdf", dither_seed=SEED + 1)
    assert not same(other, run(net, pay, out_format="444p10", dither="tpdf", dither_seed=SEED)[0])


def test_the_defaults_give_the_bytes_of_the_inputs_own_format_without_dither(clip):
    _, net, pay, wins = clip
    default, stats = run(net, pay)
    assert stats["out_format"] is None and stats["dither"] is None
    assert same(default, run(net, pay, out_format="420jpeg", dither=None)[0])
    assert same(default, [p for _, y in wins for p in egress_yuv(y, yuv_fmt(*FMT420), HH, WW).cpu().numpy()])
    assert all(p.shape == (R.frame_bytes(FMT420, HH, WW),) for p in default)
    noisy, _ = run(net, pay, dither="tpdf", dither_seed=SEED)                         # dither without another format: 8 bit out, dithered
    assert same(noisy, [p for lo, y in wins for p in D.egress(y.cpu().numpy(), FMT420, HH, WW, SEED, lo)])


def test_scene_cuts_with_dither_equal_restoring_the_scenes_as_two_videos(clip):
    _, net, pay, _ = clip
    kw = dict(out_format="444p10", dither="tpdf", dither_seed=SEED)
    got, stats = run(net, pay, scene_cuts=[5], **kw)
    assert stats["cuts"] == [5]
    want = run(net, pay[:5], **kw)[0] + run(net, pay[5:], **kw)[0]
    assert same(got, want)
    assert same(run(net, pay, scene_cuts=[5], pipeline=False, **kw)[0], want)
    assert not same(got, run(net, pay, **kw)[0])


def test_a_picture_in_another_format_is_the_cropped_streams_bytes_inside_and_the_converted_input_outside(clip):
    _, net, pay, _ = clip
    rect, tag = (8, 4, 32, 32), "444p10"
    ofmt = out_fmt(tag)
    crop = list(P.crop_payloads(np.stack(pay), FMT420, HH, WW, rect))
    rgb = R.ingest_emu(np.stack(pay), FMT420, HH, WW, HH, WW, "fp32")                # the outside: ingest to float32, egress in the output format
    outside = R.egress_emu(rgb, ofmt, HH, WW)
    for kw in (dict(), dict(dither="tpdf", dither_seed=SEED)):
        inner, _ = run(net, crop, rect[3], rect[2], out_format=tag, **kw)
        want = list(P.paste_payloads(outside, np.stack(inner), ofmt, HH, WW, rect))
        got, stats = run(net, pay, picture=rect, out_format=tag, **kw)
        assert stats["window_picture"] == [rect] * 3
        assert same(got, want), kw
        assert same(run(net, pay, picture=rect, out_format=tag, pipeline=False, **kw)[0], want), kw
        assert same(run(net, pay, picture=[rect] * 3, out_format=tag, **kw)[0], want), kw
    black = P.black_payload(FMT420, HH, WW)                                          # a bar at code 16 leaves at code 64, its chroma at 512
    Y, U, V = R.split_planes(R.egress_emu(R.ingest_emu(black[None], FMT420, HH, WW, HH, WW, "fp32"), ofmt, HH, WW)[0], ofmt, HH, WW)
    assert (Y == 64).all() and (U == 512).all() and (V == 512).all()
    with pytest.raises(ValueError, match="even"):                                    # legal at 4:4:4 out, not at 4:2:0 in
        run(net, pay, picture=(9, 4, 32, 32), out_format=tag)
    same_fmt, _ = run(net, pay, picture=rect, dither="tpdf", dither_seed=SEED)       # equal formats: the outside is the input's bytes, copied
    inner, _ = run(net, crop, rect[3], rect[2], dither="tpdf", dither_seed=SEED)
    assert same(same_fmt, list(P.paste_payloads(np.stack(pay), np.stack(inner), FMT420, HH, WW, rect)))


def test_argument_errors_of_the_restorer(clip):
    _, net, _, _ = clip
    sig = {"sigma": 10.0} if net.V.denoise else {}
    with pytest.raises(ValueError, match="out_format"):
        restore.VideoRestorer(net, ONE_LEN, out_format="422", **sig)
    with pytest.raises(ValueError, match="dither"):
        restore.VideoRestorer(net, ONE_LEN, dither="floyd", **sig)
    with pytest.raises(ValueError, match="dither_seed"):
        restore.VideoRestorer(net, ONE_LEN, dither="tpdf", dither_seed=-1, **sig)


def test_restore_video_cli_writes_the_new_c_tag_and_the_api_bytes(tmp_path, clip):
    variant, net, pay, _ = clip
    hd = y4m.Y4MHeader(width=WW, height=HH, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED", "YSCSS=420JPEG"])
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", variant, "--checkpoint", "synthetic", "--dtype", "bf16",
                        "--one_len", str(ONE_LEN), "--out_format", "444p10", "--dither", "tpdf", "--dither_seed", "3"]
                       + (["--sigma", "10"] if "denoise" in variant else []) + [str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "output: C444p10, dither tpdf seed 3" in r.stderr and f"done: {N} frames" in r.stderr
    with open(dst, "rb") as fh:
        rd = y4m.Y4MReader(fh)
        got = list(rd)
    assert rd.header.line() == b"YUV4MPEG2 W48 H40 F24:1 Ip A1:1 C444p10 XCOLORRANGE=LIMITED XYSCSS=420JPEG\n"
    api, _ = run(net, pay, out_format="444p10", dither="tpdf", dither_seed=3)       # 40 < 720: the CLI's default matrix is BT.601, as FMT420
    assert same(got, api)
