"""-m gpu: the mixed egress (``sn_egress_yuv_mix``, csrc/sn_yuv.hip) against its numpy restatement (tests/mix_ref.py) bit for bit, and the video
restorer's ``amount`` and ``view="removed"`` against windows assembled by hand."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mix_ref as M
import picture_ref as P
import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import restore, y4m
from shiftnet_amd.io_edges import egress_yuv, ingest_yuv, yuv_fmt
from test_gpu_yuv import FMT420, FORMATS, IDS, clip_payloads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [("fp32", torch.float32), ("bf16", torch.bfloat16)]
# (H, W, Hp, Wp): the wide path; the element-wise path, odd sizes shift every plane; less than a lane's unit; a single sample
SIZES = [(64, 96, 64, 96), (67, 101, 72, 107), (2, 2, 8, 8), (1, 1, 4, 8)]
MIXES = [("amount", 0.5, 0.5), ("amount", 0.25, 1.0), ("amount", 1.0, 0.0), ("amount", 0.0, 0.0), ("removed", 1.0, 1.0), ("removed", 4.0, 2.0)]
DITHERS = [None, (0xDEADBEEF, 5)]                                 # none, and TPDF with t0 = 5
RECT_WIDE, RECT_ODD, RECT_EVEN = (16, 2, 64, 40), (2, 2, 61, 33), (2, 2, 62, 34)
GUARD = 64


def tensor(T, Hp, Wp, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(T, 3, Hp, Wp, generator=g) * 1.2 - 0.1                         # drawn from [-0.1, 1.1]: the clamp matters


def schedule(i):
    """The cases of format number i: six, one per mix, and across them every size, both T, both dtypes and both dithers; the pairing turns with i,
    so that the 24 formats together see most pairs."""
    return [(SIZES[(j + i) % 4], (1, 3)[(j + i) % 2], DTYPES[(j // 2 + i) % 2], MIXES[j], DITHERS[((j + 1) // 2 + i) % 2]) for j in range(6)]


def test_the_schedule_covers_every_value_of_every_axis_for_every_format():
    for i in range(len(FORMATS)):
        s = schedule(i)
        assert {c[0] for c in s} == set(SIZES) and {c[1] for c in s} == {1, 3} and {c[2][0] for c in s} == {"fp32", "bf16"}
        assert [c[3] for c in s] == MIXES and {c[4] for c in s} == set(DITHERS)


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(FORMATS)), ids=IDS)
def test_mixed_egress_equals_the_restatement_bit_for_bit_and_writes_nothing_else(i):
    fmt = FORMATS[i]
    f = yuv_fmt(*fmt)
    for (H, W, Hp, Wp), T, (name, dt), mix, dither in schedule(i):
        x = tensor(T, Hp, Wp, H * 1000 + W + T).to(dt)
        fb = R.frame_bytes(fmt, H, W)
        inp = M.random_payloads(fmt, T, H, W, seed=H + W + T + i)                     # the whole code range, illegal codes included
        buf = torch.full((T * fb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        got = egress_yuv(x.cuda(), f, H, W, dst=buf[GUARD:GUARD + T * fb].view(T, fb), dither=dither, mix=mix, ref=torch.from_numpy(inp).cuda())
        want = M.egress(x.float().numpy(), fmt, H, W, mix, inp, dither)
        assert np.array_equal(got.cpu().numpy(), want), (fmt, H, W, Hp, Wp, T, name, mix, dither)
        b = buf.cpu().numpy()
        assert (b[:GUARD] == 0xA5).all() and (b[GUARD + T * fb:] == 0xA5).all()
        if mix == ("amount", 0.0, 0.0):
            assert np.array_equal(want, inp)
    got = egress_yuv(torch.rand(2, 3, 16, 24).cuda(), f, 15, 23, mix=("removed", 1.0, 1.0),
                     ref=torch.from_numpy(M.random_payloads(fmt, 2, 15, 23, seed=1)).cuda())                      # allocating form
    assert got.shape == (2, R.frame_bytes(fmt, 15, 23)) and got.dtype == torch.uint8


@pytest.mark.parametrize("i", range(len(FORMATS)), ids=IDS)
def test_with_a_rectangle_the_inside_is_the_mix_with_the_streams_own_samples_and_the_outside_stays(i):
    """(16, 2, 64, 40) keeps the wide path, (2, 2, 61, 33) does not.  The second is a legal rectangle at 4:4:4 only -- at 4:2:0 an odd width or
    height must reach the frame's far edge -- so there it must be refused, and (2, 2, 62, 34) stands beside it as the element-wise case."""
    fmt = FORMATS[i]
    f = yuv_fmt(*fmt)
    H, W, T = 64, 96, (1, 3)[i % 2]
    fb = R.frame_bytes(fmt, H, W)
    inp = M.random_payloads(fmt, T, H, W, seed=50 + i)
    ref = torch.from_numpy(inp).cuda()
    pre = np.random.default_rng(i).integers(0, 256, T * fb + 2 * GUARD, dtype=np.uint8)
    rects = [RECT_WIDE] + ([RECT_ODD] if fmt.chroma == R.C444 else [RECT_EVEN])
    for n, rect in enumerate(rects):
        mix, dither, (name, dt) = MIXES[(i + 3 * n) % 6], DITHERS[(i // 2 + n) % 2], DTYPES[(i // 4 + n) % 2]
        h, w = rect[3], rect[2]
        x = tensor(T, (h + 3) // 4 * 4, (w + 7) // 8 * 8, 100 * h + w + i).to(dt)
        buf = torch.from_numpy(pre).cuda()
        dst = buf[GUARD:GUARD + T * fb].view(T, fb)
        assert egress_yuv(x.cuda(), f, H, W, dst=dst, rect=rect, dither=dither, mix=mix, ref=ref) is dst
        # the cropped stream: the input's samples under the rectangle, the dither's positions counted from its origin
        inner = M.egress(x.float().numpy(), fmt, h, w, mix, P.crop_payloads(inp, fmt, H, W, rect), dither)
        want = P.paste_payloads(pre[GUARD:GUARD + T * fb].reshape(T, fb), inner, fmt, H, W, rect)
        b = buf.cpu().numpy()
        assert np.array_equal(b[GUARD:GUARD + T * fb].reshape(T, fb), want), (fmt, rect, name, mix, dither)
        assert np.array_equal(b[:GUARD], pre[:GUARD]) and np.array_equal(b[GUARD + T * fb:], pre[GUARD + T * fb:])
    if fmt.chroma != R.C444:
        x = tensor(T, 36, 64, 1).cuda()
        dst = torch.from_numpy(pre[:T * fb].reshape(T, fb)).cuda()
        rc = L.load().sn_egress_yuv_mix(x.data_ptr(), L.SN_F32, f, L.YuvRect(*RECT_ODD), None, L.YuvMix(L.SN_MIX_AMOUNT, 0.5, 0.5), ref.data_ptr(),
                                        dst.data_ptr(), T, H, W, 36, 64, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == -22 and np.array_equal(dst.cpu().numpy().reshape(-1), pre[:T * fb])


@pytest.mark.parametrize("i", [0, 5, 10, 15, 20, 23], ids=[IDS[k] for k in (0, 5, 10, 15, 20, 23)])
def test_amount_zero_is_the_input_byte_for_byte_with_a_dither_given(i):
    fmt = FORMATS[i]
    f = yuv_fmt(*fmt)
    for (H, W, Hp, Wp) in SIZES[:2]:
        T = 3
        inp = torch.from_numpy(M.random_payloads(fmt, T, H, W, seed=9)).cuda()
        x = tensor(T, Hp, Wp, 3).cuda()
        got = egress_yuv(x, f, H, W, dither=(7, 5), mix=("amount", 0.0, 0.0), ref=inp)
        assert torch.equal(got, inp)
        luma = egress_yuv(x, f, H, W, dither=(7, 5), mix=("amount", 0.0, 1.0), ref=inp)       # luma untouched, chroma the dithered egress
        full = egress_yuv(x, f, H, W, dither=(7, 5), mix=("amount", 1.0, 1.0), ref=inp)
        ny = H * W * (1 if fmt.bits == 8 else 2)
        assert torch.equal(luma[:, :ny], inp[:, :ny]) and torch.equal(luma[:, ny:], full[:, ny:]) and not torch.equal(luma, inp)


def test_bad_arguments_return_einval_and_leave_dst_untouched():
    lib = L.load()
    f420, f10 = yuv_fmt(8, L.SN_YUV_420_CENTER, 0, 0), yuv_fmt(10, L.SN_YUV_444, 0, 0)
    H, W = 24, 40
    x = torch.full((1, 3, H, W), 0.5, device="cuda")
    big = 4 * H * W * 2 + 2
    dst = torch.full((big,), 0xA5, dtype=torch.uint8, device="cuda")
    ref = torch.full((big,), 0x40, dtype=torch.uint8, device="cuda")
    ok, tp, rect = L.YuvMix(L.SN_MIX_AMOUNT, 0.5, 1.0), L.YuvDither(L.SN_DITHER_TPDF, 1, 0), L.YuvRect(6, 4, 26, 16)
    s = torch.cuda.current_stream().cuda_stream
    nan, inf = float("nan"), float("inf")
    ptr = lambda a: a if isinstance(a, (int, type(None))) else a.data_ptr()      # noqa: E731
    fb = H * W * 3 // 2

    def go(fmt=f420, r=None, d=None, m=ok, out=x, src=ref, to=dst, T=1, h=H, w=W, hp=H, wp=W, dt=L.SN_F32):
        return lib.sn_egress_yuv_mix(ptr(out), dt, fmt, r, d, m, ptr(src), ptr(to), T, h, w, hp, wp, s)
    bad = [go(m=None), go(src=None), go(m=L.YuvMix(2, 0.5, 0.5)), go(m=L.YuvMix(-1, 0.5, 0.5)),
           go(m=L.YuvMix(L.SN_MIX_AMOUNT, nan, 0.5)), go(m=L.YuvMix(L.SN_MIX_AMOUNT, 0.5, inf)), go(m=L.YuvMix(L.SN_MIX_REMOVED, nan, 1.0)),
           go(m=L.YuvMix(L.SN_MIX_REMOVED, 1.0, -inf)), go(m=L.YuvMix(L.SN_MIX_AMOUNT, -0.01, 0.5)), go(m=L.YuvMix(L.SN_MIX_AMOUNT, 0.5, 1.01)),
           go(fmt=f10, src=ref.data_ptr() + 1),                                                # 16-bit samples of `in` at an odd address
           go(src=dst), go(src=dst.data_ptr() + fb - 1), go(src=dst.data_ptr() - fb + 1),      # overlapping byte ranges
           go(T=2, src=dst.data_ptr() + fb),                                                   # ... of T payloads
           # everything sn_egress_yuv_dither refuses, a null dither apart
           go(d=L.YuvDither(2, 1, 0)), go(d=L.YuvDither(-1, 1, 0)), go(d=L.YuvDither(L.SN_DITHER_TPDF, 1, -1)), go(d=L.YuvDither(L.SN_DITHER_NONE, 1, -1)),
           go(out=None), go(to=None), go(fmt=None), go(fmt=yuv_fmt(9, 0, 0, 0)), go(fmt=yuv_fmt(8, 3, 0, 0)), go(dt=3), go(T=0), go(h=0), go(w=0),
           go(hp=H - 1), go(wp=W - 1), go(fmt=f10, to=dst.data_ptr() + 1),
           go(r=L.YuvRect(5, 4, 26, 16)), go(r=L.YuvRect(6, 4, 25, 16)), go(r=L.YuvRect(6, 4, 36, 16)), go(r=rect, hp=12)]
    torch.cuda.synchronize()
    assert bad == [-22] * len(bad), bad
    assert bool((dst == 0xA5).all()) and bool((ref == 0x40).all())                   # nothing was launched
    good = [go(), go(d=tp), go(r=rect), go(r=rect, d=tp), go(d=L.YuvDither(L.SN_DITHER_NONE, 9, 3)), go(m=L.YuvMix(L.SN_MIX_REMOVED, 100.0, 0.0)),
            go(m=L.YuvMix(L.SN_MIX_REMOVED, -1.0, 1.0)), go(m=L.YuvMix(L.SN_MIX_AMOUNT, 0.0, 1.0)),
            go(src=dst.data_ptr() + fb), go(src=dst.data_ptr() + 2 * fb, to=dst.data_ptr() + fb)]      # ranges that touch without overlapping
    torch.cuda.synchronize()
    assert good == [0] * len(good), good
    f, xx = f420, x[0:1]
    for kw in (dict(mix=("amount", 0.5, 0.5)), dict(ref=ref[:fb].view(1, fb))):
        with pytest.raises(ValueError, match="mix and ref"):
            egress_yuv(xx, f, H, W, **kw)
    for mix in (("amount", 1.5, 0.5), ("amount", 0.5, nan), ("removed", inf, 1.0), ("blend", 0.5, 0.5), ("amount", 0.5), "amount", (0, 0.5, 0.5)):
        with pytest.raises(ValueError, match="mix"):
            egress_yuv(xx, f, H, W, mix=mix, ref=ref[:fb].view(1, fb))


# ---- the restorer ---------------------------------------------------------------------------------------------------------------------------
N, HH, WW, ONE_LEN, SIGMA = 11, 70, 98, 4, 10.0                   # the clip of tests/test_gpu_yuv.py's restorer test
RECT = (8, 4, 64, 48)
_CLIPS = {}


def windows_by_hand(net, payloads, h, w):
    """The float32 result of every window of the clip: [(first frame, [n,3,hp,wp] numpy)], reflected about the clip's ends as the restorer does."""
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
        x, x32 = ingest_yuv(dev, f, h, w, hp, wp, dt), ingest_yuv(dev, f, h, w, hp, wp, torch.float32)
        with torch.no_grad():
            if net.V.denoise:
                nm = torch.full((1, 1, 1, 1, 1), SIGMA / 255.0, dtype=dt, device="cuda").expand(1, len(idx), 1, hp, wp)
                y = net.forward_fp32_out(x, nm, shortcut=x32)
            else:
                y = net.forward_fp32_out(x, shortcut=x32)
        assert tuple(y.shape) == (hi - lo, 3, hp, wp) and y.dtype == torch.float32
        out.append((lo, y.cpu().numpy()))
    return out


def get_clip(variant):
    """The net, the 11-frame 98 x 70 4:2:0 8-bit clip and the float32 windows of the whole clip, computed once per variant."""
    if variant not in _CLIPS:
        net = restore.load_net(variant, "synthetic", "bf16")
        pay = list(clip_payloads(N, HH, WW))
        _CLIPS[variant] = (variant, net, pay, windows_by_hand(net, pay, HH, WW))
    return _CLIPS[variant]


@pytest.fixture(scope="module", params=["deblur_small", "denoise_small"])
def clip(request):
    return get_clip(request.param)


def make(net, **kw):
    if net.V.denoise:
        kw.setdefault("sigma", SIGMA)
    return restore.VideoRestorer(net, ONE_LEN, **kw)


def run(net, pay, **kw):
    vr = make(net, **kw)
    return list(vr.restore(iter(pay), yuv_fmt(*FMT420), HH, WW)), vr.stats


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def mixed(wins, fmt, mix, inp, dither_seed=None):
    return [p for lo, y in wins for p in M.egress(y, fmt, HH, WW, mix, np.stack(inp[lo:lo + len(y)]), None if dither_seed is None else (dither_seed, lo))]


def test_amount_one_takes_todays_path_and_gives_the_bytes_of_no_amount(clip):
    _, net, pay, wins = clip
    default, stats = run(net, pay)
    assert stats["amount"] is None and stats["view"] is None
    assert same(default, [p for _, y in wins for p in R.egress_emu(y, FMT420, HH, WW)])
    for amount in (1.0, (1.0, 1.0)):
        vr = make(net, amount=amount)
        assert vr.mix is None
        assert same(list(vr.restore(iter(pay), yuv_fmt(*FMT420), HH, WW)), default)
        assert vr.stats["amount"] == (1.0, 1.0) and vr.stats["view"] is None and vr.slots[0].dev_ref is None


def test_amount_zero_returns_every_input_frame_byte_for_byte(clip):
    _, net, pay, _ = clip
    for kw in (dict(), dict(pipeline=False), dict(scene_cuts=[5]), dict(picture=RECT), dict(dither="tpdf", dither_seed=3)):
        got, stats = run(net, pay, amount=0.0, **kw)
        assert same(got, pay), kw
        assert stats["amount"] == (0.0, 0.0) and stats["frames"] == N
    assert not same(run(net, pay, picture=RECT)[0], pay)


def test_amounts_and_the_removed_view_equal_hand_assembled_windows_pushed_through_the_restatement(clip):
    _, net, pay, wins = clip
    for kw, mix in ((dict(amount=(0.5, 1.0)), ("amount", 0.5, 1.0)), (dict(view="removed"), ("removed", 1.0, 1.0)),
                    (dict(view="removed", removed_gain=4.0, amount=1.0), ("removed", 4.0, 4.0))):
        want = mixed(wins, FMT420, mix, pay)
        got, stats = run(net, pay, **kw)
        assert same(got, want), kw
        assert stats["amount"] == ((0.5, 1.0) if "amount" in kw and kw["amount"] != 1.0 else ((1.0, 1.0) if "amount" in kw else None))
        assert stats["view"] == kw.get("view")
        assert same(run(net, pay, pipeline=False, **kw)[0], want), kw
    noisy, _ = run(net, pay, amount=(0.5, 1.0), dither="tpdf", dither_seed=3)         # the dither's frame number counts from the clip's first frame
    assert same(noisy, mixed(wins, FMT420, ("amount", 0.5, 1.0), pay, dither_seed=3))
    plain = [p for _, y in wins for p in R.egress_emu(y, FMT420, HH, WW)]
    assert not same(want, plain) and not same(mixed(wins, FMT420, ("amount", 0.5, 1.0), pay), plain)


def test_with_a_picture_the_outside_stays_the_inputs_in_either_view(clip):
    _, net, pay, _ = clip
    crop = list(P.crop_payloads(np.stack(pay), FMT420, HH, WW, RECT))
    for kw in (dict(amount=0.5), dict(view="removed", removed_gain=2.0)):
        vr = make(net, **kw)
        inner = list(vr.restore(iter(crop), yuv_fmt(*FMT420), RECT[3], RECT[2]))       # the cropped stream, mixed with its own input
        want = list(P.paste_payloads(np.stack(pay), np.stack(inner), FMT420, HH, WW, RECT))
        got, stats = run(net, pay, picture=RECT, **kw)
        assert stats["window_picture"] == [RECT] * 3
        assert same(got, want), kw


def test_another_output_format_mixes_with_the_converted_input(clip):
    _, net, pay, wins = clip
    tag = "444p10"
    ofmt = R.Fmt(*y4m.MODES[tag], FMT420.matrix, FMT420.range)
    conv = R.egress_emu(R.ingest_emu(np.stack(pay), FMT420, HH, WW, HH, WW, "fp32"), ofmt, HH, WW)    # ingest float32 -> egress(ofmt), undithered
    want = mixed(wins, ofmt, ("amount", 0.5, 0.5), list(conv))
    vr = make(net, amount=0.5, out_format=tag)
    got = list(vr.restore(iter(pay), yuv_fmt(*FMT420), HH, WW))
    assert all(p.shape == (R.frame_bytes(ofmt, HH, WW),) for p in got)
    assert same(got, want)
    assert vr.stats["out_format"] == tag and vr.stats["amount"] == (0.5, 0.5)
    assert all(s.dev_ref is not None and s.dev_ref.data_ptr() != s.dev_out.data_ptr() for s in vr.slots)
    assert same(run(net, pay, amount=0.5, out_format=tag, pipeline=False)[0], want)
    assert same(run(net, pay, amount=0.0, out_format=tag)[0], list(conv))             # amount 0: the converted input
    assert make(net, out_format=tag).mix is None


def test_a_second_restore_on_the_same_object_starts_clean(clip):
    _, net, pay, wins = clip
    vr = make(net, amount=(0.5, 1.0))
    f = yuv_fmt(*FMT420)
    first = list(vr.restore(iter(pay), f, HH, WW))
    s1 = dict(vr.stats)
    second = list(vr.restore(iter(pay[:6]), f, HH, WW))
    assert same(first, mixed(wins, FMT420, ("amount", 0.5, 1.0), pay))
    assert same(second, run(net, pay[:6], amount=(0.5, 1.0))[0])
    assert s1["frames"] == N and s1["windows"] == 3 and vr.stats["frames"] == 6 and vr.stats["windows"] == 2
    assert vr.stats["amount"] == (0.5, 1.0) and vr.stats["view"] is None and len(vr.stats["window_picture"]) == 2


def test_argument_errors_of_the_restorer(clip):
    _, net, _, _ = clip
    for kw, word in ((dict(amount=1.5), "amount"), (dict(amount=float("nan")), "amount"), (dict(amount=(0.5, 0.5, 0.5)), "amount"),
                     (dict(view="added"), "view"), (dict(amount=0.5, view="removed"), "view='removed'"), (dict(view="removed", removed_gain=-1), "removed_gain")):
        with pytest.raises(ValueError, match=word):
            make(net, **kw)


def test_restore_video_cli_with_an_amount_gives_the_api_bytes(tmp_path):
    variant, net, pay, wins = get_clip("deblur_small")
    hd = y4m.Y4MHeader(width=WW, height=HH, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", variant, "--checkpoint", "synthetic", "--dtype", "bf16",
                        "--one_len", str(ONE_LEN), "--amount", "0.5,1", str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "amount: luma 0.5, chroma 1" in r.stderr and f"done: {N} frames" in r.stderr
    with open(dst, "rb") as fh:
        rd = y4m.Y4MReader(fh)
        got = list(rd)
    assert rd.header.line() == hd.line()
    api, _ = run(net, pay, amount=(0.5, 1.0))                                        # 70 < 720: the CLI's default matrix is BT.601, as FMT420
    assert same(got, api) and same(api, mixed(wins, FMT420, ("amount", 0.5, 1.0), pay))
