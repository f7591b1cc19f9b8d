"""-m gpu: the Y'CbCr edges (csrc/sn_yuv.hip) against their float32 restatement (tests/yuv_ref.py) bit for bit, and the video restorer
(shiftnet_amd/restore.py, inference/restore_video.py) against windows assembled by hand."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import restore, synth, y4m
from shiftnet_amd.io_edges import egress_yuv, ingest_yuv, yuv_fmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = [R.Fmt(b, c, m, r) for b in (8, 10) for c in (R.C444, R.C420_CENTER, R.C420_LEFT) for m in (R.BT601, R.BT709) for r in (R.LIMITED, R.FULL)]
IDS = [f"{f.bits}bit-{('444', '420c', '420l')[f.chroma]}-{'709' if f.matrix else '601'}-{'full' if f.range else 'lim'}" for f in FORMATS]
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
# (H, W, Hp, Wp): sizes equal to and larger than the frame; Wp % 8 == 0 takes the wide stores, the others the element-wise ones
SIZES = [(64, 96, 64, 96), (64, 96, 72, 104), (67, 101, 67, 101), (67, 101, 68, 104), (67, 101, 72, 107), (2, 2, 2, 2), (2, 2, 8, 8), (1, 1, 1, 1), (1, 1, 4, 8)]


def random_payloads(fmt, T, H, W, seed):
    rng = np.random.default_rng(seed)
    n = R.frame_bytes(fmt, H, W)
    if fmt.bits == 8:
        return rng.integers(0, 256, (T, n), dtype=np.uint8)
    return rng.integers(0, 1024, (T, n // 2)).astype("<u2").view(np.uint8).reshape(T, n)


def stored(t: torch.Tensor, name: str) -> np.ndarray:
    """The stored elements of a tensor in the form yuv_ref.to_dtype_bits gives."""
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if name == "bf16" else t.numpy()


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_ingest_yuv_equals_the_float32_restatement_bit_for_bit(fmt):
    f = yuv_fmt(*fmt)
    for (H, W, Hp, Wp), T in [(s, t) for s in SIZES for t in (1, 5)]:
        p = random_payloads(fmt, T, H, W, seed=H * 1000 + W + T)
        dev = torch.from_numpy(p).cuda()
        for name, dt in DTYPES.items():
            got = ingest_yuv(dev, f, H, W, Hp, Wp, dt)
            assert got.shape == (1, T, 3, Hp, Wp) and got.dtype == dt
            want = R.ingest_emu(p, fmt, H, W, Hp, Wp, name)
            g = stored(got[0], name)
            assert np.array_equal(g.view(np.uint16) if name != "fp32" else g.view(np.uint32),
                                  want.view(np.uint16) if name != "fp32" else want.view(np.uint32)), (fmt, H, W, Hp, Wp, T, name)
            # the padding region equals the edge pixel
            assert torch.equal(got[..., H:, :], got[..., H - 1:H, :].expand_as(got[..., H:, :]))
            assert torch.equal(got[..., :, W:], got[..., :, W - 1:W].expand_as(got[..., :, W:]))


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_egress_yuv_equals_the_float32_restatement_bit_for_bit_and_writes_nothing_else(fmt):
    f = yuv_fmt(*fmt)
    GUARD = 64
    for (H, W, Hp, Wp), T in [(s, t) for s in SIZES for t in (1, 5)]:
        g = torch.Generator().manual_seed(H * 1000 + W + T)
        x32 = torch.rand(T, 3, Hp, Wp, generator=g) * 1.4 - 0.2                  # values below 0 and above 1: the clamp matters
        fb = R.frame_bytes(fmt, H, W)
        for name, dt in DTYPES.items():
            x = x32.to(dt)
            buf = torch.full((T * fb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            got = egress_yuv(x.cuda(), f, H, W, dst=buf[GUARD:GUARD + T * fb].view(T, fb))
            want = R.egress_emu(x.float().numpy(), fmt, H, W)
            assert np.array_equal(got.cpu().numpy(), want), (fmt, H, W, Hp, Wp, T, name)
            b = buf.cpu().numpy()
            assert (b[:GUARD] == 0xA5).all() and (b[GUARD + T * fb:] == 0xA5).all()
    got = egress_yuv(torch.rand(2, 3, 16, 24).cuda(), f, 15, 23)               # allocating form
    assert got.shape == (2, R.frame_bytes(fmt, 15, 23)) and got.dtype == torch.uint8


def test_bad_arguments_are_refused():
    lib = L.load()
    f = yuv_fmt(8, L.SN_YUV_420_CENTER, 0, 0)
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    x = torch.zeros(1, 3, 8, 8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert lib.sn_ingest_yuv(buf.data_ptr(), f, x.data_ptr(), L.SN_F32, 1, 8, 8, 4, 8, s) == -22          # Hp < H
    assert lib.sn_egress_yuv(x.data_ptr(), L.SN_F32, yuv_fmt(9, 0, 0, 0), buf.data_ptr(), 1, 8, 8, 8, 8, s) == -22
    assert lib.sn_ingest_yuv(buf.data_ptr() + 1, yuv_fmt(10, 0, 0, 0), x.data_ptr(), L.SN_F32, 1, 8, 8, 8, 8, s) == -22    # odd address, 16-bit samples


# ---- the restorer -------------------------------------------------------------------------------------------------------------------
FMT420 = R.Fmt(8, R.C420_CENTER, R.BT601, R.LIMITED)


def clip_payloads(n, h, w, seed=7):
    blur, _ = synth.blurred_clip(n, h, w, seed=seed)
    x = (torch.from_numpy(blur).permute(0, 3, 1, 2).float() / 255).numpy()
    return R.egress_emu(x, FMT420, h, w)


def by_hand(net, payloads, fmt, h, w, one_len, sigma):
    """Windows assembled here: ingest_yuv -> forward_fp32_out -> egress_yuv with the reflection the issue states."""
    f = yuv_fmt(*fmt)
    dt = next(net.parameters()).dtype
    hp, wp = restore.padded_size(h, w, net.V.topo)
    n = len(payloads)

    def refl(i):
        if n <= 2:
            return min(max(i, 0), n - 1)
        return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)
    out = []
    for lo in range(0, n, one_len):
        hi = min(lo + one_len, n)
        idx = [refl(i) for i in range(lo - 2, hi + 2)]
        dev = torch.from_numpy(np.stack([payloads[i] for i in idx])).cuda()
        x = ingest_yuv(dev, f, h, w, hp, wp, dt)
        kw = {} if dt == torch.float32 else {"shortcut": ingest_yuv(dev, f, h, w, hp, wp, torch.float32)}
        with torch.no_grad():
            if net.V.denoise:
                nm = torch.full((1, 1, 1, 1, 1), sigma / 255.0, dtype=dt, device="cuda").expand(1, len(idx), 1, hp, wp)
                y = net.forward_fp32_out(x, nm, **kw)
            else:
                y = net.forward_fp32_out(x, **kw)
        assert tuple(y.shape) == (hi - lo, 3, hp, wp)
        out += list(egress_yuv(y, f, h, w).cpu().numpy())
    return out


@pytest.mark.parametrize("variant,dtype", [("deblur_small", "bf16"), ("deblur_small", "fp32"), ("denoise_small", "bf16"), ("denoise_small", "fp32")])
def test_restorer_equals_hand_assembled_windows_and_restores_every_frame(variant, dtype):
    n, h, w, one_len = 11, 70, 98, 4
    sigma = 10.0 if "denoise" in variant else None
    pay = clip_payloads(n, h, w)
    net = restore.load_net(variant, "synthetic", dtype)
    f = yuv_fmt(*FMT420)
    want = by_hand(net, pay, FMT420, h, w, one_len, sigma)
    piped = list(restore.VideoRestorer(net, one_len, sigma=sigma, pipeline=True).restore(iter(pay), f, h, w))
    serial = list(restore.VideoRestorer(net, one_len, sigma=sigma, pipeline=False).restore(iter(pay), f, h, w))
    assert len(piped) == n and len(serial) == n and len(want) == n
    for i in range(n):
        assert piped[i].shape == (R.frame_bytes(FMT420, h, w),) and piped[i].dtype == np.uint8
        assert np.array_equal(piped[i], want[i]), (i, "pipeline vs by hand")
        assert np.array_equal(serial[i], piped[i]), (i, "serial vs pipeline")
    for i in (0, 1, n - 2, n - 1):                                  # the frames upstream's harness never restores
        assert not np.array_equal(piped[i], pay[i]), i


def test_denoise_restorer_needs_sigma():
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    with pytest.raises(ValueError, match="sigma"):
        restore.VideoRestorer(net, 4)


def test_plus_variant_restores_a_size_that_is_a_multiple_of_4_but_not_of_8():
    n, h, w = 5, 100, 108
    pay = clip_payloads(n, h, w, seed=8)
    net = restore.load_net("deblur", "synthetic", "bf16")
    assert net.V.topo == "plus"
    out = list(restore.VideoRestorer(net, 4).restore(iter(pay), yuv_fmt(*FMT420), h, w))
    assert len(out) == n and all(o.shape == (R.frame_bytes(FMT420, h, w),) for o in out)        # 100 x 108 comes back
    want = by_hand(net, pay, FMT420, h, w, 4, None)
    assert all(np.array_equal(a, b) for a, b in zip(out, want))
    assert not np.array_equal(out[0], pay[0])


def test_restore_video_cli_in_a_child_process_gives_the_api_bytes(tmp_path):
    n, h, w, one_len = 11, 70, 98, 4
    pay = clip_payloads(n, h, w, seed=9)
    hd = y4m.Y4MHeader(width=w, height=h, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "deblur_small", "--checkpoint", "synthetic",
                        "--dtype", "bf16", "--one_len", str(one_len), str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "matrix bt601 (default)" in r.stderr and "range limited (stream)" in r.stderr and f"done: {n} frames" in r.stderr
    with open(dst, "rb") as fh:
        rd = y4m.Y4MReader(fh)
        got = list(rd)
    assert rd.header.line() == hd.line()
    assert len(got) == n
    net = restore.load_net("deblur_small", "synthetic", "bf16")
    api = list(restore.VideoRestorer(net, one_len).restore(iter(pay), yuv_fmt(*FMT420), h, w))
    assert all(np.array_equal(a, b) for a, b in zip(got, api))
