"""-m gpu: ``VideoRestorer(ensemble=...)`` against each window composed by hand -- the existing ingest, ``net.forward_ensemble_fp32_out`` on the window,
the existing egress -- byte for byte."""
import numpy as np
import pytest
import torch

import yuv_ref as R
from shiftnet_amd import noise, restore, synth, windows
from shiftnet_amd.io_edges import egress_yuv, ingest_u8, ingest_yuv, noise_map_level, yuv_fmt

pytestmark = pytest.mark.gpu

FMT = R.Fmt(8, R.C420_CENTER, R.BT601, R.LIMITED)
H, W, FRAMES, ONE_LEN = 36, 52, 10, 4    # three windows, the last one short
RECT = (4, 2, 40, 28)                    # x0, y0, w, h
M = 4
NEW_KEYS = {"ensemble", "ensemble_time", "ensemble_members", "ensemble_launches"}


def clip(sigma=0.0, seed=3):
    """FRAMES payloads of the synthetic sharp clip, 4:2:0 8 bit, made by the existing egress."""
    rgb = synth.sharp_clip(FRAMES, H, W, seed)
    if sigma:
        rgb = np.clip(np.rint(rgb.astype(np.float64) + np.random.default_rng(seed).normal(0.0, sigma, rgb.shape)), 0, 255).astype(np.uint8)
    x = ingest_u8(torch.from_numpy(rgb).cuda(), torch.float32)[0]
    return list(egress_yuv(x, yuv_fmt(*FMT), H, W).cpu().numpy())


def two_band_clip(split=26, seed=11):
    """FRAMES payloads whose left part is dark with luma noise of sigma 5 codes and whose right part is bright with sigma 2, noisy chroma: the
    noise-level function estimated from them has two bands with an estimate of their own, so the noise plane is not flat."""
    rng = np.random.default_rng(seed)
    ch, cw = R.chroma_shape(FMT, H, W)
    col = np.arange(W)[None, :]
    out = []
    for _ in range(FRAMES):
        Y = np.where(col < split, 64.0 + rng.normal(0.0, 5.0, (H, W)), 187.0 + rng.normal(0.0, 2.0, (H, W)))
        U, V = (np.clip(np.rint(128 + rng.normal(0.0, 3.0, (ch, cw))), 16, 240).astype(np.int64) for _ in range(2))
        out.append(R.join_planes(np.clip(np.rint(Y), 0, 255).astype(np.int64), U, V, FMT))
    return out


def run(net, pay, **kw):
    vr = restore.VideoRestorer(net, ONE_LEN, **kw)
    out = list(vr.restore(iter(pay), yuv_fmt(*FMT), H, W))
    return out, vr.stats, vr


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def composed(net, pay, rect=None, curves=None, **kw):
    """What the restorer must write, window by window: ingest_yuv, ``net.forward_ensemble_fp32_out`` on the window (with the noise plane of the window's
    curve under ``curves``), egress_yuv -- into a copy of the input's own frames where a picture is restored."""
    f = yuv_fmt(*FMT)
    dt = next(net.parameters()).dtype
    h, w = (H, W) if rect is None else (rect[3], rect[2])
    hp, wp = windows.padded_size(h, w, net.V.topo)
    lo, hi = noise.clip_codes(FMT.bits, FMT.range)
    out = []
    plan = windows.plan_windows(FRAMES, ONE_LEN)
    assert [n for _, n, _ in plan] == [4, 4, 2]
    for k, (_, n, idx) in enumerate(plan):
        dev = torch.from_numpy(np.stack([pay[i] for i in idx])).cuda()
        x = ingest_yuv(dev, f, H, W, hp, wp, dt, rect=rect)
        more = {"shortcut": ingest_yuv(dev, f, H, W, hp, wp, torch.float32, rect=rect)} if dt != torch.float32 else {}
        args = (x,)
        if curves is not None:
            args = (x, noise_map_level(dev, f, H, W, hp, wp, [c / 255.0 for c in curves[k]], dt, lo, hi, rect=rect))
        with torch.no_grad():
            o = net.forward_ensemble_fp32_out(*args, **more, **kw)
        assert o.dtype == torch.float32 and tuple(o.shape) == (n, 3, hp, wp)
        dst = dev[windows.PAST:windows.PAST + n].clone() if rect is not None else None
        out += list(egress_yuv(o, f, H, W, dst=dst, rect=rect).cpu().numpy())
    return out


@pytest.fixture(scope="module")
def deblur():
    net = restore.load_net("deblur_small", "synthetic", "bf16")
    pay = clip()
    plain, stats, vr = run(net, pay)
    assert not (NEW_KEYS & set(stats)) and vr.run.launches["geo_transform"] == vr.run.launches["geo_accumulate"] == 0 and vr.ensemble_part is None
    return net, pay, plain, stats


def test_the_restorer_writes_the_bytes_of_the_composition(deblur):
    net, pay, plain, _ = deblur
    want = composed(net, pay, ensemble=M)
    got, stats, _ = run(net, pay, ensemble=M)
    assert same(got, want) and not same(got, plain)
    assert stats["ensemble"] == M and stats["ensemble_time"] is False and stats["ensemble_members"] == [0, 1, 2, 3]
    assert stats["windows"] == 3 and stats["frames"] == FRAMES
    assert getattr(net.prepare(), "fallbacks", 0) == 0                               # the range guard did not trip: the counts are not doubled
    # a bf16 module: the frames and their float32 twin are transformed for every member but the first
    assert stats["ensemble_launches"] == {"transform": 3 * (M - 1) * 2, "accumulate": 3 * M}
    serial, stats2, _ = run(net, pay, ensemble=M, pipeline=False)
    assert same(serial, got) and stats2["ensemble_launches"] == stats["ensemble_launches"]


def test_transposed_and_time_reversed_members_in_the_restorer(deblur):
    net, pay, plain, _ = deblur
    got, stats, _ = run(net, pay, ensemble=8, ensemble_time=True)
    assert same(got, composed(net, pay, ensemble=8, time=True)) and not same(got, plain)
    assert stats["ensemble_members"] == list(range(16)) and stats["ensemble_launches"] == {"transform": 3 * 15 * 2, "accumulate": 3 * 16}
    assert getattr(net.prepare(), "fallbacks", 0) == 0


def test_a_picture_is_restored_as_the_composition_on_the_rectangle(deblur):
    net, pay, _, _ = deblur
    want = composed(net, pay, rect=RECT, ensemble=M)
    got, stats, _ = run(net, pay, picture=RECT, ensemble=M)
    assert same(got, want) and stats["window_picture"] == [RECT] * 3
    assert stats["ensemble_launches"] == {"transform": 3 * (M - 1) * 2, "accumulate": 3 * M}
    assert same(run(net, pay, picture=RECT, ensemble=M, pipeline=False)[0], got)
    assert not same(got, run(net, pay, picture=RECT)[0])


def test_the_noise_plane_is_transformed_with_the_frames():
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    pay = two_band_clip()
    kw = dict(sigma="auto", noise_model="level")
    got, stats, _ = run(net, pay, ensemble=M, **kw)
    curves = stats["window_nlf"]
    assert len(curves) == 3 and all(c[3] > 2.0 * c[12] > 0.0 for c in curves)        # a plane that is not flat: left and right differ
    assert same(got, composed(net, pay, curves=curves, ensemble=M))
    assert getattr(net.prepare(), "fallbacks", 0) == 0
    # three tensors move: the frames, their float32 twin, the plane
    assert stats["ensemble_launches"] == {"transform": 3 * (M - 1) * 3, "accumulate": 3 * M}
    assert same(run(net, pay, ensemble=M, pipeline=False, **kw)[0], got)
    assert not same(got, run(net, pay, **kw)[0])
    flat, fstats, _ = run(net, pay, sigma=10.0, ensemble=M)                          # a flat level: nothing of it is copied
    assert fstats["ensemble_launches"] == {"transform": 3 * (M - 1) * 2, "accumulate": 3 * M}
    f = yuv_fmt(*FMT)
    dev = torch.from_numpy(np.stack([pay[i] for i in windows.plan_windows(FRAMES, ONE_LEN)[0][2]])).cuda()
    x, x32 = ingest_yuv(dev, f, H, W, H, W, torch.bfloat16), ingest_yuv(dev, f, H, W, H, W, torch.float32)
    with torch.no_grad():
        o = net.forward_ensemble_fp32_out(x, 10.0 / 255.0, shortcut=x32, ensemble=M)
    assert same(flat[:4], list(egress_yuv(o, f, H, W).cpu().numpy()))


def test_ensemble_none_and_one_are_the_restorer_without_the_argument(deblur):
    net, pay, plain, stats_plain = deblur
    for e in (None, 1):
        got, stats, vr = run(net, pay, ensemble=e)
        assert same(got, plain) and set(stats) == set(stats_plain) and vr.ensemble is None and vr.ensemble_part is None
        assert {k: v for k, v in stats.items() if k.endswith("_launches")} == {k: v for k, v in stats_plain.items() if k.endswith("_launches")}


def test_an_ensemble_with_tiles_is_refused(deblur):
    net = deblur[0]
    with pytest.raises(ValueError, match="tile"):
        restore.VideoRestorer(net, ONE_LEN, ensemble=4, tile=16)
    with pytest.raises(ValueError, match="tile"):
        restore.VideoRestorer(net, ONE_LEN, ensemble_time=True, tile=16)
    with pytest.raises(ValueError, match="ensemble"):
        restore.VideoRestorer(net, ONE_LEN, ensemble=3)
