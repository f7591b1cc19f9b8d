"""Batched multi-clip forward (GShiftNet.forward_clips) on the MI355X: every result is compared BIT FOR BIT with the per-clip form.

Kernel level: a batched call over B clips laid end to end (sn_unit_src.clip, the conv frame remap) against one call per clip.  Whole net:
forward_clips / forward_clips_fp32_out against per-clip forward / forward_fp32_out.  The clips are distinct random data, so a frame borrowed
across a clip boundary shows.
"""
import ctypes

import pytest
import torch

from shiftnet_amd import lib as L
from shiftnet_amd import prep, synth
from shiftnet_amd.arch import CLASSES
from shiftnet_amd.engine import Act
from shiftnet_amd.spec import VARIANTS, shift_table
from shiftnet_amd.weights import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22


def _st():
    return torch.cuda.current_stream().cuda_stream


def _clips(B, T, h, w, C, dtype, seed):
    return torch.stack([torch.from_numpy(synth.unit_noise((T, h, w, C), seed=seed + b)) for b in range(B)]).to(dtype).to(DEV)


_NETS = {}


def _net(name, dtype, frames=None):
    """frames: (past, future) of the module, default the variant's; the CLIs build theirs with (2, 2)."""
    if (name, dtype, frames) not in _NETS:
        net = CLASSES[name]() if frames is None else CLASSES[name](past_frames=frames[0], future_frames=frames[1])
        net.load_state_dict(synth_state_dict(name), strict=True)
        _NETS[(name, dtype, frames)] = net.to(dtype).to(DEV).eval()
    return _NETS[(name, dtype, frames)]


def _unit_key(eng, shifted=True):
    return next(k for k, u in eng.P.units.items() if ("w1" in u) == shifted)


# ---- kernel level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", [0, 1])
@pytest.mark.parametrize("mode", [1, 2])
def test_gather_and_roll_per_clip(mode, wrap):
    lib = L.load()
    B, T, h, w, C = 3, 4, 12, 20, 64
    x = _clips(B, T, h, w, C, torch.bfloat16, 11)
    offs = prep.shift_offsets_i8(shift_table(C)).to(DEV)
    xb = x.reshape(B * T, h, w, C)
    for fn, cu in (("sn_gsts_gather", C + C // 2), ("sn_temporal_roll", C)):
        got = torch.empty((B * T, h, w, cu), dtype=torch.bfloat16, device=DEV)
        s = L.UnitSrc(xb.data_ptr(), B * T, h, w, C, mode, wrap, None, 0, 0, T)
        args = (ctypes.byref(s), offs.data_ptr(), got.data_ptr(), _st()) if fn == "sn_gsts_gather" else (ctypes.byref(s), got.data_ptr(), _st())
        L.check(getattr(lib, fn)(*args), fn)
        for b in range(B):
            ref = torch.empty((T, h, w, cu), dtype=torch.bfloat16, device=DEV)
            s1 = L.UnitSrc(x[b].data_ptr(), T, h, w, C, mode, wrap)
            a1 = (ctypes.byref(s1), offs.data_ptr(), ref.data_ptr(), _st()) if fn == "sn_gsts_gather" else (ctypes.byref(s1), ref.data_ptr(), _st())
            L.check(getattr(lib, fn)(*a1), fn)
            assert torch.equal(got[b * T:(b + 1) * T], ref), (fn, b)
        # a frame range of the batch: absolute frame indices, same rule
        part = torch.zeros_like(got)
        s = L.UnitSrc(xb.data_ptr(), B * T, h, w, C, mode, wrap, None, T - 1, T + 1, T)
        args = (ctypes.byref(s), offs.data_ptr(), part.data_ptr(), _st()) if fn == "sn_gsts_gather" else (ctypes.byref(s), part.data_ptr(), _st())
        L.check(getattr(lib, fn)(*args), fn)
        assert torch.equal(part[T - 1:2 * T], got[T - 1:2 * T])


@pytest.mark.parametrize("name", ["gshift_deblur1", "gshift_deblur2"])       # C = 80 kept / 64 circular
@pytest.mark.parametrize("fn", ["sn_gsts_shiftconv", "sn_gsts_shiftconv_mfma"])
def test_shiftconv_per_clip(name, fn):
    lib = L.load()
    eng = _net(name, torch.bfloat16).prepare()
    V = VARIANTS[name]
    C, B, T, h, w = V.c1, 2, 5, 40, 72
    x = _clips(B, T, h, w, C, torch.bfloat16, 21)
    xb = x.reshape(B * T, h, w, C)
    w1 = eng.P.units[_unit_key(eng)]["w1"]
    for mode in (1, 2):
        got = torch.empty((B * T, h, w, C // 2), dtype=torch.bfloat16, device=DEV)
        s = L.UnitSrc(xb.data_ptr(), B * T, h, w, C, mode, int(V.wrap), None, 0, 0, T)
        L.check(getattr(lib, fn)(ctypes.byref(s), eng.P.offs.data_ptr(), w1.data_ptr(), got.data_ptr(), _st()), fn)
        for b in range(B):
            ref = torch.empty((T, h, w, C // 2), dtype=torch.bfloat16, device=DEV)
            s1 = L.UnitSrc(x[b].data_ptr(), T, h, w, C, mode, int(V.wrap))
            L.check(getattr(lib, fn)(ctypes.byref(s1), eng.P.offs.data_ptr(), w1.data_ptr(), ref.data_ptr(), _st()), fn)
            assert torch.equal(got[b * T:(b + 1) * T], ref), (mode, b)


@pytest.mark.parametrize("name", ["gshift_deblur1", "gshift_deblur2", "gshift_denoise1", "gshift_denoise2"])
@pytest.mark.parametrize("phase1", ["auto", "0"])
def test_unit_blocks_per_clip(name, phase1):
    """CAB2 of both directions and CAB1 (K0, the fused phase 1 -- the denoisers' two passes -- or the two-kernel chain, the squeeze-excite
    tail, K4) with the neighbour rule per clip, against the same block run on each clip alone."""
    eng = _net(name, torch.bfloat16).prepare()
    V = VARIANTS[name]
    C, B, T, h, w = V.c1, 3, 4, 24, 40
    x = _clips(B, T, h, w, C, torch.bfloat16, 31)
    old = eng.phase1
    eng.phase1 = phase1
    try:
        for mode in (1, 2, 0):
            pre = _unit_key(eng, shifted=mode != 0)
            eng._clip = T
            try:
                got = eng.naf(pre, Act(x.reshape(B * T, h, w, C), C), mode).t.clone()
            finally:
                eng._clip = 0
            for b in range(B):
                ref = eng.naf(pre, Act(x[b].contiguous(), C), mode).t
                assert torch.equal(got[b * T:(b + 1) * T], ref), (mode, b)
    finally:
        eng.phase1 = old


@pytest.mark.parametrize("wrap", [0, 1])
def test_fp32_gather_and_shiftconv_per_clip(wrap):
    lib = L.load()
    eng = _net("gshift_denoise1", torch.float32).prepare()
    B, T, h, w, C = 2, 5, 16, 24, 80
    x = _clips(B, T, h, w, C, torch.float32, 41)
    xb = x.reshape(B * T, h, w, C)
    offs = eng.P.offs
    key = next(k for k in eng.P.sd if k.endswith(".conv1.weight"))       # the depthwise conv1 of a CAB2 ([3][3][1][C/2] = tap-major [9][C/2])
    w1 = eng.P.wt(key)
    for mode in (1, 2):
        s = L.UnitSrc(xb.data_ptr(), B * T, h, w, C, mode, wrap, None, 0, 0, T)
        u = torch.empty((B * T, h, w, C + C // 2), device=DEV)
        vin = torch.empty((B * T, h, w, C + C // 2), device=DEV)
        L.check(lib.sn32_gsts_gather(ctypes.byref(s), offs.data_ptr(), u.data_ptr(), None, _st()), "sn32_gsts_gather")
        L.check(lib.sn32_gsts_shiftconv(ctypes.byref(s), offs.data_ptr(), w1.data_ptr(), vin.data_ptr(), None, _st()), "sn32_gsts_shiftconv")
        for b in range(B):
            s1 = L.UnitSrc(x[b].data_ptr(), T, h, w, C, mode, wrap)
            u1 = torch.empty((T, h, w, C + C // 2), device=DEV)
            v1 = torch.empty((T, h, w, C + C // 2), device=DEV)
            L.check(lib.sn32_gsts_gather(ctypes.byref(s1), offs.data_ptr(), u1.data_ptr(), None, _st()), "sn32_gsts_gather")
            L.check(lib.sn32_gsts_shiftconv(ctypes.byref(s1), offs.data_ptr(), w1.data_ptr(), v1.data_ptr(), None, _st()), "sn32_gsts_shiftconv")
            assert torch.equal(u[b * T:(b + 1) * T], u1) and torch.equal(vin[b * T:(b + 1) * T], v1), (mode, b)


def test_clip_that_does_not_divide_t_or_meets_a_halo_is_einval():
    lib = L.load()
    T, h, w, C = 6, 8, 16, 64
    x = torch.zeros((T, h, w, C), dtype=torch.bfloat16, device=DEV)
    halo = torch.zeros((h, w, C // 2), dtype=torch.bfloat16, device=DEV)
    offs = prep.shift_offsets_i8(shift_table(C)).to(DEV)
    u = torch.empty((T, h, w, C + C // 2), dtype=torch.bfloat16, device=DEV)
    for clip, wrap, hp in ((4, 0, None), (7, 1, None), (-1, 0, None), (3, 2, halo.data_ptr()), (T, 2, halo.data_ptr())):
        s = L.UnitSrc(x.data_ptr(), T, h, w, C, 1, wrap, hp, 0, 0, clip)
        assert lib.sn_gsts_gather(ctypes.byref(s), offs.data_ptr(), u.data_ptr(), _st()) == EINVAL, (clip, wrap)
        assert lib.sn_temporal_roll(ctypes.byref(s), u.data_ptr(), _st()) == EINVAL, (clip, wrap)
        s32 = L.UnitSrc(x.data_ptr(), T, h, w, C, 1, wrap, hp, 0, 0, clip)
        assert lib.sn32_gsts_gather(ctypes.byref(s32), offs.data_ptr(), u.data_ptr(), None, _st()) == EINVAL
    s = L.UnitSrc(x.data_ptr(), T, h, w, C, 1, 0, None, 0, 0, 3)      # a valid clip
    L.check(lib.sn_gsts_gather(ctypes.byref(s), offs.data_ptr(), u.data_ptr(), _st()), "gather")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype,exact", [(torch.bfloat16, False), (torch.float32, False), (torch.float32, True)])
@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_denoise1"])      # rconcat of 3 x 16 / 3 x 24 channels, without / with PReLU
def test_rconcat_remap_reads_kept_frames_in_place(name, dtype, exact):
    eng = _net(name, dtype).prepare()
    old = getattr(eng, "split_bf16", None)
    if dtype == torch.float32:
        eng.split_bf16 = not exact
    try:
        V = VARIANTS[name]
        B, T, lo, n, h, w = 3, 7, 2, 3, 24, 40
        cs = V.c0 if dtype == torch.float32 else prep.ceil8(V.c0)
        ins = [_clips(B, T, h, w, cs, dtype, 51 + 7 * i) for i in range(3)]
        if dtype != torch.float32 and cs != V.c0:
            for t in ins:
                t[..., V.c0:] = 0
        prelu = eng.P.scalar("lrelu.weight") if V.denoise else None
        got = eng.conv("rconcat", [Act(t.reshape(B * T, h, w, cs), V.c0) for t in ins], prelu=prelu, remap=(n, T, lo)).t
        ref = eng.conv("rconcat", [Act(t[:, lo:lo + n].reshape(B * n, h, w, cs).contiguous(), V.c0) for t in ins], prelu=prelu).t
        assert got.shape == ref.shape and torch.equal(got, ref)
    finally:
        if old is not None:
            eng.split_bf16 = old


def test_remap_is_refused_where_it_is_not_implemented():
    lib = L.load()
    d = L.ConvDesc()
    d.n_in, d.cs_in, d.T, d.h_in, d.w_in, d.k, d.stride, d.pad, d.h_out, d.w_out = 1, 16, 4, 32, 64, 3, 1, 1, 32, 64
    d.mt, d.ks, d.cs_out, d.c_out = 1, 5, 16, 16
    x = torch.zeros((8, 32, 64, 16), dtype=torch.bfloat16, device=DEV)
    o = torch.zeros((4, 32, 64, 16), dtype=torch.bfloat16, device=DEV)
    wf = torch.zeros((1, 5, 64, 8), dtype=torch.bfloat16, device=DEV)
    d.inp[0], d.out, d.wfrag = x.data_ptr(), o.data_ptr(), wf.data_ptr()
    d.clip_n, d.clip_T, d.clip_lo = 2, 4, 1
    assert lib.sn_conv2d(ctypes.byref(d), _st()) == EINVAL               # single-input 3x3: the specialised kernels, no remap
    d.flags = L.SN_CONV_TILE_KERNEL
    assert lib.sn_conv2d(ctypes.byref(d), _st()) == EINVAL
    d.clip_n, d.clip_T, d.clip_lo = 3, 4, 0                              # 4 output frames are not whole clips of 3
    d.inp[1], d.inp[2], d.n_in, d.ks = x.data_ptr(), x.data_ptr(), 3, 14
    assert lib.sn_conv2d(ctypes.byref(d), _st()) == EINVAL
    torch.cuda.synchronize()


# ---- whole net ----------------------------------------------------------------------------------------------------------------------
def _inputs(name, dtype, B, T, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, T, 3, H, W), generator=g).to(dtype).to(DEV)
    nm = (torch.rand((B, 1, 1, 1, 1), generator=g) * 0.2).expand(B, T, 1, H, W).to(dtype).to(DEV) if "denoise" in name else None
    return x, nm


def _per_clip(net, name, x, nm, fp32_out=False, shortcut=None):
    outs = []
    for b in range(x.shape[0]):
        xb = x[b:b + 1]
        if fp32_out:
            sc = shortcut[b:b + 1] if shortcut is not None else None
            o = net.forward_fp32_out(xb, nm[b:b + 1], shortcut=sc) if nm is not None else net.forward_fp32_out(xb, shortcut=sc)
        else:
            o = net(xb, nm[b:b + 1]) if nm is not None else net(xb)
        outs.append(o)
    return torch.stack(outs)


def _batched(net, x, nm, fp32_out=False, shortcut=None):
    if fp32_out:
        return net.forward_clips_fp32_out(x, nm, shortcut=shortcut) if nm is not None else net.forward_clips_fp32_out(x, shortcut=shortcut)
    return net.forward_clips(x, nm) if nm is not None else net.forward_clips(x)


WHOLE = [("gshift_deblur1", torch.bfloat16, False), ("gshift_deblur2", torch.bfloat16, False), ("gshift_denoise1", torch.bfloat16, False),
         ("gshift_denoise2", torch.bfloat16, False), ("gshift_deblur2", torch.float16, False), ("gshift_denoise1", torch.float32, False),
         ("gshift_denoise1", torch.float32, True)]


@pytest.mark.parametrize("name,dtype,exact", WHOLE)
@pytest.mark.parametrize("B", [2, 3])
def test_forward_clips_equals_per_clip_forward(name, dtype, exact, B):
    net = _net(name, dtype)
    eng = net.prepare()
    old = getattr(eng, "split_bf16", None)
    if dtype == torch.float32:
        eng.split_bf16 = not exact
    try:
        T, H, W = 6, 48, 64
        x, nm = _inputs(name, dtype, B, T, H, W, seed=100 + B)
        got = _batched(net, x, nm)
        assert got.shape == (B, T - net.num_fb - net.num_ff, 3, H, W) and got.dtype == dtype
        assert torch.equal(got, _per_clip(net, name, x, nm))
        sc = torch.rand((B, T, 3, H, W), generator=torch.Generator().manual_seed(7)).to(DEV)     # a float32 shortcut, as the CLIs pass
        got32 = _batched(net, x, nm, fp32_out=True, shortcut=sc if dtype != torch.float32 else None)
        assert got32.dtype == torch.float32
        assert torch.equal(got32, _per_clip(net, name, x, nm, fp32_out=True, shortcut=sc if dtype != torch.float32 else None))
        if B == 2:                                                        # B = 1 is forward itself
            assert torch.equal(_batched(net, x[:1], nm[:1] if nm is not None else None)[0], got[0])
    finally:
        if old is not None:
            eng.split_bf16 = old


def test_forward_clips_graph_replay_matches_eager():
    name = "gshift_denoise2"
    net = _net(name, torch.bfloat16)
    eng = net.prepare()
    assert eng.graph_auto and 3 * 6 * 48 * 64 <= eng.GRAPH_AUTO_PXF
    x, nm = _inputs(name, torch.bfloat16, 3, 6, 48, 64, seed=5)
    first = _batched(net, x, nm)                                          # eager (first sight of the signature)
    second = _batched(net, x, nm)                                         # captured and replayed
    third = _batched(net, x, nm)
    key = next(k for k in eng._graphs if k[-1] == 6 and k[0][0] == 18)
    assert isinstance(eng._graphs[key], tuple)
    assert torch.equal(first, second) and torch.equal(first, third)
    # another batch with the same frame count keeps its own graph: (2 clips of 9) != (3 clips of 6)
    x2, nm2 = x.reshape(2, 9, 3, 48, 64), nm.reshape(2, 9, 1, 48, 64)
    assert torch.equal(_batched(net, x2, nm2), _per_clip(net, name, x2, nm2))
    assert torch.equal(_batched(net, x2, nm2), _per_clip(net, name, x2, nm2))


def test_streaming_fused_cab_threshold_crossed_by_the_batch_only():
    name = "gshift_deblur2"
    net = _net(name, torch.bfloat16)
    eng = net.prepare()
    B, T, H, W = 2, 8, 512, 576
    assert T * H * W < eng.CAB_FUSED_MIN_PX <= B * T * H * W and eng.cab_fused == "p16"
    x, _ = _inputs(name, torch.bfloat16, B, T, H, W, seed=9)
    assert torch.equal(_batched(net, x, None), _per_clip(net, name, x, None))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("on_device", [True, False])
def test_quadrant_forward_batched_equals_sequential(dtype, on_device):
    from shiftnet_amd import cli
    net = _net("gshift_denoise1", dtype, (2, 2))
    g = torch.Generator().manual_seed(3)
    sigma = 20 / 255.0
    x32 = (torch.rand((1, 6, 3, 64, 96), generator=g) + torch.randn((1, 6, 3, 64, 96), generator=g) * sigma).to(DEV)
    x = x32.to(dtype)
    a = cli.quadrant_forward(net, x, sigma, on_device=on_device, x32=x32)
    b = cli.quadrant_forward(net, x, sigma, on_device=on_device, x32=x32, batch=True)
    assert a.shape == (2, 3, 64, 96) and torch.equal(a, b)


def test_forward_clips_with_temporal_split_raises():
    net = _net("gshift_deblur2", torch.bfloat16)
    net.set_temporal_split(0, 2)
    try:
        with pytest.raises(ValueError, match="temporal split"):
            net.forward_clips(torch.zeros((2, 5, 3, 32, 32), dtype=torch.bfloat16, device=DEV))
        eng = net.prepare()
        with pytest.raises(ValueError, match="temporal split"):
            eng.forward_clips(torch.zeros((2, 5, 3, 32, 32), dtype=torch.bfloat16, device=DEV), None, 2, 2)
    finally:
        net.set_temporal_split(0, 1)
