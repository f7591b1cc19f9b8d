"""sn_cab2_phase2_cab1_phase1 (csrc/sn_phase1r.hip, the FK4 instance): the CAB2's phase 2 inside the stager waves of the CAB1's phase 1 -- four
launches per GSTS unit instead of five.  The fused launch performs the operations of the two launches it replaces in their order, so every
comparison here is torch.equal on raw bits against the same engine with the switch off (Engine.k4_fuse = "0", SN_K4_FUSE=0)."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "shift-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import shiftnet_oracle as O
from shiftnet_amd import synth
from shiftnet_amd.spec import VARIANTS
from shiftnet_amd.weights import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FUSED = "sn_cab2_phase2_cab1_phase1"
BLK = "stage1.decoder_level1."


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def eng64():
    from shiftnet_amd.engine import Engine, Plan
    sd = synth_state_dict("gshift_deblur2")
    return Engine(Plan(VARIANTS["gshift_deblur2"], sd, DEV))


def sibling(eng, **attrs):
    """A second Engine on the same prepared weights that records the C-ABI functions it launches."""
    from shiftnet_amd.engine import Engine
    e = Engine(eng.P)
    for k, v in attrs.items():
        setattr(e, k, v)
    e.called = []
    orig = e._call
    e._call = lambda fn, *a: (e.called.append(fn), orig(fn, *a))[1]
    return e


def noise(shape, seed):
    return torch.from_numpy(synth.unit_noise(shape, seed=seed)).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("team", [0, 1])
@pytest.mark.parametrize("T,h,w", [(3, 7, 21), (2, 5, 9), (2, 13, 70), (3, 40, 200), (2, 97, 130), (1, 64, 42), (1, 3, 40), (4, 33, 64), (5, 21, 122), (2, 9, 123)])
def test_entry_point_equals_the_two_launches(T, h, w, team, eng64):
    """The entry point alone against sn_gsts_cab2_phase2 + sn_cab1_phase1 on the same operands: y, g2, every pool row and the squeeze-excite scale,
    for both unit directions, kept and circular boundary frames, bias present and absent; one strip, two border strips, three strips, rows fewer
    than the warm-up, ragged frame blocks.  y starts as NaN everywhere: every element must have been written."""
    from shiftnet_amd import lib as L
    eng, lib = eng64, eng64.lib
    C = 64
    st = torch.cuda.current_stream().cuda_stream
    nblk = lib.sn_phase1_pool_blocks(T, h, w)
    assert nblk >= 1 and lib.sn_cab2_phase2_cab1_phase1_supported(ctypes.byref(L.UnitSrc(1, T, h, w, C, 1, 0)))
    x = noise((T, h, w, C), 300 + h)
    g2_in = noise((T, h, w, C), 301 + h)
    ca_in = (0.25 + torch.rand((T, C), generator=torch.Generator().manual_seed(w))).float().to(DEV)
    some_bias = torch.from_numpy(synth.unit_noise((C,), seed=303)).float().to(DEV)
    for mode, unit in ((1, "encoder_level1."), (2, "encoder_level1_1.")):
        u2, u1 = eng.P.units[BLK + unit + "0."], eng.P.units[BLK + unit + "1."]
        q = eng.P.cas[BLK + unit + "1.ca2"]
        for with_bias in (True, False):
            wrap = (mode + int(with_bias)) & 1
            bias = (u2["b_out"] if u2["b_out"] is not None else some_bias) if with_bias else None
            bptr = bias.data_ptr() if bias is not None else None
            src2 = L.UnitSrc(x.data_ptr(), T, h, w, C, mode, wrap)
            opt = L.Phase1Opts(None, 0, team)

            def fresh():
                return (torch.full((T, h, w, C), float("nan"), dtype=torch.bfloat16, device=DEV), torch.full((T, h, w, C), float("nan"), dtype=torch.bfloat16, device=DEV),
                        torch.full((T, nblk, C), float("nan"), dtype=torch.float32, device=DEV), torch.full((T, C), float("nan"), dtype=torch.float32, device=DEV),
                        torch.zeros((T,), dtype=torch.int32, device=DEV))
            y0, g0, p0, c0, t0 = fresh()
            se0 = L.SeFold(q["wa"].data_ptr(), q["wb"].data_ptr(), q["c"], q["cr"], t0.data_ptr(), c0.data_ptr(), None)
            L.check(lib.sn_gsts_cab2_phase2(ctypes.byref(src2), g2_in.data_ptr(), ca_in.data_ptr(), u2["w_out"].data_ptr(), bptr, y0.data_ptr(), st), "K4")
            src1 = L.UnitSrc(y0.data_ptr(), T, h, w, C, 0, 0)
            L.check(lib.sn_cab1_phase1(ctypes.byref(src1), ctypes.byref(u1["p1r"]["desc"]), g0.data_ptr(), p0.data_ptr(), ctypes.byref(se0), ctypes.byref(opt), st), "phase 1")
            y1, g1, p1, c1, t1 = fresh()
            se1 = L.SeFold(q["wa"].data_ptr(), q["wb"].data_ptr(), q["c"], q["cr"], t1.data_ptr(), c1.data_ptr(), None)
            L.check(lib.sn_cab2_phase2_cab1_phase1(ctypes.byref(src2), g2_in.data_ptr(), ca_in.data_ptr(), u2["w_out"].data_ptr(), bptr, y1.data_ptr(),
                                                   ctypes.byref(u1["p1r"]["desc"]), g1.data_ptr(), p1.data_ptr(), ctypes.byref(se1), ctypes.byref(opt), st), "fused")
            torch.cuda.synchronize()
            tag = (T, h, w, team, mode, wrap, with_bias)
            assert not torch.isnan(y1.float()).any(), tag                      # every element of y written
            assert torch.isfinite(g0.float()).all() and torch.isfinite(p0).all() and torch.isfinite(c0).all(), tag
            for a, b, what in ((y0, y1, "y"), (g0, g1, "g2"), (p0, p1, "pool"), (c0, c1, "ca")):
                assert same(a, b), (tag, what)
            assert int(t1.abs().sum()) == 0, tag


def test_entry_point_refuses_what_it_does_not_cover(eng64):
    """C = 80, a frame range, a temporally split boundary (wrap 2), a batch of clips, CAB1 sources: SN_EINVAL before anything is launched."""
    from shiftnet_amd import lib as L
    lib = eng64.lib
    T, h, w = 4, 8, 16
    t = noise((T, h, w, 80), 310)
    for s in (L.UnitSrc(t.data_ptr(), T, h, w, 80, 1, 0), L.UnitSrc(t.data_ptr(), T, h, w, 64, 1, 0, None, 1, 2), L.UnitSrc(t.data_ptr(), T, h, w, 64, 1, 2, t.data_ptr()),
              L.UnitSrc(t.data_ptr(), T, h, w, 64, 2, 0, None, 0, 0, 2), L.UnitSrc(t.data_ptr(), T, h, w, 64, 0, 0)):
        assert lib.sn_cab2_phase2_cab1_phase1_supported(ctypes.byref(s)) == 0
        rc = lib.sn_cab2_phase2_cab1_phase1(ctypes.byref(s), t.data_ptr(), t.data_ptr(), t.data_ptr(), None, t.data_ptr(), None, t.data_ptr(), None, None, None,
                                            torch.cuda.current_stream().cuda_stream)
        assert rc == -22, rc                                                 # SN_EINVAL


@pytest.mark.parametrize("T,h,w", [(4, 20, 44), (2, 13, 70), (3, 184, 328)])
def test_unit_and_shift_block_fused_equal_unfused(T, h, w, eng64):
    from shiftnet_amd.engine import Act
    on, off = sibling(eng64), sibling(eng64, k4_fuse="0")
    assert on.k4_fused(T, 64) and not off.k4_fused(T, 64)
    x = Act(noise((T, h, w, 64), 320 + h), 64)
    for unit, rev in (("encoder_level1.", False), ("encoder_level1_1.", True)):
        on.called.clear(); off.called.clear()
        a, b = on.gsts_unit(BLK + unit, x, rev).t, off.gsts_unit(BLK + unit, x, rev).t
        torch.cuda.synchronize()
        assert torch.isfinite(b.float()).all() and same(a, b), (T, h, w, unit)
        assert on.called.count(FUSED) == 1 and "sn_gsts_cab2_phase2" not in on.called and on.called.count("sn_cab1_phase2") == 1 and len(on.called) == 4, on.called
        assert FUSED not in off.called and len(off.called) == 5, off.called
    on.called.clear()
    a, b = on.shift_block(BLK, x).t, off.shift_block(BLK, x).t
    torch.cuda.synchronize()
    assert same(a, b) and on.called.count(FUSED) == on.V.units


def test_naf_alone_keeps_its_contract(eng64):
    """Engine.naf called on its own returns the CAB's y, fused route or not."""
    from shiftnet_amd.engine import Act
    on, off = sibling(eng64), sibling(eng64, k4_fuse="0")
    x = Act(noise((3, 20, 44, 64), 331), 64)
    for pre, mode in ((BLK + "encoder_level1.0.", 1), (BLK + "encoder_level1_1.0.", 2), (BLK + "encoder_level1.1.", 0)):
        a, b = on.naf(pre, x, mode), off.naf(pre, x, mode)
        torch.cuda.synchronize()
        assert isinstance(a, Act) and same(a.t, b.t) and FUSED not in on.called


def _net(name, dt=torch.bfloat16):
    mod = importlib.import_module(f"basicsr.models.archs.{name}")
    net = mod.GShiftNet(future_frames=2, past_frames=2)
    net.load_state_dict(synth_state_dict(name), strict=True)
    net = net.to(dt).cuda().eval()
    eng = net.prepare()
    eng.graph_auto, eng.use_graph = False, False          # the switch changes between calls with one input signature: no replay of the other route
    eng.called = []
    orig = eng._call
    eng._call = lambda fn, *a: (eng.called.append(fn), orig(fn, *a))[1]
    return net, eng


def _clip(T, H, W, seed):
    blur, _ = synth.blurred_clip(T, H, W, seed=seed)
    return O.frames_to_tensor(list(blur)).bfloat16().cuda()


def _on_off(net, eng, run):
    outs, calls = [], []
    for sw in ("1", "0"):
        eng.k4_fuse = sw
        eng.called.clear()
        with torch.no_grad():
            outs.append(run())
        torch.cuda.synchronize()
        calls.append(list(eng.called))
    eng.k4_fuse = "1"
    return outs, calls


@pytest.mark.parametrize("T,H,W", [(5, 64, 96), (6, 120, 200)])
def test_whole_forward_fused_equals_unfused(T, H, W):
    net, eng = _net("gshift_deblur2")
    x = _clip(T, H, W, 41)
    (a, b), (ca, cb) = _on_off(net, eng, lambda: net(x))
    assert torch.isfinite(b.float()).all() and same(a, b)
    n = ca.count(FUSED)
    assert n > 0 and n == cb.count("sn_gsts_cab2_phase2") and "sn_gsts_cab2_phase2" not in ca and FUSED not in cb
    assert ca.count("sn_cab1_phase2") == cb.count("sn_cab1_phase2") == n


def test_unsupported_routes_fall_back_and_equal_the_unfused_run():
    """forward_clips, SN_SCHEDULE=frame, C = 80 (gshift_deblur1) and a denoiser (gshift_denoise2): five launches whatever the switch says."""
    net, eng = _net("gshift_deblur2")
    x = _clip(7, 48, 64, 43)
    xb = torch.cat((x, torch.roll(x, 1, dims=1)), 0)
    (a, b), (ca, cb) = _on_off(net, eng, lambda: net.forward_clips(xb))
    assert same(a, b) and FUSED not in ca and ca == cb
    eng.schedule, eng.frame_group = "frame", 2
    (a, b), (ca, cb) = _on_off(net, eng, lambda: net(x))
    assert same(a, b) and FUSED not in ca and ca == cb
    eng.schedule = "unit"
    (a2, _), (ca2, _) = _on_off(net, eng, lambda: net(x))
    assert same(a2, a) and FUSED in ca2                                        # ... and the frame wavefront equals the fused unit schedule
    for name in ("gshift_deblur1", "gshift_denoise2"):
        net, eng = _net(name)
        x = _clip(5, 64, 96, 44)
        nm = torch.full((1, 5, 1, 64, 96), 30.0 / 255.0, dtype=torch.bfloat16, device="cuda")
        run = (lambda: net(x, nm)) if VARIANTS[name].denoise else (lambda: net(x))
        (a, b), (ca, cb) = _on_off(net, eng, run)
        assert same(a, b) and FUSED not in ca and ca == cb, name


def test_temporally_split_window_equals_the_unfused_long_window(tmp_path):
    """Two ranks, each with half the window (their units keep five launches: the boundary frame's halo), against the long window on one device with
    the switch off -- and the long window with the switch on equals both."""
    import torch.multiprocessing as mp
    import test_temporal_split as TS
    mp.spawn(TS._gpu_worker, args=(2, TS._free_port(), "gshift_deblur2", "bfloat16", str(tmp_path)), nprocs=2, join=True)
    parts = np.concatenate([np.load(tmp_path / f"part{r}.npy") for r in range(2)], 0)
    full_on = np.load(tmp_path / "full.npy")                                   # rank 0's unsplit run, default switches
    net, eng = _net("gshift_deblur2")
    x = _clip(10, 48, 64, 17)
    (a, b), (ca, cb) = _on_off(net, eng, lambda: net(x))
    assert FUSED in ca and FUSED not in cb
    assert np.array_equal(parts, b.float().cpu().numpy()) and np.array_equal(full_on, b.float().cpu().numpy()) and same(a, b)


def test_graph_capture_with_the_fusion_on_replays_bit_identically():
    net, eng = _net("gshift_deblur2")
    xa = _clip(8, 64, 96, 29)
    xb = torch.roll(xa, 2, dims=1).contiguous()
    with torch.no_grad():
        ea, eb = net(xa), net(xb)
        assert FUSED in eng.called
        eng.use_graph = True
        try:
            outs = [net(xa), net(xa), net(xb), net(xa)]                        # eager (first sight), capture, replay with another input, replay
            torch.cuda.synchronize()
            assert any(isinstance(v, tuple) for v in eng._graphs.values())
        finally:
            eng.use_graph = False
    assert same(outs[0], ea) and same(outs[1], ea) and same(outs[2], eb) and same(outs[3], ea)
