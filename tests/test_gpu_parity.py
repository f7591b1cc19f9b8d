"""Parity of the bf16-storage HIP path (through the C ABI) against the CPU oracle and the committed golden fixtures.  -m gpu.

Everything these kernels store is bf16, all accumulation is fp32.  Tolerances (stated per test, relative to the
reference tensor's max-abs ``scale``; each is <= 2x the error measured on MI355X, see gpurun_out/parity_report.json):
  * pure index work (GSTS gather, temporal roll): bit exact;
  * single kernels fed bf16-rounded inputs:            max-abs <= 8e-3 * scale (observed 2.4e-3 .. 4.2e-3: one output
    rounding of a value near the top of a bf16 binade is 2^-8 = 3.9e-3 relative on its own);
  * CAB, CAB2, CAB1:                                   max-abs <= 8e-3 * scale (observed <= 2.7e-3 / 4.7e-3 / 3.9e-3);
  * GSTS unit (CAB2 + CAB1):                           max-abs <= 1.2e-2 * scale (observed <= 6.4e-3, 184x328 case);
  * TFR_UNet (20 CABs):                                max-abs <= 1.4e-2 * scale (observed <= 6.7e-3);
  * shift block (4 / 8 units), stage 1 (48..56 units): max-abs <= 4e-2 * scale (observed <= 1.96e-2 for both);
  * whole network (synthetic checkpoint recipe v2, weights.py): the contract of BASELINE.json / SURVEY.md 8c:
        PSNR(hip, reference fp32 output) >= 48 dB   and   |PSNR(hip, gt) - PSNR(ref, gt)| <= 0.01 dB,
    both against the fp32 reference output DIRECTLY, for fp16 and bf16 modules alike: the restored frames are taken from conv_last's
    fp32 accumulators (GShiftNet.forward_fp32_out) -- a bf16 image TENSOR quantises intensities above 0.5 to 1/256 steps, which alone
    moves PSNR-vs-gt by 0.02 .. 0.06 dB -- plus a bound on the network's CORRECTION, rel-RMS of (out - x) against (ref - x) <= CORR_TOL,
    which a wrong tap / slab / gate half fails even though conv_last's small gain hides it from the 48 dB bound.
The fp32 engine (tests/test_gpu_fp32.py) pins the shared control flow to 1e-4 independently of all of this.
Every measured error is also appended to gpurun_out/parity_report.json.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import shiftnet_oracle as O
from shiftnet_amd import prep, synth
from shiftnet_amd.spec import VARIANTS, shift_table
from shiftnet_amd.weights import synth_state_dict
from prelu_edge import edge_state_dict, set_slope

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report_file():
    yield
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "parity_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


def bf(t):
    return t.to(torch.bfloat16).float()


def to_dev(t_nchw, cs=None):
    """fp32 NCHW cpu -> bf16 NHWC device [T,H,W,cs] with zero pad channels."""
    T, c, H, W = t_nchw.shape
    cs = prep.ceil8(c) if cs is None else cs
    a = torch.zeros((T, H, W, cs), dtype=torch.bfloat16)
    a[..., :c] = t_nchw.permute(0, 2, 3, 1).to(torch.bfloat16)
    return a.to(DEV)


def to_cpu(t_nhwc, c):
    return t_nhwc[..., :c].float().cpu().permute(0, 3, 1, 2).contiguous()


def check(name, got, ref, tol):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(1.0, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    rel_rms = ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-12)).item()
    REPORT.append({"name": name, "max_abs": err, "scale": scale, "rel_rms": rel_rms, "tol": tol})
    assert np.isfinite(err) and err <= tol * scale, f"{name}: max-abs {err:.4g} > {tol} * {scale:.4g} (rel rms {rel_rms:.3g})"


@pytest.fixture(scope="module")
def engines():
    from shiftnet_amd.engine import Engine, Plan
    cache = {}

    def get(name):
        if name not in cache:
            sd = synth_state_dict(name)
            cache[name] = (Engine(Plan(VARIANTS[name], sd, DEV)), sd)
        return cache[name]
    return get


def act(t, c):
    from shiftnet_amd.engine import Act
    return Act(t, c)


# ---------------------------------------------------------------------------------------------------------------
def test_mfma_lane_layout():
    from shiftnet_amd import lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(3)
    a = bf(torch.randn(16, 32, generator=g)); b = bf(torch.randn(32, 16, generator=g))
    a[3, 7] = 9.0; b[5, 11] = -7.0                      # asymmetric markers
    ad, bd = a.to(DEV), b.to(DEV)
    d = torch.zeros(16, 16, device=DEV)
    L.check(lib.sn_selftest_mfma(ad.data_ptr(), bd.data_ptr(), d.data_ptr(), torch.cuda.current_stream().cuda_stream), "selftest")
    torch.cuda.synchronize()
    check("mfma_selftest", d, a @ b, 1e-5)


@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_deblur1", "gshift_denoise2", "gshift_denoise1"])      # C = 64 circular / 80 keep / 64 keep / 80 keep
@pytest.mark.parametrize("hw", [(24, 24), (6, 10)])
def test_gsts_gather_bit_exact(name, hw):
    from shiftnet_amd import lib as L
    lib = L.load()
    V = O.VARIANTS[name]
    C, T, (h, w) = V.c1, 4, hw
    x = bf(torch.from_numpy(synth.unit_noise((T, C, h, w), seed=41)))
    xd = to_dev(x)
    offs = prep.shift_offsets_i8(shift_table(C)).to(DEV)
    for mode, rev in ((1, False), (2, True)):
        u = torch.empty((T, h, w, C + C // 2), dtype=torch.bfloat16, device=DEV)
        s = L.UnitSrc(xd.data_ptr(), T, h, w, C, mode, 1 if V.wrap else 0)
        L.check(lib.sn_gsts_gather(ctypes.byref(s), offs.data_ptr(), u.data_ptr(), torch.cuda.current_stream().cuda_stream), "gather")
        ref = O.gsts_gather(x, rev, V.wrap)
        got = to_cpu(u, C + C // 2)
        assert torch.equal(got, ref), f"gather {name} mode {mode}"
        y = torch.empty((T, h, w, C), dtype=torch.bfloat16, device=DEV)
        s2 = L.UnitSrc(xd.data_ptr(), T, h, w, C, mode, 0)
        L.check(lib.sn_temporal_roll(ctypes.byref(s2), y.data_ptr(), torch.cuda.current_stream().cuda_stream), "roll")
        assert torch.equal(to_cpu(y, C), O.temporal_roll(x, rev, False)[0])


CONV_CASES = {
    # name: (variant, plan key, weight key prefix, cins, stride, pad, kwargs)
    "in3": ("gshift_deblur2", "feat_extract.0", "feat_extract.0.", [3], 1, 1),
    "c14": ("gshift_deblur2", "conv_trans", "conv_trans.", [14], 1, 1),
    "cat3": ("gshift_deblur2", "rconcat", "rconcat.", [14, 14, 14], 1, 1),
    "s2_14": ("gshift_deblur2", "orb1.down12.down", "orb1.down12.down.", [14], 2, 1),
    "s2_64": ("gshift_deblur2", "stage1.down12.down", "stage1.down12.down.", [64], 2, 1),
    "k2s2": ("gshift_deblur2", "stage1.down01", "stage1.down01.0.", [14], 2, 0),
    "c64": ("gshift_deblur2", "stage1.skip_attn1.body.0", "stage1.skip_attn1.body.0.", [64], 1, 1),
    "c18": ("gshift_deblur2", "orb1.encoder_level2.0.body.0", "orb1.encoder_level2.0.body.0.", [18], 1, 1),
    "c22": ("gshift_deblur2", "orb1.encoder_level3.0.body.0", "orb1.encoder_level3.0.body.0.", [22], 1, 1),
    "c80": ("gshift_deblur1", "stage1.skip_attn1.body.0", "stage1.skip_attn1.body.0.", [80], 1, 1),
    "c36": ("gshift_deblur1", "orb1.encoder_level2.0.body.0", "orb1.encoder_level2.0.body.0.", [36], 1, 1),
    "cat2_24": ("gshift_deblur1", "stage1.conv_hr0", "stage1.conv_hr0.", [24, 24], 1, 1),
}


@pytest.mark.parametrize("case", list(CONV_CASES))
@pytest.mark.parametrize("hw", [(16, 64), (10, 36)])
def test_conv(case, hw, engines):
    name, key, wkey, cins, stride, pad = CONV_CASES[case]
    eng, sd = engines(name)
    T, (H, W) = 2, hw
    xs = [bf(torch.from_numpy(synth.unit_noise((T, c, H, W), seed=51 + i))) for i, c in enumerate(cins)]
    out = eng.conv(key, [act(to_dev(x), c) for x, c in zip(xs, cins)], stride=stride, pad=pad, prelu=0.2)
    torch.cuda.synchronize()
    ref = torch.nn.functional.conv2d(torch.cat(xs, 1), sd[wkey + "weight"], sd.get(wkey + "bias"), stride=stride, padding=pad)
    ref = torch.where(ref >= 0, ref, 0.2 * ref)
    check(f"conv_{case}_{H}x{W}", to_cpu(out.t, out.c), ref, 8e-3)
    if out.t.shape[-1] > out.c:
        assert out.t[..., out.c:].float().abs().max().item() == 0.0


@pytest.mark.parametrize("name,conv,cin,cout", [("gshift_deblur2", "stage1.up21", 64, 64), ("gshift_deblur2", "orb1.up21", 18, 14), ("gshift_deblur2", "orb1.up32", 22, 18),
                                                ("gshift_deblur1", "stage1.up21", 80, 80), ("gshift_deblur1", "orb1.up21", 36, 24), ("gshift_deblur1", "orb1.up32", 48, 36)])
@pytest.mark.parametrize("T,hw", [(2, (6, 20)), (3, (1, 1)), (1, (9, 37)), (2, (45, 80))])
def test_skip_upsample_both_forms(name, conv, cin, cout, T, hw, engines):
    """SkipUpSample (gshift_deblur1.py:341-350: bilinear x2 -> 1x1 -> + skip) in its two forms against the oracle: the 1x1 at low resolution followed by
    sn_upsample2_add (conv and interpolation commute; the default since round 6) and round 2's interpolation in the loader of a full-resolution conv.
    One-pixel maps (every source index clamps), odd sizes, pad channels (18 -> 24, 14 -> 16) that must stay zero."""
    eng, sd = engines(name)
    h, w = hw
    lo = bf(torch.from_numpy(synth.unit_noise((T, cin, h, w), seed=63)))
    sk = bf(torch.from_numpy(synth.unit_noise((T, cout, 2 * h, 2 * w), seed=64)))
    ref = O.skip_up_sample(sd, conv + ".", lo, sk)
    for lowres in (True, False):
        e = _sibling_engine(eng, skip_up_lowres=lowres)
        called = []
        orig = e._call
        e._call = lambda fn, *a: (called.append(fn), orig(fn, *a))[1]
        out = e.skip_up(conv, act(to_dev(lo), cin), act(to_dev(sk), cout))
        torch.cuda.synchronize()
        assert ("sn_upsample2_add" in called) == lowres, called
        check(f"skip_up_{'lowres' if lowres else 'loader'}_{name}_{conv}_{T}x{h}x{w}", to_cpu(out.t, cout), ref, 8e-3)
        if out.t.shape[-1] > cout:
            assert out.t[..., cout:].float().abs().max().item() == 0.0


def test_conv_epilogues(engines):
    eng, sd = engines("gshift_deblur2")
    F = torch.nn.functional
    T, H, W = 2, 12, 40
    # residual + pooled sums
    x = bf(torch.from_numpy(synth.unit_noise((T, 14, H, W), seed=61)))
    r = bf(torch.from_numpy(synth.unit_noise((T, 14, H, W), seed=62)))
    out, pool, npix = eng.conv("conv_trans", [act(to_dev(x), 14)], res=act(to_dev(r), 14), pool=True)
    ref = F.conv2d(x, sd["conv_trans.weight"], sd["conv_trans.bias"], padding=1) + r
    check("conv_res", to_cpu(out.t, 14), ref, 8e-3)
    check("conv_pool", pool.sum(1)[:, :14] / npix, ref.mean((2, 3)), 8e-3)
    # bilinear x2 + 1x1 + skip  (SkipUpSample)
    lo = bf(torch.from_numpy(synth.unit_noise((T, 64, H // 2, W // 2), seed=63)))
    sk = bf(torch.from_numpy(synth.unit_noise((T, 64, H, W), seed=64)))
    out = eng.skip_up("stage1.up21", act(to_dev(lo), 64), act(to_dev(sk), 64))
    check("skip_up", to_cpu(out.t, 64), O.skip_up_sample(sd, "stage1.up21.", lo, sk), 8e-3)
    lo = bf(torch.from_numpy(synth.unit_noise((T, 18, H // 2, W // 2), seed=65)))
    sk = bf(torch.from_numpy(synth.unit_noise((T, 14, H, W), seed=66)))
    out = eng.skip_up("orb1.up21", act(to_dev(lo), 18), act(to_dev(sk), 14))
    check("skip_up_unet", to_cpu(out.t, 14), O.skip_up_sample(sd, "orb1.up21.", lo, sk), 8e-3)
    # pixel shuffle
    x = bf(torch.from_numpy(synth.unit_noise((T, 64, H, W), seed=67)))
    out = eng.conv("stage1.upsample0", [act(to_dev(x), 64)], out_mode=1)
    check("pixshuf", to_cpu(out.t, 14), O.pixel_shuffle_pack(sd, "stage1.upsample0.", x), 8e-3)
    assert out.t[..., 14:].float().abs().max().item() == 0.0
    # NCHW egress: conv_last + shortcut, three dtypes
    x = bf(torch.from_numpy(synth.unit_noise((T, 14, H, W), seed=68)))
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        sc = torch.rand(T, 3, H, W).to(dt)
        o = torch.empty((T, 3, H, W), dtype=dt, device=DEV)
        eng.conv("conv_last", [act(to_dev(x), 14)], out_mode=2, nchw_out=o, nchw_sc=sc.to(DEV))
        ref = F.conv2d(x, sd["conv_last.weight"], None, padding=2) + sc.float()
        check(f"conv_last_{dt}", o, ref, 8e-3)
    # ingest
    from shiftnet_amd import lib as L
    xin = torch.rand(T, 3, H, W)
    x8 = torch.empty((T, H, W, 8), dtype=torch.bfloat16, device=DEV)
    xd = xin.half().to(DEV)
    L.check(eng.lib.sn_ingest(xd.data_ptr(), L.SN_F16, None, x8.data_ptr(), T, 3, H, W, torch.cuda.current_stream().cuda_stream), "ingest")
    assert torch.equal(to_cpu(x8, 3), xin.half().to(torch.bfloat16).float())
    assert x8[..., 3:].float().abs().max().item() == 0.0


@pytest.mark.parametrize("name,pre,c", [("gshift_deblur2", "stage1.concat.", 14), ("gshift_deblur2", "stage1.skip_attn1.", 64),
                                        ("gshift_deblur2", "orb1.encoder_level2.1.", 18), ("gshift_deblur1", "stage1.skip_attn1.", 80),
                                        ("gshift_denoise2", "stage1.concat.", 14), ("gshift_deblur1", "stage1.concat.", 24),
                                        ("gshift_deblur1", "orb1.encoder_level2.0.", 36), ("gshift_deblur1", "orb1.encoder_level3.0.", 48)])
@pytest.mark.parametrize("hw", [(20, 44), (13, 70), (2, 3)])
def test_cab(name, pre, c, hw, engines):
    """CAB (two convs, closed-form CALayer, scale / residual epilogue) incl. ragged tiles, a map smaller than one tile and the second
    residual of the last orb / rorb."""
    eng, sd = engines(name)
    x = bf(torch.from_numpy(synth.unit_noise((3, c, hw[0], hw[1]), seed=71)))
    e = bf(torch.from_numpy(synth.unit_noise((3, c, hw[0], hw[1]), seed=72)))
    ref = O.cab(sd, pre, x)
    out = eng.cab(pre, act(to_dev(x), c))
    check(f"cab_{name}_{pre}_{hw[0]}x{hw[1]}", to_cpu(out.t, c), ref, 8e-3)
    if out.t.shape[-1] > c:
        assert out.t[..., c:].float().abs().max().item() == 0.0
    out2 = eng.cab(pre, act(to_dev(x), c), act(to_dev(e), c))
    check(f"cab_extra_{name}_{pre}_{hw[0]}x{hw[1]}", to_cpu(out2.t, c), ref + e, 8e-3)


@pytest.mark.parametrize("name,pre,c", [("gshift_deblur2", "stage1.concat.", 14), ("gshift_deblur2", "orb1.encoder_level2.1.", 18),
                                        ("gshift_deblur2", "orb1.encoder_level3.1.", 22), ("gshift_deblur1", "stage1.concat.", 24),
                                        ("gshift_denoise1", "stage1.encoder_level0.", 24)])
@pytest.mark.parametrize("T,hw", [(3, (45, 150)), (2, (24, 40)), (2, (8, 32)), (1, (16, 64)), (3, (2, 3)), (2, (37, 33)), (1, (9, 34))])
def test_fused_cab_is_bit_identical_to_the_two_launch_form(name, pre, c, T, hw, engines):
    """csrc/sn_cabf.hip: statistics pass (channel sums + border lines of mid, nothing else stored) -> closed-form CALayer -> one kernel with `mid` in
    LDS.  Same operand layouts, k order, accumulation order and roundings as sn_conv2d twice, so the result must be BIT-IDENTICAL to the two-launch
    form, for both tile heights, with and without the second residual, on interior tiles, ragged right / bottom tiles, maps smaller than a tile
    and one-tile maps whose ring lies entirely outside the image; and within the CAB tolerance of the CPU oracle (gshift_deblur1.py:141-156)."""
    eng, sd = engines(name)
    two = _sibling_engine(eng, cab_fused="0", conv_tiles=True)      # (the streaming conv kernel adds the channel sums in another order)
    x = bf(torch.from_numpy(synth.unit_noise((T, c, hw[0], hw[1]), seed=73)))
    e = bf(torch.from_numpy(synth.unit_noise((T, c, hw[0], hw[1]), seed=74)))
    xa, ea = act(to_dev(x), c), act(to_dev(e), c)
    ref0 = two.cab(pre, xa).t
    ref1 = two.cab(pre, xa, ea).t
    for rows in ("8", "16"):
        fz = _sibling_engine(eng, cab_fused=rows)
        called = []
        orig = fz._call
        fz._call = lambda fn, *a: (called.append(fn), orig(fn, *a))[1]
        got0 = fz.cab(pre, xa).t
        got1 = fz.cab(pre, xa, ea).t
        torch.cuda.synchronize()
        assert called.count("sn_cab_fused") == 2 and "sn_conv2d" not in called, called      # the fused path really ran
        assert torch.equal(ref0, got0) and torch.equal(ref1, got1), (name, pre, rows, T, hw,
                                                                     (ref0.float() - got0.float()).abs().max().item(), (ref1.float() - got1.float()).abs().max().item())
    check(f"cab_fused_{name}_{pre}_{T}x{hw[0]}x{hw[1]}", to_cpu(got0, c), O.cab(sd, pre, x), 8e-3)
    check(f"cab_fused_extra_{name}_{pre}_{T}x{hw[0]}x{hw[1]}", to_cpu(got1, c), O.cab(sd, pre, x) + e, 8e-3)
    if got0.shape[-1] > c:
        assert got0[..., c:].float().abs().max().item() == 0.0


@pytest.mark.parametrize("name,pre,c", [("gshift_deblur2", "stage1.concat.", 14), ("gshift_deblur2", "orb1.encoder_level2.1.", 18),
                                        ("gshift_deblur2", "orb1.encoder_level3.1.", 22), ("gshift_deblur1", "stage1.concat.", 24)])
@pytest.mark.parametrize("T,hw", [(3, (45, 150)), (2, (24, 40)), (2, (8, 32)), (1, (16, 64)), (3, (2, 3)), (2, (37, 33)), (5, (72, 200)), (1, (360, 640))])
@pytest.mark.parametrize("depth,wgs,wlds", [(0, 0, 0), (3, 0, 0), (0, 1, 0), (0, 0, 1)])
def test_streaming_fused_cab_is_bit_identical_to_the_two_launch_form(name, pre, c, T, hw, depth, wgs, wlds, engines):
    """csrc/sn_conv3p.hip cabp_kernel: statistics pass on the streaming conv (MODE 3) -> closed-form CALayer -> ONE persistent kernel that keeps
    `mid` in LDS (loader wave + LDS-DMA, conv1 on the ring, conv2 from mid, scale + x + store).  Operand layouts, k order and roundings are those of
    the two-launch streaming form, so the result must be BIT-IDENTICAL to it -- interior tiles, ragged right / bottom tiles, maps smaller than a
    tile, chunks crossing column and frame boundaries, both prefetch depths, conv2's weights in registers or LDS -- and within the CAB tolerance of the CPU oracle
    (gshift_deblur1.py:141-156)."""
    eng, sd = engines(name)
    two = _sibling_engine(eng, cab_fused="0", conv_tiles=False, conv_stream_all=True, conv_wgs=wgs)
    fz = _sibling_engine(eng, cab_fused="p", conv_tiles=False, conv_depth=depth, conv_wgs=wgs, conv_dbg=wlds)     # wlds: both weight sets in LDS
    x = bf(torch.from_numpy(synth.unit_noise((T, c, hw[0], hw[1]), seed=76)))
    xa = act(to_dev(x), c)
    ref = two.cab(pre, xa).t
    called = []
    orig = fz._call
    fz._call = lambda fn, *a: (called.append(fn), orig(fn, *a))[1]
    got = fz.cab(pre, xa).t
    torch.cuda.synchronize()
    assert called.count("sn_cab_fused") == 1 and "sn_conv2d" not in called, called
    assert torch.equal(ref, got), (name, pre, T, hw, depth, wgs, (ref.float() - got.float()).abs().max().item())
    check(f"cab_streamfused_{name}_{pre}_{T}x{hw[0]}x{hw[1]}", to_cpu(got, c), O.cab(sd, pre, x), 8e-3)
    if got.shape[-1] > c:
        assert got[..., c:].float().abs().max().item() == 0.0


@pytest.mark.parametrize("name,pre,c", [("gshift_deblur2", "stage1.concat.", 14), ("gshift_deblur2", "orb1.encoder_level2.1.", 18),
                                        ("gshift_deblur2", "orb1.encoder_level3.1.", 22), ("gshift_deblur1", "stage1.concat.", 24),
                                        ("gshift_deblur1", "orb1.encoder_level2.0.", 36), ("gshift_deblur1", "orb1.encoder_level3.0.", 48),
                                        ("gshift_deblur2", "stage1.skip_attn1.", 64)])      # >= 36 channels: weight fragments staged in LDS
@pytest.mark.parametrize("T,hw", [(3, (45, 150)), (2, (24, 40)), (2, (8, 32)), (1, (16, 64)), (3, (2, 3)), (2, (37, 33)), (5, (72, 200)), (1, (360, 640))])
@pytest.mark.parametrize("wgs", [0, 1])
def test_streaming_conv_is_bit_identical_to_the_tile_kernel(name, pre, c, T, hw, wgs, engines):
    """csrc/sn_conv3p.hip (persistent workgroups, LDS-DMA loader wave, zero padding by the buffer range check) against conv3_fast_kernel: the first
    conv of a CAB (bias-free 3x3 + PReLU + channel sums) and the second one (CALayer scale + residual) must be BIT-IDENTICAL -- same operands,
    same k order -- for interior tiles, ragged right / bottom tiles, maps smaller than a tile, chunks that cross column and frame boundaries
    (wgs = 1: one workgroup per CU, long chunks; 0: the library's choice); the channel sums are the same numbers added in another order."""
    eng, sd = engines(name)
    new = _sibling_engine(eng, conv_tiles=False, conv_wgs=wgs, conv_stream_all=True)
    old = _sibling_engine(eng, conv_tiles=True)
    x = act(to_dev(bf(torch.from_numpy(synth.unit_noise((T, c, hw[0], hw[1]), seed=75)))), c)
    slope = eng.P.scalar(pre + "body.1.weight")
    m_new, p_new, _ = new.conv(pre + "body.0", [x], prelu=slope, pool=True)
    m_old, p_old, _ = old.conv(pre + "body.0", [x], prelu=slope, pool=True)
    torch.cuda.synchronize()
    assert torch.equal(m_new.t, m_old.t), (name, pre, T, hw, (m_new.t.float() - m_old.t.float()).abs().max().item())
    s_new, s_old = p_new.sum(1), p_old.sum(1)
    assert torch.isfinite(s_new).all() and (s_new - s_old).abs().max().item() <= 1e-4 * max(1.0, s_old.abs().max().item())
    ca = (0.5 + torch.rand(T, p_old.shape[2], device=DEV)).float()
    o_new = new.conv(pre + "body.2", [m_old], res=x, oscale=ca)
    o_old = old.conv(pre + "body.2", [m_old], res=x, oscale=ca)
    torch.cuda.synchronize()
    assert torch.equal(o_new.t, o_old.t), (name, pre, T, hw, (o_new.t.float() - o_old.t.float()).abs().max().item())
    check(f"conv3p_{name}_{pre}_{T}x{hw[0]}x{hw[1]}", to_cpu(m_new.t, c),
          torch.nn.functional.prelu(torch.nn.functional.conv2d(to_cpu(x.t, c), sd[pre + "body.0.weight"].to(torch.bfloat16).float(), None, padding=1),
                                    torch.tensor([slope])), 8e-3)


@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_deblur1", "gshift_denoise1"])
@pytest.mark.parametrize("T,hw", [(4, (20, 44)), (2, (16, 16)), (3, (37, 70)), (2, (64, 96)), (1, (5, 3)), (5, (90, 160))])
def test_shiftconv_on_the_matrix_cores(name, T, hw, engines):
    """K0 = CAB2.conv1(spatial_shift2(borrowed half)) (gshift_deblur1.py:470-503,223,251) as a banded GEMM over a channel-planar LDS window
    (sn_gsts_shiftconv_mfma) against the oracle -- temporal roll, 24 displacements with zero fill, depthwise 3x3 with zero padding -- and against
    the VALU kernel of rounds 1-5 (same bf16 products, another accumulation order): both directions, C = 64 and 80, maps smaller than a tile,
    ragged right / bottom tiles (the conv's padding masks on border tiles), interior tiles, several tiles per persistent workgroup."""
    from shiftnet_amd import lib as L
    eng, sd = engines(name)
    V = O.VARIANTS[name]
    C, (h, w) = V.c1, hw
    x = bf(torch.from_numpy(synth.unit_noise((T, C, h, w), seed=82)))
    xd = act(to_dev(x), C)
    blk = "stage1.decoder_level1."
    st = torch.cuda.current_stream().cuda_stream
    for mode, rev, unit in ((1, False, "encoder_level1."), (2, True, "encoder_level1_1.")):
        pre = blk + unit + "0."
        src = eng._unit_src(xd, mode)
        new = torch.full((T, h, w, C // 2), float("nan"), dtype=torch.bfloat16, device=DEV)
        old = torch.empty_like(new)
        L.check(eng.lib.sn_gsts_shiftconv_mfma(C_byref(src), eng.P.offs.data_ptr(), eng.P.units[pre]["w1"].data_ptr(), new.data_ptr(), st), "shiftconv_mfma")
        L.check(eng.lib.sn_gsts_shiftconv(C_byref(src), eng.P.offs.data_ptr(), eng.P.units[pre]["w1"].data_ptr(), old.data_ptr(), st), "shiftconv")
        torch.cuda.synchronize()
        _, hw_ref = O.temporal_roll(x, rev, V.wrap)
        hw_ref = torch.nn.functional.conv2d(O.spatial_shift(hw_ref.contiguous()), sd[pre + "conv1.weight"], padding=1, groups=C // 2)
        assert torch.isfinite(new.float()).all()
        check(f"shiftconv_mfma_{name}_{mode}_{T}x{h}x{w}", to_cpu(new, C // 2), hw_ref, 8e-3)
        # the two kernels round the same fp32 sums (up to the order of nine additions) to bf16: at most one bf16 step apart
        d = (new.float() - old.float()).abs()
        assert (d <= 2.0 ** -7 * old.float().abs().clamp_min(2.0 ** -10)).all(), d.max().item()


@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_denoise2", "gshift_deblur1", "gshift_denoise1"])
def test_gsts_pieces(name, engines):
    """shiftconv alone, then CAB2 (both directions), CAB1, a whole unit and a whole Encoder_shift_block (production chain)."""
    _gsts_pieces(engines(name), name, "")


def _gsts_pieces(eng_sd, name, tag):
    from shiftnet_amd import lib as L
    eng, sd = eng_sd
    V = O.VARIANTS[name]
    C, T, h, w = V.c1, 4, 20, 44
    x = bf(torch.from_numpy(synth.unit_noise((T, C, h, w), seed=81)))
    xd = act(to_dev(x), C)
    blk = "stage1.decoder_level1."
    for mode, rev, unit in ((1, False, "encoder_level1."), (2, True, "encoder_level1_1.")):
        pre = blk + unit + "0."
        hwb = torch.empty((T, h, w, C // 2), dtype=torch.bfloat16, device=DEV)
        src = eng._unit_src(xd, mode)
        L.check(eng.lib.sn_gsts_shiftconv(C_byref(src), eng.P.offs.data_ptr(), eng.P.units[pre]["w1"].data_ptr(), hwb.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "shiftconv")
        _, hw_ref = O.temporal_roll(x, rev, V.wrap)
        hw_ref = torch.nn.functional.conv2d(O.spatial_shift(hw_ref.contiguous()), sd[pre + "conv1.weight"], padding=1, groups=C // 2)
        check(f"shiftconv_{name}_{mode}", to_cpu(hwb, C // 2), hw_ref, 8e-3)
        out = eng.naf(pre, xd, mode)
        check(f"cab2{tag}_{name}_{mode}", to_cpu(out.t, C), O.cab2(sd, pre, O.gsts_gather(x, rev, V.wrap), V), 8e-3)
    pre = blk + "encoder_level1.1."
    out = eng.naf(pre, xd, 0)
    check(f"cab1{tag}_{name}", to_cpu(out.t, C), O.cab1(sd, pre, x, V), 8e-3)
    out = eng.gsts_unit(blk + "encoder_level1_1.", xd, True)
    check(f"unit_rev{tag}_{name}", to_cpu(out.t, C), O.gsts_unit(sd, blk + "encoder_level1_1.", x, True, V), 1.2e-2)
    out = eng.shift_block(blk, xd)
    check(f"shift_block{tag}_{name}", to_cpu(out.t, C), O.shift_block(sd, blk, x, V), 4e-2)
    # ragged sizes: partial tiles in both kernels' tilings
    x2 = bf(torch.from_numpy(synth.unit_noise((2, C, 13, 70), seed=82)))
    out = eng.gsts_unit(blk + "encoder_level1.", act(to_dev(x2), C), False)
    check(f"unit_fwd_ragged{tag}_{name}", to_cpu(out.t, C), O.gsts_unit(sd, blk + "encoder_level1.", x2, False, V), 1.2e-2)


@pytest.mark.parametrize("name,p1key", [("gshift_deblur2", "p1r"), ("gshift_deblur1", "p1r")])
@pytest.mark.parametrize("team", [0, 1])
@pytest.mark.parametrize("T,h,w", [(3, 7, 21), (2, 5, 9), (2, 13, 70), (3, 40, 200), (2, 97, 130), (1, 64, 42), (1, 3, 40), (4, 33, 64), (5, 21, 122), (2, 9, 123)])
def test_cab_phase1_fused_kernel(T, h, w, name, p1key, team, engines):
    """sn_gsts_cab2_phase1 / sn_cab1_phase1 (fused LayerNorm -> 1x1 -> dw3x3 -> gate -> RepConv -> 1x1 -> gate2) alone against the reference's g2 and its
    channel sums, CAB1 and both CAB2 directions -- the role-split kernel with the RepConv on the matrix cores (csrc/sn_phase1r.hip: C = 64 depthwise
    and C = 80 grouped, gshift_deblur1.py:157-165,183-255): maps smaller than the warm-up rows / the pixel region, one strip (w <= 64: the region
    starts AT the image edge), two border strips (61 + 61 = 122 columns exactly, and 123 = three strips), several strips, row chunks that cross
    strip and frame boundaries, teams of 4 / 2 frames in lock step with a ragged last frame block (T = 5) and one workgroup per walk (team 1).
    Per element, against a float64 interval reference that models every rounding of the kernel: tests/test_gpu_phase1_edges.py."""
    from shiftnet_amd import lib as L
    eng, sd = engines(name)
    V = O.VARIANTS[name]
    C = V.c1
    x = bf(torch.from_numpy(synth.unit_noise((T, C, h, w), seed=85 + h)))
    xd = to_dev(x)
    blk = "stage1.decoder_level1."
    st = torch.cuda.current_stream().cuda_stream

    def ref_g2(q, v):
        a = O._conv(sd, f"{q}body.0.", v)
        a = O._conv(sd, f"{q}body.1.conv_2.", a, groups=a.shape[1]) + a
        a1, a2 = a.chunk(2, dim=1)
        b1, b2 = O._conv(sd, f"{q}body.4.", O._rep_conv(sd, f"{q}body.3.", a1 * a2, groups=(C // 8 if V.grouped_rep else C))).chunk(2, dim=1)
        return b1 * torch.sigmoid(b2)
    for mode, rev, unit in ((0, False, "encoder_level1.1."), (1, False, "encoder_level1.0."), (2, True, "encoder_level1_1.0.")):
        pre = blk + unit
        with torch.no_grad():
            if mode:
                u = O.gsts_gather(x, rev, V.wrap)
                hw = bf(O._conv(sd, pre + "conv1.", u[:, C:], groups=C // 2))
                ref = ref_g2(pre, O.layer_norm_2d(torch.cat((u[:, :C], hw), 1), sd[pre + "norm.weight"], sd[pre + "norm.bias"]))
                hwd = to_dev(hw)
            else:
                ref = ref_g2(pre, O.layer_norm_2d(x, sd[pre + "norm.weight"], sd[pre + "norm.bias"]))
                hwd = None
        p1 = eng.P.units[pre][p1key]
        src = L.UnitSrc(xd.data_ptr(), T, h, w, C, mode, 1 if (V.wrap and mode) else 0)
        nblk = eng.lib.sn_phase1_pool_blocks(T, h, w)
        assert nblk >= 1
        g2 = torch.full((T, h, w, C), float("nan"), dtype=torch.bfloat16, device=DEV)
        pool = torch.full((T, nblk, C), float("nan"), dtype=torch.float32, device=DEV)
        L.check(L.cab_phase1(eng.lib, src, hwd.data_ptr() if hwd is not None else None, p1["desc"], g2.data_ptr(), pool.data_ptr(), st,
                             None, L.Phase1Opts(None, 0, team)), "phase 1")
        check(f"phase1_g2_{name}_{p1key}_{mode}_{T}x{h}x{w}", to_cpu(g2, C), ref, 1.2e-2)
        sums = pool.sum(1).cpu()
        rs = ref.sum((2, 3))
        assert torch.isfinite(sums).all() and (sums - rs).abs().max().item() <= 1e-2 * max(1.0, rs.abs().max().item())


def C_byref(s):
    return ctypes.byref(s)


@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_deblur1", "gshift_denoise1"])
def test_phase1_results_do_not_depend_on_launch_geometry(name, engines):
    """csrc/sn_phase1r.hip: pool rows are per (frame, strip, block of 8 image rows) and every walk computes a row from the same operands in the
    same order, so g2, the partial channel sums and the squeeze-excite scale are BIT-IDENTICAL whatever the launch looks like: the library's
    own team size, teams of 1 / 2 / 8 workgroups (other chunk boundaries, other walks per workgroup), and the frames launched in three
    separate frame ranges -- what a temporally split window, the halo-overlap pieces and the frame wavefront rely on."""
    from shiftnet_amd import lib as L
    eng, sd = engines(name)
    V = O.VARIANTS[name]
    C_, T, h, w = V.c1, 5, 45, 150                                  # 3 strips, 6 row blocks (the last one short), a ragged last frame block for teams of 2 / 8
    x = torch.from_numpy(synth.unit_noise((T, h, w, C_), seed=17)).to(torch.bfloat16).to(DEV)
    hwb = torch.from_numpy(synth.unit_noise((T, h, w, C_ // 2), seed=18)).to(torch.bfloat16).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    nblk = eng.lib.sn_phase1_pool_blocks(T, h, w)
    for mode, unit in ((0, "encoder_level1.1."), (2, "encoder_level1_1.0.")):
        pre = "stage1.decoder_level1." + unit
        p1, q = eng.P.units[pre]["p1r"], eng.P.cas[pre + "ca2"]
        ca1 = None
        if V.denoise:                                               # the inner scale of the denoisers' second pass: any fixed values do
            ca1 = (0.5 + torch.rand(T, C_, device=DEV)).float()

        def run(team, ranges):
            g2 = torch.full((T, h, w, C_), float("nan"), dtype=torch.bfloat16, device=DEV)
            pool = torch.full((T, nblk, C_), float("nan"), dtype=torch.float32, device=DEV)
            ca = torch.full((T, C_), float("nan"), dtype=torch.float32, device=DEV)
            tickets = torch.zeros((T,), dtype=torch.int32, device=DEV)
            for t0, nt in ranges:
                src = L.UnitSrc(x.data_ptr(), T, h, w, C_, mode, 1 if (mode and V.wrap) else 0, None, t0, nt)
                se = L.SeFold(q["wa"].data_ptr(), q["wb"].data_ptr(), q["c"], q["cr"], tickets.data_ptr(), ca.data_ptr(), None)
                opt = L.Phase1Opts(ca1.data_ptr() if ca1 is not None else None, 0, team)
                L.check(L.cab_phase1(eng.lib, src, hwb.data_ptr() if mode else None, p1["desc"], g2.data_ptr(), pool.data_ptr(), st, se, opt), "phase 1")
            torch.cuda.synchronize()
            assert int(tickets.abs().sum()) == 0
            return g2, pool, ca
        ref = run(0, [(0, 0)])
        assert torch.isfinite(ref[0].float()).all() and torch.isfinite(ref[1]).all() and torch.isfinite(ref[2]).all()
        for team, ranges in ((1, [(0, 0)]), (2, [(0, 0)]), (8, [(0, 0)]), (0, [(1, 3), (0, 1), (4, 1)]), (1, [(3, 2), (0, 3)])):
            got = run(team, ranges)
            for a, b, what in zip(ref, got, ("g2", "pool", "ca")):
                assert torch.equal(a, b), (name, mode, team, ranges, what)


@pytest.mark.parametrize("name,T,h,w", [("gshift_deblur2", 3, 184, 328), ("gshift_deblur2", 3, 40, 200), ("gshift_deblur1", 3, 184, 328),
                                        ("gshift_deblur1", 3, 40, 200), ("gshift_denoise1", 3, 136, 224)])
def test_unit_parity_at_production_tile_counts(name, T, h, w, engines):
    """A whole GSTS unit against the oracle at sizes where the persistent, XCD-partitioned schedule of the matrix-core
    stencil kernel really loops: 184x328x3 = 414 tiles of 64x8 (> 256 workgroups, ragged right and bottom tiles, a
    segment boundary in the middle of a frame); 40x200x3 = 60 tiles (a workgroup count that is not a multiple of 8, so
    the XCD partition falls back to one segment); gshift_denoise1 at 3 x 136 x 224 = level 1 of the denoise CLI's quadrants (config 4): the
    two-kernel phase 1 with the inner CALayer2 and the grouped RepConv kernel's persistent walk over 238 tiles."""
    eng, sd = engines(name)
    V = O.VARIANTS[name]
    x = bf(torch.from_numpy(synth.unit_noise((T, V.c1, h, w), seed=83)))
    blk = "stage1.decoder_level1."
    for unit, rev in (("encoder_level1.", False), ("encoder_level1_1.", True)):
        out = eng.gsts_unit(blk + unit, act(to_dev(x), V.c1), rev)
        check(f"unit_{'rev' if rev else 'fwd'}_{name}_{T}x{h}x{w}", to_cpu(out.t, V.c1), O.gsts_unit(sd, blk + unit, x, rev, V), 1.2e-2)


@pytest.mark.parametrize("name,G", [("gshift_deblur2", 2), ("gshift_deblur2", 3), ("gshift_deblur1", 2), ("gshift_denoise1", 3)])
def test_frame_wavefront_schedule_is_bit_identical(name, G, engines):
    """SURVEY.md 8 f2 (Engine.shift_chain, SN_SCHEDULE=frame): the units of consecutive Encoder_shift_blocks issued per frame group in dependency
    order -- forward units wait for the group before, reverse units for the group after, deblur2's circular roll closes the ring (the first
    group of a forward unit is then issued LAST) -- against the unit-major order: the whole stage 1 (every chain of every pyramid level,
    with the convs / CABs between them) must be bit-identical, for groups that divide T = 7 unevenly."""
    eng, sd = engines(name)
    V = O.VARIANTS[name]
    wave = _sibling_engine(eng, schedule="frame", frame_group=G)
    x0 = bf(torch.from_numpy(synth.unit_noise((7, V.c0, 24, 40), seed=93)))
    a = eng.stage1(act(to_dev(x0), V.c0)).t
    b = wave.stage1(act(to_dev(x0), V.c0)).t
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    with torch.no_grad():                                       # ... and against the CPU oracle, at stage 1's own tolerance (test_unet_and_stage1)
        check(f"stage1_frame_wavefront_{name}_G{G}", to_cpu(b, V.c0), O.stage1(sd, x0, V), 4e-2)
    # ... and the launch order really was a wavefront: the second unit started before the first one had finished
    order = []
    orig = wave.naf
    wave.naf = lambda pre, x, mode, **kw: (order.append((pre, kw.get("frames"))), orig(pre, x, mode, **kw))[1]
    wave.shift_chain(["stage1.decoder_level1.", "stage1.decoder_level1_1."], act(to_dev(bf(torch.from_numpy(synth.unit_noise((7, V.c1, 12, 20), seed=94)))), V.c1))
    first = [i for i, (pre, fr) in enumerate(order) if pre == "stage1.decoder_level1.encoder_level1_1.0."][0]      # second unit's first launch
    last0 = [i for i, (pre, fr) in enumerate(order) if pre == "stage1.decoder_level1.encoder_level1.1."][-1]       # first unit's last launch
    assert first < last0 and all(fr is not None for _, fr in order)


@pytest.mark.parametrize("name,ng", [("gshift_deblur2", 2), ("gshift_deblur2", 3), ("gshift_deblur1", 2), ("gshift_denoise1", 3), ("gshift_denoise2", 2)])
def test_streams_schedule_is_bit_identical_and_matches_the_oracle(name, ng, engines):
    """Engine._shift_chain_streams (SN_SCHEDULE=streams): every frame group runs its chain of GSTS launches on its own HIP stream, ordered against
    the neighbouring group only by the events of engine.stream_plan (one borrowed boundary frame per shifted unit; a ring of three buffer sets).
    The whole stage 1 must be bit-identical to the unit-major order on one stream AND within stage 1's tolerance of the CPU oracle; repeated, with
    uneven groups of T = 7, for the ring (deblur2), the kept boundary and the denoisers' two passes."""
    eng, sd = engines(name)
    V = O.VARIANTS[name]
    par = _sibling_engine(eng, schedule="streams", stream_groups=ng, STREAMS_MIN_PXF=0)
    x0 = bf(torch.from_numpy(synth.unit_noise((7, V.c0, 24, 40), seed=95)))
    a = eng.stage1(act(to_dev(x0), V.c0)).t
    launches = []
    orig = par._shift_chain_streams
    par._shift_chain_streams = lambda pres, x, n: (launches.append(n), orig(pres, x, n))[1]
    for rep in range(3):
        b = par.stage1(act(to_dev(x0), V.c0)).t
        torch.cuda.synchronize()
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), (name, ng, rep)
    assert launches and all(n == ng for n in launches)          # the chains really took the streams path
    with torch.no_grad():
        check(f"stage1_streams_{name}_ng{ng}", to_cpu(b, V.c0), O.stage1(sd, x0, V), 4e-2)
    # a larger level-1 chain where the launches are long enough to really run concurrently (12 units, 3 x 4 or 8)
    xs = act(to_dev(bf(torch.from_numpy(synth.unit_noise((6, V.c1, 96, 160), seed=96)))), V.c1)
    pres = ["stage1.decoder_level1.", "stage1.decoder_level1_1."]
    ya = eng.shift_chain(pres, xs).t
    for rep in range(3):
        yb = par.shift_chain(pres, xs).t
        torch.cuda.synchronize()
        assert torch.equal(ya, yb), (name, ng, rep)


def _sibling_engine(eng, **attrs):
    """A second Engine on the SAME prepared weights with other switches (phase 1 as the bf16 chain, fewer squeeze-excite counters ...)."""
    from shiftnet_amd.engine import Engine
    e2 = Engine(eng.P)
    for k, v in attrs.items():
        setattr(e2, k, v)
    return e2


@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_denoise2", "gshift_deblur1", "gshift_denoise1"])
def test_gsts_pieces_bf16_chain(name, engines):
    """The chain the range guard falls back to (SN_PHASE1=0: sn_ln_gemm_gate + sn_dw5m_gemm_gate / sn_grp5_gemm_gate, g1 in bf16 through HBM,
    sn_ca_mlp between the phases) for all four variants: CAB2 both directions, CAB1, a unit, a whole Encoder_shift_block, ragged sizes --
    the same checks and tolerances as the fused default.  Element by element, inside float64 intervals per kernel:
    tests/test_gpu_chain_edges.py."""
    eng, sd = engines(name)
    chain = _sibling_engine(eng, phase1="0")
    assert not chain._fused_phase1(4)
    _gsts_pieces((chain, sd), name, "_chain")


@pytest.mark.parametrize("name,T,h,w", [("gshift_deblur2", 3, 184, 328), ("gshift_deblur1", 3, 184, 328), ("gshift_denoise1", 3, 136, 224)])
def test_unit_parity_bf16_chain_at_production_tile_counts(name, T, h, w, engines):
    eng, sd = engines(name)
    chain = _sibling_engine(eng, phase1="0")
    V = O.VARIANTS[name]
    x = bf(torch.from_numpy(synth.unit_noise((T, V.c1, h, w), seed=83)))
    blk = "stage1.decoder_level1."
    for unit, rev in (("encoder_level1.", False), ("encoder_level1_1.", True)):
        out = chain.gsts_unit(blk + unit, act(to_dev(x), V.c1), rev)
        check(f"unit_chain_{'rev' if rev else 'fwd'}_{name}_{T}x{h}x{w}", to_cpu(out.t, V.c1), O.gsts_unit(sd, blk + unit, x, rev, V), 1.2e-2)


@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_denoise1"])
def test_gsts_pieces_with_more_frames_than_squeeze_excite_counters(name, engines):
    """T > Engine.MAX_TICKETS (4096 frames in production; 2 here): the deblur models keep the fused kernel and finish CALayer2 with sn_ca_mlp,
    the denoisers -- whose two-pass phase 1 needs the fold for the inner scale -- run the chain (engine.py: _fused_phase1)."""
    eng, sd = engines(name)
    few = _sibling_engine(eng, MAX_TICKETS=2)
    assert few._fused_phase1(4) == (not O.VARIANTS[name].denoise)
    _gsts_pieces((few, sd), name, "_fewtickets")


def _hot_state_dict(name, gain):
    """The synthetic checkpoint with the first 1x1 of every CAB2 / CAB1 of stage 1 times `gain`: `a` grows by gain, g1 = a1 a2 by gain^2."""
    sd = synth_state_dict(name)
    for k in list(sd):
        if k.startswith("stage1.") and k.endswith(".body.0.weight") and sd[k].shape[-1] == 1 and sd[k].shape[0] == 2 * O.VARIANTS[name].c1:
            sd[k] = sd[k] * gain
    return sd


@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_denoise1"])
def test_range_guard_moves_a_module_to_the_bf16_chain(name):
    """ADVICE r04 / VERDICT r04 item 3b: a checkpoint whose activations leave the fp16 range of the fused phase-1 kernel (body.0.weight x 300:
    g1 = a1 a2 2^-4 ~ 1e5 .. 1e6 overflows fp16) must not produce inf / NaN silently.  The squeeze-excite reductions flag the non-finite channel
    sums; forward() then warns, switches the module to the two-kernel chain (g1 in bf16) for good and recomputes the window: the result is
    finite, bit-identical to a module that ran the chain from the start, and within the block tolerance of the oracle on the same weights."""
    import importlib
    import warnings
    from shiftnet_amd.engine import Engine, Plan
    mod = importlib.import_module(f"basicsr.models.archs.{name}")
    V = O.VARIANTS[name]
    sd = _hot_state_dict(name, 300.0)
    T, H, W = 5, 32, 48
    blur, _ = synth.blurred_clip(T, H, W, seed=3)
    x = O.frames_to_tensor(list(blur)).bfloat16().cuda()
    nm = torch.full((1, T, 1, H, W), 30.0 / 255.0, device="cuda", dtype=torch.bfloat16) if V.denoise else None
    net = mod.GShiftNet(future_frames=2, past_frames=2)
    net.load_state_dict(sd, strict=True)
    net = net.to(torch.bfloat16).cuda().eval()
    eng = net.prepare()
    assert eng.range_guard and eng._fused_phase1(T)
    with torch.no_grad():
        with pytest.warns(UserWarning, match="fp16 range"):
            y = net(x, nm) if V.denoise else net(x)
        assert eng.fallbacks == 1 and eng.phase1 == "0" and torch.isfinite(y.float()).all()
        with warnings.catch_warnings():
            warnings.simplefilter("error")                   # the second window runs the chain quietly
            y2 = net(x, nm) if V.denoise else net(x)
        assert torch.equal(y, y2) and eng.fallbacks == 1
        # a module on the chain from the start
        chain = Engine(Plan(VARIANTS[name], {k: v.bfloat16() for k, v in sd.items()}, DEV))
        chain.phase1 = "0"
        y3 = chain.forward(x[0], nm[0] if nm is not None else None, 2, 2)
        assert torch.equal(y, y3)
        # and the chain is right on these weights.  One CAB1 against the oracle, judged per element: with pre-activations of ~1e5 SimpleGate2's
        # sigmoid is a step function, so the few elements whose b2 sits within a bf16 rounding of zero flip by their full magnitude (a longer
        # chain of such blocks is chaotic for ANY arithmetic: a shift block of 8 decorrelates completely) -- 90 % within the block tolerance
        # (measured 95.6 % / deblur2; a wrong tap, slab or gate half leaves ~0 %)
        C = V.c1
        xb = bf(torch.from_numpy(synth.unit_noise((3, C, 20, 44), seed=81)))
        blk = "stage1.decoder_level1."
        pre = blk + "encoder_level1.1."
        out = to_cpu(chain.naf(pre, act(to_dev(xb), C), 0).t, C)
        ref = O.cab1({k: v.bfloat16().float() for k, v in sd.items()}, pre, xb, V)
        assert torch.isfinite(out).all()
        frac = ((out - ref).abs() <= 8e-3 * ref.abs().max()).float().mean().item()
        REPORT.append({"name": f"cab1_hot_chain_{name}", "fraction_within_8e-3_scale": frac, "scale": ref.abs().max().item()})
        assert frac >= 0.90, frac
        # the fused kernel on the same block does overflow (otherwise this test would not test the guard)
        hot = Engine(chain.P)
        hot.range_guard = False
        bad = hot.shift_block(blk, act(to_dev(xb), C)).t.float()
        assert not torch.isfinite(bad).all()


def test_range_guard_async_mode_and_explicit_fused_request():
    """(a) SN_RANGE_GUARD=async -- the flag travels to pinned host memory behind the forward and is read when the NEXT forward starts:
    no device sync at the end of a window; the tripped window is reported (it was handed out already), the module moves to the chain and the
    next window equals a module that ran the chain from the start.  (b) an explicit SN_PHASE1=r is honoured: a warning, no switch.
    (c) Engine.guard_scope (the denoise CLIs' four quadrants): no check inside, one at the exit, `tripped` asks the caller for a second run."""
    import warnings
    from shiftnet_amd.engine import Engine, Plan
    name = "gshift_deblur2"
    sd = {k: v.bfloat16() for k, v in _hot_state_dict(name, 300.0).items()}
    T, H, W = 5, 32, 48
    blur, _ = synth.blurred_clip(T, H, W, seed=3)
    x = O.frames_to_tensor(list(blur)).bfloat16().cuda()[0]
    P = Plan(VARIANTS[name], sd, DEV)
    chain = Engine(P)
    chain.phase1 = "0"
    ref = chain.forward(x, None, 2, 2)
    with torch.no_grad():
        a = Engine(P)
        a.range_guard_async = True
        with warnings.catch_warnings():
            warnings.simplefilter("error")                   # the tripped window itself is handed out without a word (and without a sync)
            a.forward(x, None, 2, 2)
        assert a.phase1 != "0" and a._bad_pending
        with pytest.warns(UserWarning, match="already handed out"):
            y = a.forward(x, None, 2, 2)                     # the check at its start switches the module: this window runs the chain
        assert a.phase1 == "0" and a.fallbacks == 1 and torch.equal(y, ref)
        assert a.check_range_guard() is False                # the chain does not trip it
        g = Engine(P)                                        # (c) guard_scope: two forwards, ONE check at the exit, the caller runs them again
        with pytest.warns(UserWarning, match="run them again"):
            with g.guard_scope() as sc:
                with warnings.catch_warnings():
                    warnings.simplefilter("error")
                    g.forward(x, None, 2, 2)
                    g.forward(x, None, 2, 2)
        assert sc.tripped and g.phase1 == "0" and g.fallbacks == 1
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with g.guard_scope() as sc:
                y = g.forward(x, None, 2, 2)
        assert not sc.tripped and torch.equal(y, ref)
        r = Engine(P)
        r.phase1 = "r"
        with pytest.warns(UserWarning, match="asked for explicitly"):
            r.forward(x, None, 2, 2)
        assert r.phase1 == "r" and r.fallbacks == 0


@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_deblur1", "gshift_denoise1", "gshift_denoise2"])
def test_unet_and_stage1(name, engines):
    eng, sd = engines(name)
    V = O.VARIANTS[name]
    x0 = bf(torch.from_numpy(synth.unit_noise((3, V.c0, 24, 40), seed=91)))
    out = eng.tfr_unet("orb1.", act(to_dev(x0), V.c0))
    check(f"tfr_unet_{name}", to_cpu(out.t, V.c0), O.tfr_unet(sd, "orb1.", x0, V), 1.4e-2)
    out = to_cpu(eng.stage1(act(to_dev(x0), V.c0)).t, V.c0)
    with torch.no_grad():
        ref = O.stage1(sd, x0, V)
    check(f"stage1_{name}", out, ref, 4e-2)                      # absolute bound: 48..56 GSTS units + ~20 CABs in series


def _psnr(a, b):
    mse = (a.float() - b.float()).pow(2).mean().item()
    return 99.0 if mse == 0 else 10 * np.log10(1.0 / mse)


# relative RMS error of the network's correction (out - input) against the reference's: <= 2x the largest value measured on MI355X
# for the four variants (fp16 / bf16 modules, gpurun_out/parity_report.json); a wrong tap or gate half is O(1) here
CORR_TOL = 0.035


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_whole_net_vs_golden(name, dt, golden_dir):
    """The drop-in class end to end (state_dict load, .to(dtype), .to('cuda'), forward) against reference outputs."""
    import importlib
    mod = importlib.import_module(f"basicsr.models.archs.{name}")
    V = O.VARIANTS[name]
    g = np.load(os.path.join(golden_dir, f"net_{name}.npz"))
    blur, sharp = synth.blurred_clip(7, 48, 64, seed=3)
    assert synth.crc(blur) == int(g["in_crc"])
    x = O.frames_to_tensor(list(blur))
    net = mod.GShiftNet(future_frames=2, past_frames=2)
    net.load_state_dict(synth_state_dict(name), strict=True)
    net = net.to(dt).to("cuda").eval()
    nm = torch.full((1, 7, 1, 48, 64), 30.0 / 255.0) if V.denoise else None
    with torch.no_grad():
        out = net(x.to(dt).cuda(), nm.to(dt).cuda()) if V.denoise else net(x.to(dt).cuda())
    ref = torch.from_numpy(g["p2f2"])
    assert tuple(out.shape) == tuple(ref.shape) and out.dtype == dt
    out = out.float().cpu()
    gt = torch.from_numpy(sharp[2:5]).permute(0, 3, 1, 2).float() / 255
    p_oo = _psnr(out, ref)                                    # the module contract: a tensor of the module dtype
    # The CLI path: restored frames as float32 from conv_last's accumulators, the final "+ x" on the un-rounded frames
    # (GShiftNet.forward_fp32_out).  Compared with the REFERENCE's fp32 output directly, no re-definition of the reference.
    with torch.no_grad():
        kw = {"shortcut": x.cuda()}
        out32 = (net.forward_fp32_out(x.to(dt).cuda(), nm.to(dt).cuda(), **kw) if V.denoise else net.forward_fp32_out(x.to(dt).cuda(), **kw))
    assert out32.dtype == torch.float32 and tuple(out32.shape) == tuple(ref.shape)
    out32 = out32.cpu()
    p_32 = _psnr(out32, ref)
    dpsnr = abs(_psnr(out32.clamp(0, 1), gt) - _psnr(ref.clamp(0, 1), gt))
    dpsnr_tensor = abs(_psnr(out.clamp(0, 1), gt) - _psnr(ref.clamp(0, 1), gt))
    # The synthetic checkpoint makes the restored frame "input + small correction" (conv_last gain 0.01), so a PSNR against the
    # reference output alone would tolerate a badly wrong correction: bound the CORRECTION itself, relative to the reference's.
    xin = x[0, 2:5]
    corr_err = ((out32 - xin) - (ref - xin)).pow(2).mean().sqrt().item() / (ref - xin).pow(2).mean().sqrt().item()
    REPORT.append({"name": f"net_{name}_{dt}", "psnr_vs_ref": p_oo, "psnr_fp32_out_vs_ref": p_32, "ref_own_bf16_psnr": float(g["p2f2_ref_bf16_psnr"]),
                   "delta_psnr_gt": dpsnr, "delta_psnr_gt_module_dtype_tensor": dpsnr_tensor, "correction_rel_rms_err": corr_err,
                   "max_abs": (out32 - ref).abs().max().item()})
    assert p_oo >= 48.0 and p_32 >= 48.0 and dpsnr <= 0.01, (name, dt, p_oo, p_32, dpsnr, dpsnr_tensor)
    assert corr_err <= CORR_TOL, (name, dt, corr_err)
    # The module contract itself: forward() takes and returns tensors of the module dtype, which quantises the frames for ANY implementation.
    # Against the reference under the same I/O quantisation -- the fp32 oracle on the clip rounded to the module dtype, its output rounded to
    # it: what upstream's half-precision CLI computes (test_deblur.py:128-143) -- the 0.01 dB bound holds for the module tensor too.
    with torch.no_grad():
        ref_q = O.forward(V, synth_state_dict(name), x.to(dt).float(), nm.to(dt).float() if V.denoise else None, 2, 2).to(dt).float()
    dpsnr_q = abs(_psnr(out.clamp(0, 1), gt) - _psnr(ref_q.clamp(0, 1), gt))
    REPORT[-1]["delta_psnr_gt_vs_reference_in_module_dtype"] = dpsnr_q
    assert dpsnr_q <= 0.01, (name, dt, dpsnr_q)
    # default past/future of the ctor
    net2 = mod.GShiftNet()
    net2.load_state_dict(synth_state_dict(name), strict=True)
    net2 = net2.to(dt).to("cuda").eval()
    with torch.no_grad():
        out2 = net2(x.to(dt).cuda(), nm.to(dt).cuda()) if V.denoise else net2(x.to(dt).cuda())
    assert _psnr(out2.float().cpu(), torch.from_numpy(g["default"])) >= 48.0
    # T <= past+future -> empty
    with torch.no_grad():
        e = net(x[:, :4].to(dt).cuda(), nm[:, :4].to(dt).cuda()) if V.denoise else net(x[:, :4].to(dt).cuda())
    assert e.shape[0] == 0


def test_config1_and_cli_windows(golden_dir):
    from basicsr.models.archs.gshift_deblur2 import GShiftNet
    name = "gshift_deblur2"
    net = GShiftNet(future_frames=2, past_frames=2)
    net.load_state_dict(synth_state_dict(name), strict=True)
    net = net.to(torch.bfloat16).cuda().eval()
    g = np.load(os.path.join(golden_dir, f"config1_{name}.npz"))
    blur, _ = synth.blurred_clip(5, 256, 256, seed=5)
    with torch.no_grad():
        out = net(O.frames_to_tensor(list(blur)).bfloat16().cuda()).float().cpu()
    p = _psnr(out, torch.from_numpy(g["out"]))
    REPORT.append({"name": "config1", "psnr_vs_ref": p, "ref_own_bf16_psnr": float(g["ref_bf16_psnr"])})
    assert p >= 48.0
    g = np.load(os.path.join(golden_dir, f"windows_{name}.npz"))
    blur, _ = synth.blurred_clip(12, 32, 40, seed=7)
    outs = []
    with torch.no_grad():
        for a, _ in O.deblur_windows(12, 4):
            outs.append(net(O.frames_to_tensor(list(blur[a.start:a.stop])).bfloat16().cuda()).float().cpu())
    p = _psnr(torch.cat(outs), torch.from_numpy(g["out"]))
    REPORT.append({"name": "cli_windows", "psnr_vs_ref": p, "ref_own_bf16_psnr": float(g["ref_bf16_psnr"])})
    assert p >= 48.0


def test_full_size_properties():
    """BASELINE config 2 size (Shift-Net-s, 720p, T_in=20): size-independent properties instead of an oracle run.

    * determinism: two runs are bit identical (no atomics anywhere in the path);
    * circular-shift equivariance: deblur2 rolls frames circularly (gshift_deblur2.py:504-505) and everything else is
      per frame, so rotating the input clip by one frame rotates the restored interior frames, bit for bit;
    * finite output, restored frames stay close to the input (conv_last is small in the synthetic checkpoint).
    """
    from basicsr.models.archs.gshift_deblur2 import GShiftNet
    net = GShiftNet(future_frames=2, past_frames=2)
    net.load_state_dict(synth_state_dict("gshift_deblur2"), strict=True)
    net = net.to(torch.bfloat16).cuda().eval()
    T = 20
    blur, _ = synth.blurred_clip(T, 720, 1280, seed=9)
    x = torch.from_numpy(blur).permute(0, 3, 1, 2).unsqueeze(0).cuda().to(torch.bfloat16) / 255
    with torch.no_grad():
        y1 = net(x)
        y2 = net(x)
        yr = net(torch.roll(x, 1, dims=1))
    torch.cuda.synchronize()
    assert y1.shape == (16, 3, 720, 1280) and torch.isfinite(y1.float()).all()
    assert torch.equal(y1, y2)
    assert torch.equal(yr[1:], y1[:-1])                      # out(roll(x))[i] == out(x)[i-1]
    assert (y1.float() - x[0, 2:18].float()).abs().max().item() < 1.0


FULL_SIZE = {
    # BASELINE config 2 (the bench's headline workload): Shift-Net-s, 1280x720, one_len 16 -> T_in 20
    "config2": ("gshift_deblur2", 20, 720, 1280),
    # BASELINE config 3: Shift-Net+ deblur, 1280x720, one_len 48 -> T_in 52 (three levels, 56 GSTS units)
    "config3": ("gshift_deblur1", 52, 720, 1280),
    # BASELINE config 4: Shift-Net+ denoise sigma 30, 852x480 T=32 -> T_in 36, ONE of the CLI's 4 quadrants of 272x448
    # (inference/test_denoise.py:153-173; the four differ only in their crop)
    "config4_quadrant": ("gshift_denoise1", 36, 272, 448),
}


@pytest.mark.parametrize("cfg", list(FULL_SIZE))
def test_full_size_parity_against_fp32_engine(cfg):
    """Full-size parity for the "+" configs, where the CPU oracle would take hours: the bf16 module against the SAME module in
    float32 on the fp32 engine, which tests/test_gpu_fp32.py pins to the oracle / reference fixtures at 1e-4 on small sizes and
    which shares no kernel with the bf16 path.  Contract bound: PSNR >= 48 dB; plus determinism and finiteness.
    This is where production tile counts, three levels and ragged level-3 maps (90x160, 34x56) meet the "+" kernels."""
    import importlib
    name, T, H, W = FULL_SIZE[cfg]
    mod = importlib.import_module(f"basicsr.models.archs.{name}")
    V = O.VARIANTS[name]
    blur, _ = synth.blurred_clip(T, H, W, seed=23)
    x = torch.from_numpy(blur).permute(0, 3, 1, 2).unsqueeze(0).cuda().float() / 255
    nm = torch.full((1, T, 1, H, W), 30.0 / 255.0, device="cuda") if V.denoise else None
    net = mod.GShiftNet(future_frames=2, past_frames=2)
    net.load_state_dict(synth_state_dict(name), strict=True)
    net = net.cuda().eval()
    with torch.no_grad():
        ref = net(x, nm) if V.denoise else net(x)                        # float32 module -> fp32 engine
        net = net.to(torch.bfloat16)
        xb, nb = x.bfloat16(), (nm.bfloat16() if V.denoise else None)
        y1 = net(xb, nb) if V.denoise else net(xb)
        again = [net(xb, nb) if V.denoise else net(xb) for _ in range(2)]
    torch.cuda.synchronize()
    assert ref.dtype == torch.float32 and y1.dtype == torch.bfloat16 and y1.shape == ref.shape == (T - 4, 3, H, W)
    # bit-reproducible: no atomics, and no buffer handed back to the allocator before its last reader is launched (Engine.naf's ca1)
    assert torch.isfinite(y1.float()).all() and all(torch.equal(y1, y) for y in again)
    p = _psnr(y1.float(), ref)
    REPORT.append({"name": f"full_size_{cfg}", "psnr_bf16_vs_fp32_engine": p, "max_abs": (y1.float() - ref).abs().max().item()})
    assert p >= 48.0, (cfg, p)


def test_denoise_unit_is_reproducible_under_allocator_churn():
    """Regression for a buffer-lifetime bug of round 2: Engine.naf took `.data_ptr()` of the CALayer2 scale tensor as a temporary,
    so the caching allocator could hand its block to g2 / pool2 -- which the K3 kernel writes while still reading the scale.
    With random small allocations between calls the pre-fix code gave 316 differing runs out of 531 (tools/determinism_probe.py
    documents the search); every run must now be bit-identical."""
    from shiftnet_amd.engine import Act, Engine, Plan
    name = "gshift_denoise1"
    V = O.VARIANTS[name]
    dev = torch.device("cuda:0")
    eng = Engine(Plan(V, {k: v.bfloat16() for k, v in synth_state_dict(name).items()}, dev))
    g = torch.Generator().manual_seed(1)
    pre = "stage1.decoder_level1.encoder_level1.0."
    for (T, h, w) in ((36, 34, 56), (8, 17, 28)):
        x = Act(torch.randn(T, h, w, V.c1, generator=g).to(torch.bfloat16).to(dev), V.c1)
        for mode in (0, 1, 2):
            ref = None
            for _ in range(40):
                junk = [torch.empty(int(torch.randint(1, 600, (1,))) * 512, dtype=torch.uint8, device=dev) for _ in range(6)]
                del junk
                y = eng.naf(pre, x, mode).t
                torch.cuda.synchronize()
                if ref is None:
                    ref = y.clone()
                else:
                    assert torch.equal(ref, y), (T, h, w, mode)


@pytest.mark.parametrize("name,p1key", [("gshift_deblur2", "p1r"), ("gshift_deblur1", "p1r")])
def test_squeeze_excite_fold_matches_ca_mlp_and_is_reproducible(name, p1key, engines):
    """sn_se_fold: the last workgroup of each frame of the fused phase-1 launch finishes CALayer2 (fixed-order reduction of the partial sums
    + the MLP).  Against sn_ca_mlp on the very same partial sums (another summation order: 1e-6; sn_ca_mlp itself is held to float64 in
    tests/test_gpu_ca_kernels.py), bit-identical over repeated launches
    whichever workgroup arrives last, counters left at zero -- at a production size (6 x 360 x 640: row chunks that cross strips and frames,
    two or three walks per strip and frame) and a small one."""
    from shiftnet_amd import lib as L
    eng, sd = engines(name)
    lib, P = eng.lib, eng.P
    st = torch.cuda.current_stream().cuda_stream
    C_ = O.VARIANTS[name].c1
    for (T, h, w), reps in (((6, 360, 640), 12), ((3, 20, 44), 4)):
        x = torch.from_numpy(synth.unit_noise((T, h, w, C_), seed=7)).to(torch.bfloat16).to(DEV)
        hwb = torch.from_numpy(synth.unit_noise((T, h, w, C_ // 2), seed=8)).to(torch.bfloat16).to(DEV)
        for mode, unit in ((0, "encoder_level1.1."), (1, "encoder_level1.0.")):
            pre = "stage1.decoder_level1." + unit
            p1, q = P.units[pre][p1key], P.cas[pre + "ca2"]
            src = L.UnitSrc(x.data_ptr(), T, h, w, C_, mode, 1 if mode else 0)
            nblk = lib.sn_phase1_pool_blocks(T, h, w)
            g2 = torch.empty((T, h, w, C_), dtype=torch.bfloat16, device=DEV)
            tickets = torch.zeros((T,), dtype=torch.int32, device=DEV)
            ref = first = None
            for r in range(reps):
                pool = torch.full((T, nblk, C_), float("nan"), dtype=torch.float32, device=DEV)
                ca = torch.full((T, C_), float("nan"), dtype=torch.float32, device=DEV)
                se = L.SeFold(q["wa"].data_ptr(), q["wb"].data_ptr(), q["c"], q["cr"], tickets.data_ptr(), ca.data_ptr(), None)
                L.check(L.cab_phase1(lib, src, hwb.data_ptr() if mode else None, p1["desc"], g2.data_ptr(), pool.data_ptr(), st, se), "phase 1 + fold")
                torch.cuda.synchronize()
                assert int(tickets.abs().sum()) == 0, "counters not re-armed"
                if ref is None:
                    ref = torch.empty_like(ca)
                    L.check(lib.sn_ca_mlp(pool.data_ptr(), nblk, C_, q["c"], q["cr"], 1.0 / (h * w), q["wa"].data_ptr(), q["wb"].data_ptr(),
                                          ref.data_ptr(), T, None, st), "sn_ca_mlp")
                    torch.cuda.synchronize()
                    first = ca.clone()
                    assert torch.isfinite(ca).all() and (ca - ref).abs().max().item() <= 2e-6, (T, h, w, mode, (ca - ref).abs().max().item())
                else:
                    assert torch.equal(ca, first), (T, h, w, mode, r)


def test_hipgraph_replay_is_bit_identical_to_eager():
    """SN_GRAPH=1 path: second call captures the whole forward into a hipGraph, later calls replay it; results must be bit
    identical to the eager run and must follow the INPUT (the graph reads a static buffer the new input is copied into)."""
    import time
    from basicsr.models.archs.gshift_deblur2 import GShiftNet
    net = GShiftNet(future_frames=2, past_frames=2)
    net.load_state_dict(synth_state_dict("gshift_deblur2"), strict=True)
    net = net.to(torch.bfloat16).cuda().eval()
    blur, _ = synth.blurred_clip(8, 64, 96, seed=29)
    xa = O.frames_to_tensor(list(blur)).bfloat16().cuda()
    xb = torch.roll(xa, 2, dims=1).contiguous()
    eng = net.prepare()
    assert eng.graph_auto and not eng.use_graph              # default: replay for windows below Engine.GRAPH_AUTO_PXF pixel-frames only
    with torch.no_grad():
        d1, d2, d3 = net(xa), net(xa), net(xa)               # default policy at 8 x 64 x 96: eager, capture, replay
        assert any(isinstance(v, tuple) for v in eng._graphs.values()) and torch.equal(d1, d2) and torch.equal(d1, d3)
        big = eng.GRAPH_AUTO_PXF
        eng.GRAPH_AUTO_PXF = 8 * 64 * 96 - 1                 # ... and none above the threshold
        for v in eng._graphs.values():
            if isinstance(v, tuple):
                v[0].reset()
        eng._graphs.clear()
        net(xa); net(xa)
        assert not eng._graphs
        eng.GRAPH_AUTO_PXF = big
    eng.graph_auto = False                                   # from here on the test switches replay on and off itself
    with torch.no_grad():
        ea, eb = net(xa), net(xb)                         # eager references
        assert torch.equal(ea, d1)
        eng.use_graph = True
        try:
            outs = [net(xa), net(xa), net(xb), net(xa)]  # eager (first sight), capture, replay with another input, replay
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                net(xa)
            torch.cuda.synchronize()
            t_graph = (time.perf_counter() - t0) / 5
        finally:
            eng.use_graph = False
        t0 = time.perf_counter()
        for _ in range(5):
            net(xa)
        torch.cuda.synchronize()
        t_eager = (time.perf_counter() - t0) / 5
    assert any(isinstance(v, tuple) for v in eng._graphs.values()), "no graph was captured"
    assert torch.equal(outs[0], ea) and torch.equal(outs[1], ea) and torch.equal(outs[2], eb) and torch.equal(outs[3], ea)
    # the cache is an LRU with GRAPH_SLOTS captured graphs: a client that varies the window shape does not pin one activation pool per shape
    eng.use_graph = True
    try:
        with torch.no_grad():
            for T in (5, 6, 7):
                xs = xa[:, :T].contiguous()
                e = net(xs); c = net(xs); r = net(xs)
                assert torch.equal(e, c) and torch.equal(e, r)
            live = [k for k, v in eng._graphs.items() if isinstance(v, tuple)]
            assert len(live) == eng.GRAPH_SLOTS and live[-1][0][0] == 7
            assert torch.equal(net(xa), ea)                 # the evicted signature still works (eager again, then re-captured)
    finally:
        eng.use_graph = False
    REPORT.append({"name": "hipgraph_small_clip", "ms_eager": 1e3 * t_eager, "ms_graph": 1e3 * t_graph})


def test_cli_synthetic_runs(tmp_path):
    """The drop-in CLIs end to end on a synthetic clip with the synthetic checkpoint (deblur-small and denoise-small)."""
    from shiftnet_amd import cli
    p, s = cli.main("gshift_deblur2", ["--synthetic", "64", "96", "12", "--one_len", "4", "--dtype", "bf16",
                                       "--result_path", str(tmp_path / "d"), "--save_image"])
    assert np.isfinite(p) and 0 < s <= 1
    assert len(list((tmp_path / "d" / "synthetic").glob("*.png"))) == 8
    p, s = cli.main("gshift_denoise2", ["--synthetic", "96", "128", "9", "--sigma", "30", "--result_path", str(tmp_path / "n")])
    assert np.isfinite(p) and p > 15


def test_odd_sizes_small_variant():
    """Shift-Net-s only needs H, W % 4 == 0: 68x100 has odd level-2 maps (17x25) and ragged tiles everywhere."""
    from basicsr.models.archs.gshift_deblur2 import GShiftNet
    name = "gshift_deblur2"
    sd = synth_state_dict(name)
    net = GShiftNet(future_frames=2, past_frames=2)
    net.load_state_dict(sd, strict=True)
    net = net.to(torch.bfloat16).cuda().eval()
    blur, _ = synth.blurred_clip(6, 68, 100, seed=13)
    x = O.frames_to_tensor(list(blur))
    with torch.no_grad():
        out = net(x.bfloat16().cuda()).float().cpu()
        ref = O.forward(O.VARIANTS[name], sd, x, None, 2, 2)
        ref_b = O.forward(O.VARIANTS[name], {k: v.bfloat16() for k, v in sd.items()}, x.bfloat16(), None, 2, 2).float()
    p_hip, p_yard = _psnr(out, ref), _psnr(ref_b, ref)
    REPORT.append({"name": "odd_68x100", "psnr_vs_ref": p_hip, "cpu_bf16_oracle_psnr": p_yard})
    assert out.shape == ref.shape and p_hip >= 48.0
    with pytest.raises(ValueError):
        net(torch.zeros(1, 5, 3, 66, 100, dtype=torch.bfloat16, device="cuda"))


@pytest.mark.gpu
def test_nhwc_to_planar_bit_exact():
    """layout op of the matrix-core stencil path: [T][h][w][C] -> [T][h][C][wr], zeros in the pad columns."""
    from shiftnet_amd import lib as L
    lib = L.load()
    T, h, w, C = 2, 5, 77, 64
    x = torch.randn(T, h, w, C, device=DEV).to(torch.bfloat16)
    wr = lib.sn_planar_pitch(w)
    assert wr == 80
    xp = torch.full((T, h, C, wr), 7.0, dtype=torch.bfloat16, device=DEV)
    L.check(lib.sn_nhwc_to_planar(x.data_ptr(), xp.data_ptr(), T, h, w, C, torch.cuda.current_stream().cuda_stream), "planar")
    torch.cuda.synchronize()
    assert torch.equal(xp[..., :w], x.permute(0, 1, 3, 2))
    assert torch.count_nonzero(xp[..., w:]) == 0


@pytest.mark.parametrize("name,p1key", [("gshift_deblur2", "p1r"), ("gshift_deblur1", "p1r")])
@pytest.mark.parametrize("ratio", [20.0, 100.0])
def test_cab_phase1_layernorm_with_large_mean(name, p1key, ratio, engines):
    """The role-split fused phase 1 computes the LayerNorm statistics in TWO passes (mean, then sum (x - mean)^2) and feeds the normalised
    operand to the matrix core; the reference's LayerNorm2d (gshift_deblur1.py:17-28) on pixels whose channel mean is `ratio` times their
    standard deviation, large absolute values included, must still come out within the kernel's usual bound (a one-pass E[x^2] - mean^2 loses
    log2(ratio^2) bits there).  The input is generated as bf16-exact values so both sides see the same numbers."""
    from shiftnet_amd import lib as L
    eng, sd = engines(name)
    V = O.VARIANTS[name]
    C = V.c1
    T, h, w = 2, 24, 70
    base = torch.from_numpy(synth.unit_noise((T, C, h, w), seed=97))
    pix_mean = torch.from_numpy(synth.unit_noise((1, 1, h, w), seed=98)).sign() * ratio          # the same for every frame: the rolled halves of CAB2's input keep the ratio
    x = bf(((base + pix_mean) * 8.0))                               # |x| up to ~ 8 * (ratio + 4): 800+ at ratio 100
    hw_in = bf(torch.from_numpy(synth.unit_noise((T, C // 2, h, w), seed=99)) * 8.0 + pix_mean * 8.0)
    xd, hwd = to_dev(x), to_dev(hw_in)
    st = torch.cuda.current_stream().cuda_stream
    groups = C // 8 if V.grouped_rep else C

    def ref_g2(q, v):
        a = O._conv(sd, f"{q}body.0.", v)
        a = O._conv(sd, f"{q}body.1.conv_2.", a, groups=a.shape[1]) + a
        a1, a2 = a.chunk(2, dim=1)
        b1, b2 = O._conv(sd, f"{q}body.4.", O._rep_conv(sd, f"{q}body.3.", a1 * a2, groups=groups)).chunk(2, dim=1)
        return b1 * torch.sigmoid(b2)
    blk = "stage1.decoder_level1."
    for mode, unit in ((0, "encoder_level1.1."), (1, "encoder_level1.0.")):
        pre = blk + unit
        with torch.no_grad():
            if mode:
                u = O.gsts_gather(x, False, V.wrap)
                ref = ref_g2(pre, O.layer_norm_2d(torch.cat((u[:, :C], hw_in), 1).double(), sd[pre + "norm.weight"].double(), sd[pre + "norm.bias"].double()).float())
            else:
                ref = ref_g2(pre, O.layer_norm_2d(x.double(), sd[pre + "norm.weight"].double(), sd[pre + "norm.bias"].double()).float())
        p1 = eng.P.units[pre][p1key]
        src = L.UnitSrc(xd.data_ptr(), T, h, w, C, mode, 1 if (V.wrap and mode) else 0)
        nblk = eng.lib.sn_phase1_pool_blocks(T, h, w)
        g2 = torch.full((T, h, w, C), float("nan"), dtype=torch.bfloat16, device=DEV)
        pool = torch.zeros((T, nblk, C), dtype=torch.float32, device=DEV)
        L.check(L.cab_phase1(eng.lib, src, hwd.data_ptr() if mode else None, p1["desc"], g2.data_ptr(), pool.data_ptr(), st), "phase 1")
        check(f"phase1_ln_ratio{ratio}_{name}_{mode}", to_cpu(g2, C), ref, 1.5e-2)


def _cli_lines(path):
    """The metric part of the CLI's log lines (times differ from run to run)."""
    import glob
    import re
    out = []
    for f in sorted(glob.glob(os.path.join(path, "inference_log_*.txt"))):
        for ln in open(f):
            if ln.startswith(">"):
                out.append(re.sub(r" pre_time:.*", "", ln.strip()))
            elif ln.startswith("#"):
                out.append(ln.strip())
    return out


def test_cli_real_inputs_directory_of_pngs_and_a_saved_checkpoint(tmp_path):
    """The path no --synthetic run touches (inference/test_deblur.py:85,98-137): torch.load(path)['params'] with a strict load_state_dict,
    directory walking ./dataset/GOPRO/test/{blur,gt}/<video>/*.png, PNG decoding -- on a checkpoint file and PNG frames written here from
    the synthetic generators.  Run as the drop-in script itself (inference/test_deblur_small.py) from a scratch working directory, and
    compared line for line with the in-memory --synthetic run of the same clip and weights."""
    import subprocess
    import sys
    from PIL import Image
    from shiftnet_amd import cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    H, W, N = 64, 96, 16
    blur, sharp = synth.blurred_clip(N, H, W, seed=0)
    for sub, clip in (("blur", blur), ("gt", sharp)):
        d = tmp_path / "dataset" / "GOPRO" / "test" / sub / "synthetic"
        d.mkdir(parents=True)
        for i in range(N):
            Image.fromarray(clip[i]).save(d / ("%05d.png" % i))
    ck = tmp_path / "net.pth"
    torch.save({"params": synth_state_dict("gshift_deblur2")}, ck)
    script = os.path.join(root, "inference", "test_deblur_small.py")
    r = subprocess.run([sys.executable, script, "--default_data", "GOPRO", "--checkpoint", str(ck), "--one_len", "4", "--dtype", "bf16",
                        "--result_path", str(tmp_path / "real"), "--save_image"], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cli.main("gshift_deblur2", ["--synthetic", str(H), str(W), str(N), "--one_len", "4", "--dtype", "bf16", "--result_path", str(tmp_path / "syn")])
    real, syn = _cli_lines(str(tmp_path / "real")), _cli_lines(str(tmp_path / "syn"))
    assert len(real) == 3 + 2 and real == syn, (real, syn)          # 3 windows of 4, the video line, the total line
    assert len(list((tmp_path / "real" / "synthetic").glob("*.png"))) == 12


def test_cli_clip_parallel_two_ranks_log_the_single_process_lines(tmp_path):
    """--gpus 2 on the drop-in deblur CLI (windows of a clip two at a time, one per rank, halo frames by all-gather): two
    ranks share this box's one device (gloo transport with host staging, RCCL refuses two ranks per device), 5 windows = two full rounds
    and a partial one, PNGs written by both ranks.  Log lines and images must equal the single-process run's."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "inference", "test_deblur_small.py")
    common = ["--synthetic", "64", "96", "24", "--one_len", "4", "--dtype", "bf16", "--save_image"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    for tag, extra in (("one", []), ("two", ["--gpus", "2"])):
        r = subprocess.run([sys.executable, script] + common + extra + ["--result_path", str(tmp_path / tag)], cwd=tmp_path, env=env,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    one, two = _cli_lines(str(tmp_path / "one")), _cli_lines(str(tmp_path / "two"))
    assert len(one) == 5 + 2 and one == two, (one, two)
    a = sorted((tmp_path / "one" / "synthetic").glob("*.png"))
    b = sorted((tmp_path / "two" / "synthetic").glob("*.png"))
    assert len(a) == 20 and [p.name for p in a] == [p.name for p in b]
    for pa, pb in zip(a, b):
        assert pa.read_bytes() == pb.read_bytes(), pa.name


@pytest.mark.parametrize("name", ["gshift_denoise1", "gshift_denoise2"])
@pytest.mark.parametrize("T,h,w", [(2, 13, 70), (3, 40, 200), (2, 97, 130)])
def test_cab_phase1_fused_kernel_denoisers_two_passes(T, h, w, name, engines):
    """The denoisers' phase 1 on the role-split kernel (csrc/sn_phase1r.hip, sn_phase1_opts): pass 1 leaves the channel sums of g1 and -- through
    the squeeze-excite tail -- the scale of the inner CALayer2 (gshift_denoise1.py:224,257; gshift_denoise2.py:194,227), pass 2 the block's g2 with
    g1 scaled before the RepConv.  Against the reference's g1 sums, scale and g2, CAB1 and a forward CAB2; several strips and row segments."""
    from shiftnet_amd import lib as L
    eng, sd = engines(name)
    V = O.VARIANTS[name]
    C = V.c1
    x = bf(torch.from_numpy(synth.unit_noise((T, C, h, w), seed=101 + h)))
    xd = to_dev(x)
    st = torch.cuda.current_stream().cuda_stream
    groups = C // 8 if V.grouped_rep else C
    blk = "stage1.decoder_level1."
    tickets = torch.zeros((T,), dtype=torch.int32, device=DEV)
    for mode, unit in ((0, "encoder_level1.1."), (1, "encoder_level1.0.")):
        pre = blk + unit
        with torch.no_grad():
            if mode:
                u = O.gsts_gather(x, False, V.wrap)
                hw = bf(O._conv(sd, pre + "conv1.", u[:, C:], groups=C // 2))
                v = O.layer_norm_2d(torch.cat((u[:, :C], hw), 1), sd[pre + "norm.weight"], sd[pre + "norm.bias"])
                hwd = to_dev(hw)
            else:
                v = O.layer_norm_2d(x, sd[pre + "norm.weight"], sd[pre + "norm.bias"])
                hwd = None
            a = O._conv(sd, f"{pre}body.0.", v)
            a = O._conv(sd, f"{pre}body.1.conv_2.", a, groups=a.shape[1]) + a
            a1, a2 = a.chunk(2, dim=1)
            g1 = a1 * a2
            ca_ref = torch.sigmoid(O._conv(sd, f"{pre}body.3.conv_du.2.", torch.relu(O._conv(sd, f"{pre}body.3.conv_du.0.", g1.mean((2, 3), keepdim=True))))).reshape(T, C)
            b1, b2 = O._conv(sd, f"{pre}body.5.", O._rep_conv(sd, f"{pre}body.4.", O.channel_attention(sd, f"{pre}body.3.", g1), groups=groups)).chunk(2, dim=1)
            ref = b1 * torch.sigmoid(b2)
        p1, q1 = eng.P.units[pre]["p1r"], eng.P.cas[pre + "ca1"]
        src = L.UnitSrc(xd.data_ptr(), T, h, w, C, mode, 0)
        nblk = eng.lib.sn_phase1_pool_blocks(T, h, w)
        pool = torch.full((T, nblk, C), float("nan"), dtype=torch.float32, device=DEV)
        ca1 = torch.full((T, C), float("nan"), dtype=torch.float32, device=DEV)
        se1 = L.SeFold(q1["wa"].data_ptr(), q1["wb"].data_ptr(), q1["c"], q1["cr"], tickets.data_ptr(), ca1.data_ptr())
        hp = hwd.data_ptr() if hwd is not None else None
        L.check(L.cab_phase1(eng.lib, src, hp, p1["desc"], None, pool.data_ptr(), st, se1, L.Phase1Opts(None, 1)), "phase 1, g1 sums")
        torch.cuda.synchronize()
        sums, rs = pool.sum(1).cpu(), g1.sum((2, 3))
        assert torch.isfinite(sums).all() and (sums - rs).abs().max().item() <= 1e-2 * max(1.0, rs.abs().max().item()), (name, mode, (sums - rs).abs().max().item())
        assert (ca1.cpu() - ca_ref).abs().max().item() <= 2e-3, (name, mode, (ca1.cpu() - ca_ref).abs().max().item())
        assert int(tickets.abs().sum()) == 0
        g2 = torch.full((T, h, w, C), float("nan"), dtype=torch.bfloat16, device=DEV)
        L.check(L.cab_phase1(eng.lib, src, hp, p1["desc"], g2.data_ptr(), pool.data_ptr(), st, None, L.Phase1Opts(ca1.data_ptr(), 0)), "phase 1, pass 2")
        check(f"phase1_denoise_g2_{name}_{mode}_{T}x{h}x{w}", to_cpu(g2, C), ref, 1.2e-2)
        s2 = pool.sum(1).cpu()
        r2 = ref.sum((2, 3))
        assert (s2 - r2).abs().max().item() <= 1e-2 * max(1.0, r2.abs().max().item())
        # the same two passes with a g1 store (sn_phase1_opts.g1_store): pass 1 writes its g1 rows, pass 2 reads them back instead of recomputing
        # them -- same sums, same scale, bit-identical g2 and pool rows
        nbv = ctypes.c_longlong(0)
        L.check(eng.lib.sn_phase1_g1_store_bytes(T, h, w, C, ctypes.byref(nbv)), "sn_phase1_g1_store_bytes")
        nb = nbv.value
        assert nb > 0
        store = torch.full((nb // 2,), float("nan"), dtype=torch.float16, device=DEV)       # NaN: a row pass 2 reads but pass 1 did not write would show
        pool_b = torch.full((T, nblk, C), float("nan"), dtype=torch.float32, device=DEV)
        ca1_b = torch.full((T, C), float("nan"), dtype=torch.float32, device=DEV)
        se1_b = L.SeFold(q1["wa"].data_ptr(), q1["wb"].data_ptr(), q1["c"], q1["cr"], tickets.data_ptr(), ca1_b.data_ptr())
        L.check(L.cab_phase1(eng.lib, src, hp, p1["desc"], None, pool_b.data_ptr(), st, se1_b, L.Phase1Opts(None, 1, 0, store.data_ptr())), "phase 1, g1 sums + store")
        torch.cuda.synchronize()
        assert torch.equal(ca1_b, ca1), (name, mode)
        g2_b = torch.full((T, h, w, C), float("nan"), dtype=torch.bfloat16, device=DEV)
        L.check(L.cab_phase1(eng.lib, src, hp, p1["desc"], g2_b.data_ptr(), pool_b.data_ptr(), st, None, L.Phase1Opts(ca1_b.data_ptr(), 0, 0, store.data_ptr())),
                "phase 1, pass 2 from the g1 store")
        torch.cuda.synchronize()
        assert torch.equal(g2_b.view(torch.int16), g2.view(torch.int16)), (name, mode, (g2_b.float() - g2.float()).abs().max().item())
        assert torch.equal(pool_b, pool), (name, mode)


# ---------------------------------------------------------------------------------------------------------------
# PReLU slopes outside [0, 1].  Every slope of the synthetic checkpoint is 0.25 +- 0.05, but the kernels branch on the VALUE: conv3_fast_kernel
# (csrc/sn_conv.hip) and cab_fused_kernel (csrc/sn_cabf.hip) compute max(v, a v) for a slope in [0, 1] and fma(a, min(v, 0), max(v, 0)) for any
# other; the streaming conv (csrc/sn_conv3p.hip) implements its PReLU + pool epilogue and the streaming fused CAB for [0, 1] only, and the
# library / the engine must route other slopes elsewhere.  nn.PReLU does not constrain its weight: a trained checkpoint may hold any of these.
PRELU_SLOPES = (-0.25, 0.0, 1.0, 1.25)          # both ends of the fast path's [0, 1] and one value outside on each side


@pytest.mark.parametrize("case", list(CONV_CASES))
@pytest.mark.parametrize("slope", PRELU_SLOPES)
@pytest.mark.parametrize("tiles", [True, False])
def test_conv_prelu_slopes(case, slope, tiles, engines):
    """test_conv at the edges of [0, 1] and outside it, on the tile kernels (conv_tiles) and with the streaming kernel allowed: every conv
    kernel's PReLU epilogue against F.prelu, ragged tiles, pad channels that must stay zero."""
    name, key, wkey, cins, stride, pad = CONV_CASES[case]
    eng, sd = engines(name)
    e = _sibling_engine(eng, conv_tiles=tiles)
    T, H, W = 2, 10, 36
    xs = [bf(torch.from_numpy(synth.unit_noise((T, c, H, W), seed=151 + i))) for i, c in enumerate(cins)]
    out = e.conv(key, [act(to_dev(x), c) for x, c in zip(xs, cins)], stride=stride, pad=pad, prelu=slope)
    torch.cuda.synchronize()
    ref = torch.nn.functional.conv2d(torch.cat(xs, 1), sd[wkey + "weight"], sd.get(wkey + "bias"), stride=stride, padding=pad)
    ref = torch.nn.functional.prelu(ref, torch.tensor([slope]))
    check(f"conv_prelu{slope}_{case}_{'tile' if tiles else 'stream'}_{H}x{W}", to_cpu(out.t, out.c), ref, 8e-3)
    if out.t.shape[-1] > out.c:
        assert out.t[..., out.c:].float().abs().max().item() == 0.0


@pytest.mark.parametrize("name,pre,c", [("gshift_deblur2", "stage1.concat.", 14), ("gshift_deblur2", "orb1.encoder_level2.1.", 18),
                                        ("gshift_deblur1", "orb1.encoder_level2.0.", 36), ("gshift_deblur2", "stage1.skip_attn1.", 64)])
@pytest.mark.parametrize("slope", (0.2,) + PRELU_SLOPES)
@pytest.mark.parametrize("T,hw", [(2, (37, 33)), (5, (72, 200))])
def test_cab_first_conv_prelu_slopes_with_pool(name, pre, c, slope, T, hw, engines):
    """The first conv of a CAB (3x3 + PReLU + channel sums of the activated map) on the streaming kernel -- for a slope outside [0, 1] the library
    sends it to the tile kernel (c3p_mode) -- and on the tile kernel: the activations bit-identical to each other, and both the activations and
    the pooled means within the kernel tolerance of the oracle (the pool rows must sum the ACTIVATED values)."""
    eng, sd = engines(name)
    new = _sibling_engine(eng, conv_tiles=False, conv_stream_all=True)
    old = _sibling_engine(eng, conv_tiles=True)
    x = act(to_dev(bf(torch.from_numpy(synth.unit_noise((T, c, hw[0], hw[1]), seed=152)))), c)
    m_new, p_new, npix = new.conv(pre + "body.0", [x], prelu=slope, pool=True)
    m_old, p_old, _ = old.conv(pre + "body.0", [x], prelu=slope, pool=True)
    torch.cuda.synchronize()
    assert torch.equal(m_new.t, m_old.t), (name, pre, slope, T, hw, (m_new.t.float() - m_old.t.float()).abs().max().item())
    F = torch.nn.functional
    ref = F.prelu(F.conv2d(to_cpu(x.t, c), bf(sd[pre + "body.0.weight"]), sd.get(pre + "body.0.bias"), padding=1), torch.tensor([slope]))
    for tag, m, p in (("stream", m_new, p_new), ("tile", m_old, p_old)):
        check(f"conv_pool_prelu{slope}_{tag}_{name}_{pre}_{T}x{hw[0]}x{hw[1]}", to_cpu(m.t, c), ref, 8e-3)
        check(f"conv_pool_prelu{slope}_{tag}_{name}_{pre}_{T}x{hw[0]}x{hw[1]}_sums", p.sum(1)[:, :c] / npix, ref.mean((2, 3)), 8e-3)


# gshift_deblur2 CABs with 16-channel storage (14 channels: fused instance key 1016) and 24-channel storage (18 channels: key 2024)
CAB_EDGE = [("stage1.concat.", 14), ("orb1.encoder_level2.1.", 18)]
CAB_FORMS = {"0_tile": dict(cab_fused="0", conv_tiles=True), "0_stream": dict(cab_fused="0", conv_tiles=False),
             "8": dict(cab_fused="8", conv_tiles=False), "16": dict(cab_fused="16", conv_tiles=False),
             "s8": dict(cab_fused="s8", conv_tiles=False), "p": dict(cab_fused="p", conv_tiles=False)}


@pytest.fixture(scope="module")
def edge_engines():
    """(Engine, state dict) of gshift_deblur2's edge checkpoint (tests/prelu_edge.py) with the PReLU of both CAB_EDGE CABs set to `slope`."""
    from shiftnet_amd.engine import Engine, Plan
    cache = {}

    def get(slope):
        if slope not in cache:
            sd = edge_state_dict("gshift_deblur2")
            for pre, _ in CAB_EDGE:
                set_slope(sd, "gshift_deblur2", pre + "body.1.weight", slope)
            cache[slope] = (Engine(Plan(VARIANTS["gshift_deblur2"], sd, DEV)), sd)
        return cache[slope]
    return get


def _traced(eng, **attrs):
    """_sibling_engine that records the C-ABI functions it launches."""
    e = _sibling_engine(eng, **attrs)
    e.called = []
    orig = e._call
    e._call = lambda fn, *a: (e.called.append(fn), orig(fn, *a))[1]
    return e


@pytest.mark.parametrize("pre,c", CAB_EDGE)
@pytest.mark.parametrize("slope", PRELU_SLOPES)
@pytest.mark.parametrize("T,hw", [(3, (45, 150)), (3, (2, 3)), (1, (360, 640))])
def test_cab_prelu_slopes_every_form(pre, c, slope, T, hw, edge_engines):
    """A CAB on the edge checkpoint through every form -- two launches on the tile / streaming convs, the tile fused form with 8 and 16 rows, its
    streaming-statistics variant, the streaming fused form -- with and without the second residual, ragged tiles, a map smaller than a tile and a
    360 x 640 frame: each within the CAB tolerance of O.cab.  The tile fused forms stay bit-identical to the two-launch tile form.  "p" runs the
    streaming fused form for a slope in [0, 1] and, decided before anything is launched, the two-launch form for any other slope; either way
    its result is bit-identical to the two-launch form with the same switches."""
    eng, sd = edge_engines(slope)
    assert eng.P.scalar(pre + "body.1.weight") == torch.tensor(slope).item()
    x = bf(torch.from_numpy(synth.unit_noise((T, c, hw[0], hw[1]), seed=153)))
    e = bf(torch.from_numpy(synth.unit_noise((T, c, hw[0], hw[1]), seed=154)))
    xa, ea = act(to_dev(x), c), act(to_dev(e), c)
    ref = O.cab(sd, pre, x)
    outs, called = {}, {}
    for form, attrs in CAB_FORMS.items():
        f = _traced(eng, **attrs)
        outs[form] = (f.cab(pre, xa).t, f.cab(pre, xa, ea).t)
        called[form] = f.called
    torch.cuda.synchronize()
    tag = f"{slope}_{pre}_{T}x{hw[0]}x{hw[1]}"
    for form, (o0, o1) in outs.items():
        check(f"cab_prelu{tag}_{form}", to_cpu(o0, c), ref, 8e-3)
        check(f"cab_prelu{tag}_{form}_extra", to_cpu(o1, c), ref + e, 8e-3)
        if o0.shape[-1] > c:
            assert o0[..., c:].float().abs().max().item() == 0.0 and o1[..., c:].float().abs().max().item() == 0.0, form
    for form in ("8", "16", "s8"):
        assert called[form].count("sn_cab_fused") == 2 and "sn_conv2d" not in called[form], (form, called[form])
    for form in ("8", "16"):
        assert torch.equal(outs[form][0], outs["0_tile"][0]) and torch.equal(outs[form][1], outs["0_tile"][1]), (form, tag)
    inside = 0.0 <= slope <= 1.0
    assert called["p"].count("sn_cab_fused") == int(inside) and called["p"].count("sn_cab_stats") == int(inside), called["p"]
    assert torch.equal(outs["p"][0], outs["0_stream"][0]) and torch.equal(outs["p"][1], outs["0_stream"][1]), tag


@pytest.mark.parametrize("slope", [-0.25, 0.6])
def test_default_cab_path_at_720p_prelu_slopes(slope, edge_engines):
    """The product default (SN_CAB_FUSED=p16, streaming convs) on Shift-Net-s' 14-channel full-resolution CAB at T = 5, 720 x 1280: 4.6 M
    pixel-frames, above CAB_FUSED_MIN_PX, where the engine picks the streaming fused form.  With a negative slope the engine used to launch the
    statistics pass and the CALayer and then fail in sn_cab_fused(rows = 0) (ShiftNetLibError: the forward aborted); it must take the two-launch
    form instead.  0.6 (in [0, 1]) shows that this geometry does reach the streaming fused form."""
    eng, sd = edge_engines(slope)
    pre, c = "stage1.concat.", 14
    f = _traced(eng, cab_fused="p16", conv_tiles=False)
    T, H, W = 5, 720, 1280
    assert T * H * W >= f.CAB_FUSED_MIN_PX
    x = bf(torch.from_numpy(synth.unit_noise((T, c, H, W), seed=155)))
    out = f.cab(pre, act(to_dev(x), c)).t
    torch.cuda.synchronize()
    assert f.called.count("sn_cab_fused") == int(0.0 <= slope <= 1.0), f.called
    check(f"cab_default_p16_prelu{slope}_{T}x{H}x{W}", to_cpu(out, c), O.cab(sd, pre, x), 8e-3)


@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_denoise1"])
def test_whole_net_prelu_edge_checkpoint(name):
    """The drop-in class on the edge checkpoint (every PReLU of the network at -0.25 / 0 / 0.6 / 1 / 1.25), SN_CAB_FUSED=p so that this small clip
    reaches the streaming fused CAB wherever the slope allows it, against a live fp32 O.forward with the bounds of test_whole_net_vs_golden.  The
    denoiser adds the PReLU'd DownSample convs (stride 2) and the PReLU after rconcat.  The range guard must not have tripped: the result comes
    from the fused phase 1, not the chain."""
    import importlib
    mod = importlib.import_module(f"basicsr.models.archs.{name}")
    V = O.VARIANTS[name]
    sd = edge_state_dict(name)
    blur, sharp = synth.blurred_clip(7, 48, 64, seed=3)
    x = O.frames_to_tensor(list(blur))
    nm = torch.full((1, 7, 1, 48, 64), 30.0 / 255.0) if V.denoise else None
    net = mod.GShiftNet(future_frames=2, past_frames=2)
    net.load_state_dict(sd, strict=True)
    net = net.to(torch.bfloat16).to("cuda").eval()
    eng = net.prepare()
    eng.cab_fused = "p"
    called = []
    orig = eng._call
    eng._call = lambda fn, *a: (called.append(fn), orig(fn, *a))[1]
    args = (x.bfloat16().cuda(), nm.bfloat16().cuda()) if V.denoise else (x.bfloat16().cuda(),)
    with torch.no_grad():
        out = net(*args).float().cpu()
        out32 = net.forward_fp32_out(*args, shortcut=x.cuda()).cpu()
        ref = O.forward(V, sd, x, nm, 2, 2)
    assert eng.fallbacks == 0 and eng.phase1 != "0"
    assert "sn_cab_fused" in called and "sn_cab_stats" in called                 # the streaming fused CAB ran where the slope is in [0, 1]
    assert torch.isfinite(ref).all() and out.shape == ref.shape
    gt = torch.from_numpy(sharp[2:5]).permute(0, 3, 1, 2).float() / 255
    p_oo, p_32 = _psnr(out, ref), _psnr(out32, ref)
    dpsnr = abs(_psnr(out32.clamp(0, 1), gt) - _psnr(ref.clamp(0, 1), gt))
    xin = x[0, 2:5]
    corr_err = ((out32 - xin) - (ref - xin)).pow(2).mean().sqrt().item() / (ref - xin).pow(2).mean().sqrt().item()
    REPORT.append({"name": f"net_prelu_edge_{name}", "psnr_vs_ref": p_oo, "psnr_fp32_out_vs_ref": p_32, "delta_psnr_gt": dpsnr,
                   "correction_rel_rms_err": corr_err, "max_abs": (out32 - ref).abs().max().item()})
    assert p_oo >= 48.0 and p_32 >= 48.0 and dpsnr <= 0.01, (name, p_oo, p_32, dpsnr)
    assert corr_err <= CORR_TOL, (name, corr_err)
