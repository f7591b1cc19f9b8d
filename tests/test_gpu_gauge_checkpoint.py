"""-m gpu: whole checkpoints moved along the gate's rescaling orbit (tests/gauge.py) through the engines.  The network function is the same bit for
bit in fp32 (tests/test_host_gauge.py), so every reference here is an EXISTING one: the golden outputs of tests/golden/net_<name>.npz and the oracle
blocks on the BASE weights.

  * bf16 / fp16 module, all four variants: per block and channel random exponents in [-3, 3], loaded strict=True, on the clip and with the asserts
    of test_gpu_parity.py::test_whole_net_vs_golden; the range guard does not move the engine (fallbacks == 0);
  * one GSTS unit's CAB2 and CAB1 per variant through Engine.naf at the uniform rungs k = -4 (a third of the fused kernel's g1 is an fp16 subnormal)
    and k = +6, on the fused kernel and on the two-kernel chain, at the tolerance test_gsts_pieces / test_gsts_pieces_bf16_chain use for the block;
  * fp32 engine, exact and split products: a unit on a checkpoint regauged with random exponents in +-6 is bit-identical to the base-gauge run
    (bf16 hi / lo splitting and fp32 sums commute with powers of two).
"""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import gauge as G
from oracle import shiftnet_oracle as O
from shiftnet_amd import synth
from shiftnet_amd.spec import VARIANTS
from shiftnet_amd.weights import synth_state_dict
from test_gpu_parity import CORR_TOL, _psnr, _sibling_engine, act, bf, check, to_cpu, to_dev

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ["gshift_deblur2", "gshift_denoise2", "gshift_deblur1", "gshift_denoise1"]
BLK = "stage1.decoder_level1."
REPORT = []
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    d = os.environ.get("SN_PARITY_REPORT_DIR") or os.path.join(ROOT, "parity_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "parity_report_gauge_checkpoint.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_regauged_whole_net_vs_golden(name, dt, golden_dir):
    """test_whole_net_vs_golden's clip, golden and bounds on a checkpoint that sits elsewhere on the orbit"""
    mod = importlib.import_module(f"basicsr.models.archs.{name}")
    V = O.VARIANTS[name]
    g = np.load(os.path.join(golden_dir, f"net_{name}.npz"))
    blur, sharp = synth.blurred_clip(7, 48, 64, seed=3)
    assert synth.crc(blur) == int(g["in_crc"])
    x = O.frames_to_tensor(list(blur))
    net = mod.GShiftNet(future_frames=2, past_frames=2)
    net.load_state_dict(G.regauge_state_dict(name, synth_state_dict(name), *G.seeded_exponents(3, 23)), strict=True)
    net = net.to(dt).to("cuda").eval()
    nm = torch.full((1, 7, 1, 48, 64), 30.0 / 255.0) if V.denoise else None
    args = (x.to(dt).cuda(), nm.to(dt).cuda()) if V.denoise else (x.to(dt).cuda(),)
    with torch.no_grad():
        out = net(*args)
        out32 = net.forward_fp32_out(*args, shortcut=x.cuda())
    ref = torch.from_numpy(g["p2f2"])
    assert tuple(out.shape) == tuple(ref.shape) and out.dtype == dt
    assert out32.dtype == torch.float32 and tuple(out32.shape) == tuple(ref.shape)
    out, out32 = out.float().cpu(), out32.cpu()
    gt = torch.from_numpy(sharp[2:5]).permute(0, 3, 1, 2).float() / 255
    p_oo, p_32 = _psnr(out, ref), _psnr(out32, ref)
    dpsnr = abs(_psnr(out32.clamp(0, 1), gt) - _psnr(ref.clamp(0, 1), gt))
    xin = x[0, 2:5]
    corr_err = ((out32 - xin) - (ref - xin)).pow(2).mean().sqrt().item() / (ref - xin).pow(2).mean().sqrt().item()
    eng = net._plan
    REPORT.append({"name": f"net_regauged_{name}_{dt}", "psnr_vs_ref": p_oo, "psnr_fp32_out_vs_ref": p_32, "delta_psnr_gt": dpsnr,
                   "correction_rel_rms_err": corr_err, "max_abs": (out32 - ref).abs().max().item(), "fallbacks": eng.fallbacks})
    assert p_oo >= 48.0 and p_32 >= 48.0 and dpsnr <= 0.01, (name, dt, p_oo, p_32, dpsnr)
    assert corr_err <= CORR_TOL, (name, dt, corr_err)
    assert eng.fallbacks == 0 and eng.phase1 != "0", (name, dt, eng.fallbacks, eng.phase1)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("k", [-4, 6])
def test_gsts_unit_at_a_uniform_rung(name, k):
    """CAB2 (both directions) and CAB1 of one unit through Engine.naf on weights regauged to the uniform rung k, fused and chain, against the oracle
    block on the BASE weights at the 8e-3 of test_gsts_pieces"""
    from shiftnet_amd.engine import Engine, Plan
    V = O.VARIANTS[name]
    sd = synth_state_dict(name)
    keep = {kk: v for kk, v in sd.items() if kk.startswith(BLK)}
    fused = Engine(Plan(VARIANTS[name], G.regauge_state_dict(name, sd, k, k), DEV))
    chain = _sibling_engine(fused, phase1="0")
    assert fused._fused_phase1(4) and not chain._fused_phase1(4)
    C, T, h, w = V.c1, 4, 20, 44
    x = bf(torch.from_numpy(synth.unit_noise((T, C, h, w), seed=81)))
    xd = act(to_dev(x), C)
    with torch.no_grad():
        refs = [(BLK + unit + "0.", mode, O.cab2(keep, BLK + unit + "0.", O.gsts_gather(x, rev, V.wrap), V))
                for mode, rev, unit in ((1, False, "encoder_level1."), (2, True, "encoder_level1_1."))]
        refs.append((BLK + "encoder_level1.1.", 0, O.cab1(keep, BLK + "encoder_level1.1.", x, V)))
    for tag, eng in (("fused", fused), ("chain", chain)):
        for pre, mode, ref in refs:
            out = eng.naf(pre, xd, mode)
            torch.cuda.synchronize()
            got = to_cpu(out.t, C)
            REPORT.append({"name": f"gauge_k{k:+d}_{tag}_{name}_mode{mode}", "max_abs": (got - ref).abs().max().item(), "scale": max(1.0, ref.abs().max().item())})
            check(f"gauge_k{k:+d}_{tag}_{name}_mode{mode}", got, ref, 8e-3)
        assert not eng._guard_tripped(), (name, k, tag)
    assert fused.fallbacks == 0


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("split", [False, True], ids=["exact", "split"])
def test_fp32_engine_is_gauge_invariant_bit_for_bit(name, split, monkeypatch):
    from shiftnet_amd.engine import Act, make_engine
    from shiftnet_amd.engine32 import Engine32
    monkeypatch.setattr(Engine32, "split_bf16", split)
    V = O.VARIANTS[name]
    sd = synth_state_dict(name)
    C, T, h, w = V.c1, 3, 13, 44
    x = torch.from_numpy(synth.unit_noise((T, C, h, w), seed=85)).permute(0, 2, 3, 1).contiguous().to(DEV)
    outs = []
    for d in (sd, G.regauge_state_dict(name, sd, *G.seeded_exponents(6, 29))):
        eng = make_engine(VARIANTS[name], d, DEV, torch.float32)
        with torch.no_grad():
            outs.append([eng.gsts_unit(BLK + unit, Act(x, C), rev).t.clone() for unit, rev in (("encoder_level1.", False), ("encoder_level1_1.", True))])
        torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert bool(torch.isfinite(a).all())
        assert torch.equal(a, b), (name, split, (a - b).abs().max().item())
