"""The launch sequence of a GSTS unit (Engine.gsts_unit / Engine.naf, engine.py), route by route: which C-ABI entry points are called in which order,
which profiler records they leave, which tensors Engine.naf_buffers allocates for the route -- and that frame ranges, caller-owned buffers and the
composition of a unit from two CABs leave every bit of the result alone (torch.equal on raw bits).  One strip with ragged blocks, three frames: a
boundary frame on each side and an interior one; nothing about the sequence depends on the size."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "shift-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from shiftnet_amd import synth
from shiftnet_amd.spec import VARIANTS
from shiftnet_amd.weights import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BLK = "stage1.decoder_level1."
FWD, REV = BLK + "encoder_level1.", BLK + "encoder_level1_1."          # a forward and a reverse unit
T, H, W = 3, 8, 12
DEFAULTS = dict(phase1="auto", k4_fuse="1", g1_store=True, fold_se=True, k0_mfma=True, schedule="unit")      # whatever the SN_* environment says

# K0: sn_gsts_shiftconv_mfma where Plan.k0_mfma_ok, else sn_gsts_shiftconv.  K3: sn_dw5m_gemm_gate, sn_grp5_gemm_gate for the grouped "+" models.
LAUNCHES = {
    "four": ["K0", "sn_gsts_cab2_phase1", "sn_cab2_phase2_cab1_phase1", "sn_cab1_phase2"],
    "five": ["K0", "sn_gsts_cab2_phase1", "sn_gsts_cab2_phase2", "sn_cab1_phase1", "sn_cab1_phase2"],
    "two passes": ["K0", "sn_gsts_cab2_phase1", "sn_gsts_cab2_phase1", "sn_gsts_cab2_phase2", "sn_cab1_phase1", "sn_cab1_phase1", "sn_cab1_phase2"],
    "chain": ["K0", "sn_ln_gemm_gate", "K3", "sn_ca_mlp", "sn_gsts_cab2_phase2", "sn_ln_gemm_gate", "K3", "sn_ca_mlp", "sn_cab1_phase2"],
    "chain, denoise": ["K0", "sn_ln_gemm_gate", "sn_ca_mlp", "K3", "sn_ca_mlp", "sn_gsts_cab2_phase2",
                       "sn_ln_gemm_gate", "sn_ca_mlp", "K3", "sn_ca_mlp", "sn_cab1_phase2"],
    "no fold": ["K0", "sn_gsts_cab2_phase1", "sn_ca_mlp", "sn_gsts_cab2_phase2", "sn_cab1_phase1", "sn_ca_mlp", "sn_cab1_phase2"],
}
# (variant, switches, launches of a unit, what naf_buffers holds besides g2, y, pool2, ca2 and -- mode 1 / 2 -- hwb)
ROUTES = [
    ("gshift_deblur2", {}, "four", set()),
    ("gshift_deblur2", {"k4_fuse": "0"}, "five", set()),
    ("gshift_deblur1", {}, "five", set()),
    ("gshift_deblur1", {"k4_fuse": "0"}, "five", set()),
    ("gshift_denoise1", {}, "two passes", {"ca1", "g1s"}),
    ("gshift_denoise2", {}, "two passes", {"ca1", "g1s"}),
    ("gshift_denoise1", {"g1_store": False}, "two passes", {"ca1"}),
    ("gshift_denoise2", {"g1_store": False}, "two passes", {"ca1"}),
    ("gshift_deblur1", {"phase1": "0"}, "chain", {"g1"}),
    ("gshift_deblur2", {"phase1": "0"}, "chain", {"g1"}),
    ("gshift_denoise1", {"phase1": "0"}, "chain, denoise", {"ca1", "g1", "pool1"}),
    ("gshift_denoise2", {"phase1": "0"}, "chain, denoise", {"ca1", "g1", "pool1"}),
    ("gshift_deblur2", {"fold_se": False}, "no fold", set()),
]
ROUTE_IDS = [f"{n}-{','.join(f'{k}={v}' for k, v in sw.items()) or 'defaults'}" for n, sw, _, _ in ROUTES]


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


_plans = {}


def sibling(name, **attrs):
    """An Engine on the variant's prepared weights (built once per module) that records the C-ABI functions it launches."""
    from shiftnet_amd.engine import Engine, Plan
    if name not in _plans:
        _plans[name] = Plan(VARIANTS[name], synth_state_dict(name), DEV)
    e = Engine(_plans[name])
    for k, v in {**DEFAULTS, **attrs}.items():
        setattr(e, k, v)
    e.called = []
    orig = e._call
    e._call = lambda fn, *a: (e.called.append(fn), orig(fn, *a))[1]
    return e


def clip(name, seed=0):
    from shiftnet_amd.engine import Act
    c = VARIANTS[name].c1
    return Act(torch.from_numpy(synth.unit_noise((T, H, W, c), seed=340 + seed)).to(torch.bfloat16).to(DEV), c)


def spelled(eng, launches):
    k0 = "sn_gsts_shiftconv_mfma" if eng.P.k0_mfma_ok else "sn_gsts_shiftconv"
    k3 = "sn_grp5_gemm_gate" if eng.V.grouped_rep else "sn_dw5m_gemm_gate"
    return [{"K0": k0, "K3": k3}.get(fn, fn) for fn in LAUNCHES[launches]]


@pytest.mark.parametrize("name,switches,launches,extra", ROUTES, ids=ROUTE_IDS)
def test_launch_order_of_a_unit(name, switches, launches, extra):
    eng, x = sibling(name, **switches), clip(name)
    for pre, rev in ((FWD, False), (REV, True)):
        eng.called.clear()
        y = eng.gsts_unit(pre, x, rev)
        torch.cuda.synchronize()
        print(name, switches, pre, eng.called)
        assert eng.called == spelled(eng, launches), (pre, eng.called)
        assert y.dims == x.dims and torch.isfinite(y.t.float()).all()


@pytest.mark.parametrize("name,switches,launches,extra", ROUTES, ids=ROUTE_IDS)
def test_buffers_follow_the_route(name, switches, launches, extra):
    eng, c = sibling(name, **switches), VARIANTS[name].c1
    for mode in (0, 1, 2):
        keys = set(eng.naf_buffers(T, H, W, c, mode))
        assert keys == {"g2", "y", "pool2", "ca2"} | ({"hwb"} if mode else set()) | extra, (mode, keys)


def test_profiler_records_of_the_four_launch_unit():
    eng, x = sibling("gshift_deblur2"), clip("gshift_deblur2")
    assert eng.P.k0_mfma_ok
    eng.prof = []
    eng.gsts_unit(FWD, x, False)
    torch.cuda.synchronize()
    cab2, cab1 = ("naf", 3, 8, 12, 64, 1, 3), ("naf", 3, 8, 12, 64, 0, 3)
    assert [r[:3] for r in eng.prof] == [
        ("sn_gsts_shiftconv_mfma", "sn_gsts_shiftconv", cab2),
        ("sn_gsts_cab2_phase1", "sn_gsts_cab2_phase1", cab2),
        ("sn_gsts_cab2_phase2", "sn_gsts_cab2_phase2 [in sn_cab1_phase1]", cab2),
        ("sn_cab1_phase1", "sn_cab2_phase2_cab1_phase1", cab1),
        ("sn_cab1_phase2", "sn_cab1_phase2", cab1)], eng.prof
    assert len(eng.called) == 4 and all(len(r) == 5 for r in eng.prof)
    extra, fused = eng.prof[2], eng.prof[3]
    assert extra[3] is extra[4] and extra[3] is fused[3]           # zero length: the fused launch's start event, twice
    assert extra[2] == ("naf", T, H, W, 64, 1, T) and fused[0] == "sn_cab1_phase1"
    assert all(r[3] is not r[4] for i, r in enumerate(eng.prof) if i != 2)


def test_profiler_records_of_the_five_launch_unit():
    eng, x = sibling("gshift_deblur2", k4_fuse="0"), clip("gshift_deblur2")
    eng.prof = []
    eng.gsts_unit(FWD, x, False)
    torch.cuda.synchronize()
    cab2, cab1 = ("naf", 3, 8, 12, 64, 1, 3), ("naf", 3, 8, 12, 64, 0, 3)
    assert [r[:3] for r in eng.prof] == [
        ("sn_gsts_shiftconv_mfma", "sn_gsts_shiftconv", cab2),
        ("sn_gsts_cab2_phase1", "sn_gsts_cab2_phase1", cab2),
        ("sn_gsts_cab2_phase2", "sn_gsts_cab2_phase2", cab2),
        ("sn_cab1_phase1", "sn_cab1_phase1", cab1),
        ("sn_cab1_phase2", "sn_cab1_phase2", cab1)], eng.prof
    assert all(r[3] is not r[4] for r in eng.prof)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_frame_range_and_caller_buffers_change_no_bit(name):
    """naf(pre, x, mode) against the same call as ONE frame range over all frames on buffers the caller owns."""
    eng, x, c = sibling(name), clip(name, 1), VARIANTS[name].c1
    for pre, mode in ((FWD + "0.", 1), (REV + "0.", 2), (FWD + "1.", 0)):
        a = eng.naf(pre, x, mode)
        bufs = eng.naf_buffers(T, H, W, c, mode)
        b = eng.naf(pre, x, mode, frames=(0, T), bufs=bufs)
        torch.cuda.synchronize()
        assert b.t.data_ptr() == bufs["y"].data_ptr()
        assert torch.isfinite(a.t.float()).all() and same(a.t, b.t), (name, mode)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_unit_equals_its_two_cabs_composed_by_hand(name):
    eng, off, x = sibling(name), sibling(name, k4_fuse="0"), clip(name, 2)
    for pre, rev in ((FWD, False), (REV, True)):
        a = eng.gsts_unit(pre, x, rev)
        b = off.naf(pre + "1.", off.naf(pre + "0.", x, 2 if rev else 1), 0)
        torch.cuda.synchronize()
        assert torch.isfinite(b.t.float()).all() and same(a.t, b.t), (name, pre)
    assert ("sn_cab2_phase2_cab1_phase1" in eng.called) == (name == "gshift_deblur2") and "sn_cab2_phase2_cab1_phase1" not in off.called
