"""CPU: the edge checkpoint of tests/prelu_edge.py (PReLU slopes outside [0, 1]) is a valid checkpoint of every variant, loads strictly into the
reference modules, keeps the shared PReLUs shared, and leaves the synthetic checkpoint itself unchanged."""
import importlib

import pytest
import torch

from oracle import shiftnet_oracle as O
from prelu_edge import EDGE_SLOPES, edge_state_dict, prelu_groups
from shiftnet_amd import synth
from shiftnet_amd.spec import VARIANTS
from shiftnet_amd.weights import alias_groups, synth_state_dict

PRELU_SUFFIXES = (".body.1.weight", ".down.1.weight", "down01.1.weight", "act.weight", "lrelu.weight")


@pytest.mark.parametrize("name", list(VARIANTS))
def test_edge_state_dict_covers_every_prelu_and_keeps_aliases(name):
    sd, base = edge_state_dict(name), synth_state_dict(name)
    assert list(sd) == list(base)
    scalars = {k for k, v in base.items() if v.numel() == 1}
    assert scalars and all(k.endswith(PRELU_SUFFIXES) for k in scalars), sorted(k for k in scalars if not k.endswith(PRELU_SUFFIXES))
    groups = prelu_groups(name)
    assert {k for g in groups.values() for k in g} == scalars                 # every PReLU key is covered, nothing else
    for canon, keys in alias_groups(name).items():                              # shared slopes stay one tensor
        assert all(sd[k] is sd[canon] for k in keys), canon
    slopes = {canon: sd[canon].item() for canon in groups}
    assert len(groups) >= len(EDGE_SLOPES) and set(slopes.values()) == {torch.tensor(v).item() for v in EDGE_SLOPES}     # (fp32 values)
    for k, v in sd.items():                                                     # nothing but the slopes moved
        if k not in scalars:
            assert v is base[k] or torch.equal(v, base[k]), k
    assert any(v < 0 for v in slopes.values()) and any(v > 1 for v in slopes.values())
    mod = importlib.import_module(f"basicsr.models.archs.{name}")
    net = mod.GShiftNet(future_frames=2, past_frames=2)
    net.load_state_dict(sd, strict=True)
    for canon, keys in groups.items():                                          # the module's shared nn.PReLU got the one value
        for k in keys:
            assert net.state_dict()[k].item() == slopes[canon], k
    assert all(0 < base[k].item() < 1 for k in scalars)                        # the synthetic recipe itself is untouched


def test_edge_state_dict_has_the_required_out_of_range_slopes():
    sd = edge_state_dict("gshift_deblur2")
    orb = {k: sd[k].item() for k in prelu_groups("gshift_deblur2") if k.split(".")[0].lstrip("r").startswith("orb")}
    assert len(orb) == 10 and min(orb.values()) < 0, orb                       # a negative orb slope of Shift-Net-s
    sd = edge_state_dict("gshift_denoise1")
    down = {k: sd[k].item() for k in prelu_groups("gshift_denoise1") if k.endswith("down.1.weight")}
    assert down and any(not 0 <= v <= 1 for v in down.values()), down           # a DownSample PReLU outside [0, 1]


@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_denoise1"])
def test_edge_state_dict_forward_is_finite(name):
    V = O.VARIANTS[name]
    blur, _ = synth.blurred_clip(5, 32, 32, seed=5)
    x = O.frames_to_tensor(list(blur))
    nm = torch.full((1, 5, 1, 32, 32), 30.0 / 255.0) if V.denoise else None
    with torch.no_grad():
        y = O.forward(V, edge_state_dict(name), x, nm, 2, 2)
    assert y.shape == (1, 3, 32, 32) and torch.isfinite(y).all()
