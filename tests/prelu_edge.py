"""The synthetic checkpoint with PReLU slopes outside [0, 1] (test-side; shiftnet_amd.weights.synth_state_dict is left as it is).

Every PReLU slope of ``synth_state_dict`` is 0.25 +- 0.05, so the kernels' general PReLU form -- the branch a slope below 0 or above 1
takes in csrc/sn_conv.hip (conv3_fast_kernel) and csrc/sn_cabf.hip (cab_fused_kernel), and the fall-backs of the streaming kernels of
csrc/sn_conv3p.hip, which implement only [0, 1] -- never ran on it.  ``nn.PReLU`` does not constrain its weight: a trained checkpoint may
hold any of these values.
"""
from collections import OrderedDict
from typing import Dict, List

import torch

from shiftnet_amd.spec import VARIANTS, param_table
from shiftnet_amd.weights import alias_groups, synth_state_dict

# both ends of the fast path's [0, 1], one value inside, one on each side outside
EDGE_SLOPES = (-0.25, 0.0, 0.6, 1.0, 1.25)


def prelu_groups(name: str) -> Dict[str, List[str]]:
    """canonical PReLU key -> every key that aliases it (itself first): the 1-element leaves of the state dict."""
    tab = param_table(VARIANTS[name])
    groups = alias_groups(name)
    out: Dict[str, List[str]] = {}
    for key, shape in tab.entries:
        if shape == (1,):
            canon = tab.alias.get(key, key)
            out.setdefault(canon, groups.get(canon, [canon]))
    return out


def set_slope(sd: "OrderedDict[str, torch.Tensor]", name: str, key: str, value: float) -> None:
    """Give the PReLU that `key` names (any key of its alias group) the slope `value`, on every key of the group: one shared tensor."""
    tab = param_table(VARIANTS[name])
    canon = tab.alias.get(key, key)
    t = torch.full((1,), float(value))
    for k in prelu_groups(name)[canon]:
        sd[k] = t


def edge_state_dict(name: str) -> "OrderedDict[str, torch.Tensor]":
    """synth_state_dict(name) with the canonical PReLU slopes, in sorted key order, cycling through EDGE_SLOPES (aliases keep sharing)."""
    sd = synth_state_dict(name)
    for i, canon in enumerate(sorted(prelu_groups(name))):
        set_slope(sd, name, canon, EDGE_SLOPES[i % len(EDGE_SLOPES)])
    return sd
