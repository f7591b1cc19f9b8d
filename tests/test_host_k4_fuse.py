"""Which GSTS units take the four-launch route (Engine.k4_fused: the CAB2's phase 2 inside the CAB1's phase 1) -- the predicate alone, no device."""
import os
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "shift-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _stub(**kw):
    from shiftnet_amd.engine import Engine

    class Stub:
        k4_fuse, phase1, fold_se, MAX_TICKETS, schedule = "1", "auto", True, 4096, "unit"
        _clip, split = 0, None
        V = SimpleNamespace(denoise=False)
        _fused_phase1, _fold_ok, k4_fused = Engine._fused_phase1, Engine._fold_ok, Engine.k4_fused
    s = Stub()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_default_route_is_fused_for_c64_deblur():
    assert _stub().k4_fused(20, 64)
    assert _stub(phase1="r").k4_fused(20, 64)


@pytest.mark.parametrize("kw,T,c", [
    (dict(k4_fuse="0"), 20, 64),                                  # the switch
    (dict(), 20, 80),                                             # C = 80 keeps five launches
    (dict(V=SimpleNamespace(denoise=True)), 20, 64),              # the denoisers' two passes
    (dict(phase1="0"), 20, 64),                                   # the bf16 chain (the range guard's fallback)
    (dict(MAX_TICKETS=2), 4, 64),                                 # no fold: the CAB2's scale comes from sn_ca_mlp
    (dict(fold_se=False), 20, 64),
    (dict(split=object()), 20, 64),                               # a temporally split window
    (dict(_clip=5), 20, 64),                                      # a batch of clips
    (dict(schedule="frame"), 20, 64),
    (dict(schedule="streams"), 20, 64),
])
def test_units_that_keep_five_launches(kw, T, c):
    assert not _stub(**kw).k4_fused(T, c)


def test_fp32_engine_is_never_fused():
    from shiftnet_amd.engine32 import Engine32
    assert Engine32.k4_fuse == "0"


def test_switch_value_is_validated(monkeypatch):
    from shiftnet_amd.engine import Engine
    monkeypatch.setattr(Engine, "k4_fuse", "yes")
    with pytest.raises(ValueError, match="SN_K4_FUSE"):
        Engine(SimpleNamespace(V=None, device=None))
