"""The fp32 engine beside the bf16 engine: what each class can reach of the library, by the class hierarchy alone -- and the two switch checks that
sit in the same block (the packed sn_conv_desc.flags, SN_CAB_FUSED).  No device."""
import inspect
import itertools
import os
import sys
import types
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "shift-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _reachable(classes):
    """The lib.SYMBOLS names among the string constants and attribute names of the code objects (nested ones included) of every function the classes define."""
    from shiftnet_amd import lib
    seen, names = set(), set()

    def walk(code):
        names.update(code.co_names)
        for c in code.co_consts:
            if isinstance(c, str):
                names.add(c)
            elif isinstance(c, types.CodeType):
                walk(c)
    for cls in classes:
        for v in vars(cls).values():
            v = getattr(v, "__func__", v)                    # staticmethod / classmethod
            v = getattr(v, "fget", v)                        # property
            if callable(v) and not isinstance(v, type):
                v = inspect.unwrap(v)                        # torch.no_grad(), contextlib.contextmanager
            if isinstance(v, types.FunctionType) and v.__code__ not in seen:
                seen.add(v.__code__)
                walk(v.__code__)
    return names & set(lib.SYMBOLS)


def test_engines_are_siblings_under_network():
    from shiftnet_amd.engine import Engine, Plan
    from shiftnet_amd.engine32 import Engine32, Plan32
    from shiftnet_amd.network import Network
    assert issubclass(Engine, Network) and issubclass(Engine32, Network)
    assert not issubclass(Engine32, Engine) and not issubclass(Engine, Engine32)
    assert not issubclass(Plan32, Plan) and not issubclass(Plan, Plan32)


def test_fp32_engine_reaches_no_bf16_entry_point():
    from shiftnet_amd.engine import Engine
    from shiftnet_amd.engine32 import Engine32
    from shiftnet_amd.network import Network
    assert _reachable([Network]) == {"sn_ca_mlp"}
    r32 = _reachable(Engine32.__mro__)
    assert {n for n in r32 if not n.startswith("sn32_")} == {"sn_ca_mlp", "sn_cab_ca_scratch_floats"}
    assert {n for n in r32 if n.startswith("sn32_")} >= {"sn32_conv2d", "sn32_cab_ca", "sn32_ingest", "sn32_gsts_gather"}    # the walk does see names
    r16 = _reachable(Engine.__mro__)
    assert not [n for n in r16 if n.startswith("sn32_")]
    assert r16 >= {"sn_conv2d", "sn_cab_fused", "sn_gsts_cab2_phase1", "sn_cab2_phase2_cab1_phase1", "sn_upsample2_add"}


def test_conv_flags_pack_as_the_bare_shifts_did_and_refuse_what_does_not_fit():
    from shiftnet_amd import lib as L
    for wgs, stream_all, res_regs, depth, dbg, s2 in itertools.product((0, 1, 7, 15), (False, True), (False, True), (0, 1, 3), (0, 1, 5, 7), (False, True)):
        want = (wgs << 4) | (256 if stream_all else 0) | (512 if res_regs else 0) | (depth << 10) | (dbg << 12)
        if s2:
            want |= 1 << 15
        assert L.conv_flags(wgs=wgs, stream_all=stream_all, res_regs=res_regs, depth=depth, dbg=dbg, s2_small=s2) == want
        assert L.conv_flags(wgs=wgs, depth=depth, dbg=dbg) == (wgs << 4) | (depth << 10) | (dbg << 12)      # the fused CAB's statistics pass
    assert L.conv_flags() == 0 and not L.conv_flags(wgs=15, stream_all=1, res_regs=1, depth=3, dbg=7, s2_small=1) & L.SN_CONV_TILE_KERNEL
    for bad in (dict(wgs=16), dict(depth=4), dict(dbg=8), dict(wgs=-1), dict(depth=-1), dict(dbg=-1)):
        with pytest.raises(ValueError, match="sn_conv_desc.flags"):
            L.conv_flags(**bad)


@pytest.mark.parametrize("value", ["", "x", "p8"])
def test_cab_fused_value_is_validated(monkeypatch, value):
    from shiftnet_amd.engine import Engine
    monkeypatch.setattr(Engine, "cab_fused", value)
    with pytest.raises(ValueError, match="SN_CAB_FUSED"):
        Engine(SimpleNamespace(V=None, device=None))
