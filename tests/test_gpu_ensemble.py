"""-m gpu: ``GShiftNet.forward_ensemble_fp32_out`` against the composition made with public pieces -- torch's flip and transpose, ``forward_fp32_out``,
torch's sums -- bit for bit, on synthetic weights."""
import numpy as np
import pytest
import torch

from shiftnet_amd import ensemble, restore

pytestmark = pytest.mark.gpu

T, H, W = 6, 24, 40                      # two frames restored; non-square; legal for the padding of both topologies (multiples of 8)
MODULES = {"deblur_small-bf16": ("deblur_small", "bf16"), "denoise-bf16": ("denoise", "bf16"), "deblur_small-fp32": ("deblur_small", "fp32")}


def moved(a, op):
    """a: [T, C, H, W] -> the member's tensor, with torch's own ops: transpose first, then the flips, then time."""
    if op & 4:
        a = a.transpose(-1, -2)
    if op & 2:
        a = a.flip(-2)
    if op & 1:
        a = a.flip(-1)
    if op & 8:
        a = a.flip(0)
    return a.contiguous()


def back(r, op):
    """The inverse of ``moved`` on a member's result."""
    if op & 8:
        r = r.flip(0)
    if op & 1:
        r = r.flip(-1)
    if op & 2:
        r = r.flip(-2)
    if op & 4:
        r = r.transpose(-1, -2)
    return r.contiguous()


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


@pytest.fixture(scope="module", params=list(MODULES))
def case(request):
    """(net, the positional and keyword arguments of a forward as tensors [1, T, ., H, W], the plain result) -- made once per module."""
    variant, dtype = MODULES[request.param]
    net = restore.load_net(variant, "synthetic", dtype)
    dt = next(net.parameters()).dtype
    g = torch.Generator().manual_seed(len(request.param))
    x32 = torch.rand((1, T, 3, H, W), generator=g).cuda()
    x = x32.to(dt)
    plane = (0.02 + 0.1 * torch.rand((1, T, 1, H, W), generator=g)).cuda().to(dt) if net.V.denoise else None      # not flat: it must move with the frames
    shortcut = x32 if dt != torch.float32 else None
    with torch.no_grad():
        plain = forward(net, x, plane, shortcut)
    assert tuple(plain.shape) == (T - 4, 3, H, W) and plain.dtype == torch.float32
    return net, x, plane, shortcut, plain


def forward(net, x, plane, shortcut):
    args = (x,) if plane is None else (x, plane)
    return net.forward_fp32_out(*args, **({"shortcut": shortcut} if shortcut is not None else {}))


def composed(net, x, plane, shortcut, ops):
    total = None
    for op in ops:
        r = forward(net, moved(x[0], op)[None], moved(plane[0], op)[None] if plane is not None else None,
                    moved(shortcut[0], op)[None] if shortcut is not None else None)
        r = back(r, op)
        total = r.clone() if total is None else total + r                            # the sequential float32 sum in list order
    return total * (1.0 / len(ops))


def run(net, x, plane, shortcut, **kw):
    args = (x,) if plane is None else (x, plane)
    with torch.no_grad():
        return net.forward_ensemble_fp32_out(*args, **({"shortcut": shortcut} if shortcut is not None else {}), **kw)


@pytest.mark.parametrize("kw", [dict(ensemble=8, time=True), dict(ensemble=2)], ids=["8-time", "2"])
def test_the_ensemble_equals_the_composition_bit_for_bit_and_differs_from_the_plain_forward(case, kw):
    net, x, plane, shortcut, plain = case
    ops = ensemble.members(kw["ensemble"], kw.get("time", False))
    assert len(ops) == (16 if "time" in kw else 2)
    with torch.no_grad():
        want = composed(net, x, plane, shortcut, ops)
    got = run(net, x, plane, shortcut, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(plain.shape)
    differ = int((bits(got) != bits(want)).sum())
    print(f"{kw}: {differ} of {got.numel()} samples differ from the composition; max |ensemble - plain| = {float((got - plain).abs().max()):.3e}")
    assert differ == 0
    assert not np.array_equal(bits(got), bits(plain))                                # the network is not equivariant: the mean is not the plain result
    assert np.array_equal(bits(run(net, x, plane, shortcut, **kw)), bits(want))      # again, from the reused buffers
    assert getattr(net.prepare(), "fallbacks", 0) == 0                               # the range guard did not trip


def test_one_member_is_the_plain_forward(case):
    net, x, plane, shortcut, plain = case
    for e in (1, None):
        assert np.array_equal(bits(run(net, x, plane, shortcut, ensemble=e)), bits(plain))
    assert np.array_equal(bits(forward(net, x, plane, shortcut)), bits(plain))       # and the forward is repeatable, which everything above rests on


def test_a_flat_noise_level_is_the_same_for_every_member_and_illegal_arguments_are_refused(case):
    net, x, plane, shortcut, plain = case
    with pytest.raises(ValueError, match="ensemble"):
        run(net, x, plane, shortcut, ensemble=3)
    if plane is None:
        with pytest.raises(ValueError, match="x:\\[1,T,3,H,W\\]"):
            run(net, x[0], None, None, ensemble=2)
        return
    level = torch.full((1, 1, 1, 1, 1), 0.04, dtype=x.dtype, device="cuda")
    flat = level.expand(1, T, 1, H, W)
    with torch.no_grad():
        want = composed(net, x, flat, shortcut, list(range(8)))                      # moved() of a stride-0 expansion is the constant plane of the new shape
    assert np.array_equal(bits(run(net, x, flat, shortcut, ensemble=8)), bits(want))
    assert np.array_equal(bits(run(net, x, 0.04, shortcut, ensemble=8)), bits(want)) # a number
    with pytest.raises(ValueError, match="noise plane"):
        run(net, x, plane[:, :, :, :, :8], shortcut, ensemble=2)
