"""Test-time self-ensemble: the network runs on mirrored, transposed and time-reversed copies of a window, every result is mapped back and the
results are averaged.  Not part of the upstream API.

Shift-Net is not equivariant under any of these: its grouped spatial shifts point in fixed directions and its temporal shift tells past from
future, so every copy gives another answer, and their mean is the ensemble's.  It needs no training and no other checkpoint; **a window costs M
forwards**, M the number of members.  **Nobody has measured what it gains on this network**: the +0.05 to +0.2 dB quoted for image
super-resolution is a figure from the literature for other networks, not a property of Shift-Net, and no trained checkpoint ships here.

A member is an ``op`` of ``sn_geo_transform`` (include/shiftnet_hip.h): bit 1 mirrors the columns, 2 the rows, 4 transposes (before the flips), 8
reverses time.  ``members`` lists them; ``forward_ensemble`` runs them.  The data movement is two kernels of csrc/sn_geo.hip: ``sn_geo_transform``
writes a member's input into buffers that are reused, ``sn_geo_accumulate`` maps its float32 result back and adds it into the float32 canvas; the
last launch multiplies by 1 / M, which is exact.  The transposed members have another input signature than the window itself: the engine keeps a
plan -- and, where a forward is replayed from a captured graph, a graph -- of its own for them.
"""
from __future__ import annotations

from typing import List

SPATIAL = (1, 2, 4, 8)             # the legal numbers of spatial members
REVERSE_T = 8                      # == lib.SN_GEO_REVERSE_T


def members(ensemble=8, time: bool = False) -> List[int]:
    """The ops of the ensemble's members in the order they are run and summed.  ``ensemble``: None or 1 -- the identity alone, ``[0]``; 2 -- and the
    mirrored columns, ``[0, 1]``; 4 -- and the mirrored rows and both, ``[0, 1, 2, 3]``; 8 -- and the transposes of those four, ``[0 .. 7]``.  With
    ``time`` the list is followed by the same ops on the window reversed in time (``op | 8``).  The identity comes first; the length is a power of two.
    Anything else -- another number, a bool, a string -- is a ValueError."""
    if ensemble is None:
        ensemble = 1
    if isinstance(ensemble, bool) or not isinstance(ensemble, int) or ensemble not in SPATIAL:
        raise ValueError(f"ensemble must be None, 1, 2, 4 or 8 (the number of mirrored / transposed members), got {ensemble!r}")
    ops = list(range(ensemble))
    return ops + [op | REVERSE_T for op in ops] if time else ops


class Buffers:
    """The reusable device buffers of ``forward_ensemble``: one flat tensor per name, grown when a larger shape asks and otherwise kept, so that a
    shape that has been seen allocates nothing and finds its tensors at the same addresses."""

    def __init__(self) -> None:
        self.flat = {}

    def reserve(self, torch, name: str, numel: int, dtype, device) -> None:
        have = self.flat.get(name)
        if have is None or have.numel() < numel or have.dtype != dtype or have.device != device:
            self.flat[name] = torch.empty(numel, dtype=dtype, device=device)

    def view(self, torch, name: str, shape, dtype, device):
        numel = 1
        for v in shape:
            numel *= int(v)
        self.reserve(torch, name, numel, dtype, device)
        return self.flat[name][:numel].view(*shape)


def is_flat(noise_map) -> bool:
    """A noise level that is one number everywhere: a number, or a tensor every dimension of which has size 1 or stride 0."""
    if isinstance(noise_map, (int, float)):
        return True
    return all(n == 1 or s == 0 for n, s in zip(noise_map.shape, noise_map.stride()))


def forward_ensemble(net, x, noise_map, shortcut, members, out=None, buffers=None, counts=None):
    """The mean of the network's float32 results over ``members`` (a list of ops that starts with the identity, as ``members()`` makes it).

    net: a GShiftNet on a HIP device; x: [1, T, 3, H, W] in its dtype; noise_map: None (deblur variants), a number or a stride-0 expansion (flat: it is
    invariant under every op and is re-expanded to the member's shape, which copies nothing), or [1, T, 1, H, W] (a plane: it is transformed with the
    frames); shortcut: None or the float32 twin of x, transformed as well.  -> ``out`` [T - past - future, 3, H, W] float32 (allocated where None).

    Member 0 runs on ``x`` itself and starts the canvas (``init``: whatever ``out`` held is not read).  Every other member: ``sn_geo_transform`` of x,
    of shortcut and of a plane into ``buffers``; ``net.forward_fp32_out``; ``sn_geo_accumulate`` with the member's op.  The scale is 1 except in the
    last launch, where it is 1 / M -- a power of two -- so the result is the sequential float32 sum in list order, divided by M.  All members share one
    range-guard check (``net.guard_scope()``); if it tripped the whole loop runs once more, into a canvas that ``init`` starts again.
    ``counts``: None or a dict whose ``"geo_transform"`` / ``"geo_accumulate"`` are raised by one per launch."""
    import torch
    from .io_edges import geo_accumulate, geo_out_shape, geo_transform
    members = [int(op) for op in members]
    M = len(members)
    if M < 1 or members[0] != 0 or M & (M - 1) or len(set(members)) != M or not all(0 <= op <= 15 for op in members):
        raise ValueError(f"forward_ensemble: members must be distinct ops 0 .. 15 that start with the identity, a power of two of them, got {members!r}")
    if not (isinstance(x, torch.Tensor) and x.dim() == 5 and x.shape[0] == 1):
        raise ValueError(f"forward_ensemble expects x:[1,T,3,H,W], got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    past, future = net.num_fb, net.num_ff
    _, T, C, H, W = x.shape
    n = T - past - future
    if n < 1:
        raise ValueError(f"forward_ensemble: a window of {T} frames restores none ({past} past and {future} future frames)")
    if past != future and any(op & REVERSE_T for op in members):
        raise ValueError(f"forward_ensemble: a time-reversed window is a legal window only where past_frames == future_frames, got {past} and {future}")
    if net.V.denoise and noise_map is None:
        raise TypeError("noise_map is required by the denoise variants")
    if not net.V.denoise:
        noise_map = None
    dev = x.device
    flat = noise_map is None or is_flat(noise_map)
    if noise_map is not None:
        if isinstance(noise_map, (int, float)):
            noise_map = torch.full((1, 1, 1, 1, 1), float(noise_map), dtype=x.dtype, device=dev)
        elif not flat and tuple(noise_map.shape) != (1, T, 1, H, W):
            raise ValueError(f"forward_ensemble: a noise plane must be [1, {T}, 1, {H}, {W}] like x, got {tuple(noise_map.shape)}")
        level = noise_map[(0,) * noise_map.dim()].view(1, 1, 1, 1, 1) if flat else None      # a view of one element: no copy
    if shortcut is not None and tuple(shortcut.shape) != tuple(x.shape):
        raise ValueError(f"shortcut must be [1,T,3,H,W] like x, got {tuple(shortcut.shape)}")
    x = x.contiguous()                                            # no copy where it is already (the restorer's tensors are)
    shortcut = shortcut.contiguous() if shortcut is not None else None
    plane = noise_map.contiguous() if not flat else None
    buffers = Buffers() if buffers is None else buffers
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device=dev)
    if tuple(out.shape) != (n, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"forward_ensemble: out must be a contiguous float32 [{n}, 3, {H}, {W}], got {tuple(out.shape)} {out.dtype}")

    def count(name: str) -> None:
        if counts is not None:
            counts[name] = counts.get(name, 0) + 1

    def member_input(op: int):
        """(x, noise_map, shortcut) of member ``op``: the window's own tensors for the identity, else their transforms in the reused buffers."""
        if op == 0:
            return x, noise_map, shortcut
        moved = []
        for name, a in (("x", x), ("plane", plane), ("shortcut", shortcut)):
            if a is None:
                moved.append(None)
                continue
            dst = buffers.view(torch, name, geo_out_shape(a.shape[1:], op), a.dtype, dev)
            moved.append(geo_transform(a[0], op, out=dst).unsqueeze(0))
            count("geo_transform")
        xm, nm, sc = moved
        if noise_map is not None and flat:
            nm = level.expand(1, *geo_out_shape((T, 1, H, W), op))
        return xm, nm, sc

    for _ in range(2):
        with net.guard_scope() as gs:
            for i, op in enumerate(members):
                xm, nm, sc = member_input(op)
                args = (xm,) if nm is None else (xm, nm)
                result = net.forward_fp32_out(*args, **({"shortcut": sc} if sc is not None else {}))
                geo_accumulate(result, out, op, init=(i == 0), scale=(1.0 / M if i == M - 1 else 1.0))
                count("geo_accumulate")
        if not gs.tripped:
            break
    return out
